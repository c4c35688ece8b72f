"""The nmse and weighted_mse losses of the Koopman training step (include/koopman_mpc.h
sim_koopman_trainer_set_loss / _get_loss; control/koopman_train.py loss_name=) against a numpy restatement
of the reference, for the DKUC and the bilinear DBKN trainers.

The reference's k_linear_loss (models/losses.py:54-129) applies BaseLoss(loss_name) (losses.py:35-52) to
four pairs per step i -- koopman (z^_{i+1}, Psi(x_{t0+i+1})), pred (z^_{i+1}[:x_dim], x_{t0+i+1}), dis and
angle (pred's columns < npos / >= npos) -- and sums them with beta_i = gamma^i over cont = sum beta_i:
    nmse          mse(preds, labels) / mean(labels^2) = sum (preds - labels)^2 / sum labels^2;
    weighted_mse  (mse(preds[:, :3], labels[:, :3]) + 9 mse(preds[:, 3:], labels[:, 3:])) / 10, the split at
                  column 3 of the pair's own slice: dis (npos columns) has no column past its third at the
                  default npos = 3 and is NaN -- the mean of an empty array, which the restatement takes
                  literally -- and angle is NaN when x_dim - npos <= 3.
`ref_loss_grad` is that forward and its hand-written backward (the rollout and its adjoint as in
test_koopman_train_bilinear.py, DKUC being the case without H) from the flat parameter vector; no product
code computes it.  With c_i = beta_i / cont, e = z^_{i+1} - Psi(x), ex its x columns:
    nmse          g_{i+1} = c_i 2 e / D^k_i (+ c_i 2 ex / D^p_i on the x columns), D^k_i = sum Psi(x)^2,
                  D^p_i = sum x^2; the label is not detached, so the target encode's output gradient is
                  c_i (-2 e_f / D^k_i - 2 N^k_i / (D^k_i)^2 z_f), N^k_i = sum e^2;
    weighted_mse  g_{i+1} = c_i 2 w(column) e with w = 1 / (30 n) for columns < 3 and 9 / (10 n (d - 3)) for the
                  others of a d-column pair (d = nz for koopman, x_dim for pred).
A CPU test checks the restatement against torch.autograd over a literal BaseLoss (F.mse_loss) on this
project's Koopmanlinear / KoopmanBlinear in float64.

Tolerances are test_koopman_train.py's rule, no new numbers: per test input the reference's own spread per
parameter block (max |float64 - longdouble| and max |float64 - reversed summation|, over the block's max)
is asserted below 1e-12, and the product is held to min(100 max(spread, 2.2e-16), 1e-9) of the block's max;
the losses that are not NaN likewise as an rtol, and the parameters after Adam steps.  Conditions on the
inputs, asserted by every reference with no sample excluded: min |hidden pre-activation| >= 1e-9, and every
nmse normaliser >= 1e-3 times its number of summands.

Measured over the GPU tests' inputs (both encoders, both models and u_z, n = 1 .. 130, P = 1 and 5): gradient
spreads <= 1.9e-15 per block (H: 1.2e-15), so the bars are 2.2e-14 .. 1.9e-13; loss spreads <= 5.6e-16 (bar <=
5.6e-14); parameter spreads after 1 and after 5 Adam steps <= 1.6e-14 per block (bars <= 1.6e-12); the least
pre-activation 7.8e-8, the least nmse normaliser 0.0195 per summand.
Measured on an MI355X against those bars: gradient error <= 2.2e-15 (H: 2.1e-15), at most 5.2% of its bar;
loss error <= 6.6e-16 (2.3%); parameter error <= 3.0e-14 (9.9%).  Every figure is printed beside its bar.
"""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import soarm_pkg  # noqa: F401
import test_koopman_train as tk
import test_koopman_train_bilinear as tb

LAYERS, LAYERS3 = tk.LAYERS, tk.LAYERS3
XD, UD, GAMMA = tk.XD, tk.UD, tk.GAMMA
BETA1, BETA2, EPS = tk.BETA1, tk.BETA2, tk.EPS
SPREAD, BAR, F64EPS, PRE_MIN, SENTINEL, T = tk.SPREAD, tk.BAR, tk.F64EPS, tk.PRE_MIN, tk.SENTINEL, tk.T
DEN_MIN = 1e-3  # an nmse normaliser per summand
LOSSES = ("nmse", "weighted_mse")
KLOSS = {"mse": 0, "nmse": 1, "weighted_mse": 2}
DKUC, DBKN = "dkuc", "dbkn"


# ------------------------------------------------------------------------------------ the reference
def blocks(model, layers):
    return tb.blocks(layers) if model == DBKN else tk.blocks(layers)


def ref_loss_grad(p, model, layers, u_z, loss, npos, x, u, P, dt=np.float64, reverse=False):
    """x [P+1, n, x_dim], u [P, n, u_dim] (float32 data, widened) -> (losses [6], grad [nparam], min |hidden
    pre-activation|, min nmse normaliser per summand) in dtype dt.  reverse: every contraction, the sum over c
    and every loss sum in the opposite order."""
    fl = (lambda a, ax: np.ascontiguousarray(np.flip(a, ax))) if reverse else (lambda a, ax: a)

    def mm(a, b):  # a [m, k] @ b [k, q]
        return fl(a, 1) @ fl(b, 0)

    def tot(a):  # the sum of all entries
        return (np.ascontiguousarray(a.ravel()[::-1]) if reverse else a).sum(dtype=dt)

    def mean(a):  # (the mean of no entry is NaN, as torch's)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return dt(np.mean(np.ascontiguousarray(a.ravel()[::-1]) if reverse else a, dtype=dt))

    nlin = tk.blocks(layers)[-1][2]
    Ws, bs, A, B = [[w.astype(dt) for w in g] if isinstance(g, list) else g.astype(dt) for g in tk.unpack(p[:nlin], layers)]
    nl, n, nz = len(Ws), x.shape[1], A.shape[0]
    Hc = tb.h_blocks(p[nlin:].astype(dt).reshape(nz, nz * UD), u_z) if model == DBKN else []
    cs = list(range(len(Hc)))[::-1] if reverse else list(range(len(Hc)))
    x, u = x.astype(dt), u.astype(dt)
    premin, denmin = [np.inf], [np.inf]

    def psi(xx):
        acts, h = [xx], xx
        for l in range(nl):
            pre = mm(h, Ws[l].T) + bs[l]
            if l + 1 < nl:
                premin[0] = min(premin[0], float(np.abs(pre).min()))
                h = np.maximum(pre, 0)
            else:
                h = pre
            acts.append(h)
        return np.concatenate([xx, h], -1), acts

    def psi_backward(acts, gam, dW, db):
        d = gam
        for l in range(nl - 1, -1, -1):
            dW[l] += mm(d.T, acts[l])
            db[l] += fl(d, 0).sum(0)
            if l > 0:
                d = mm(d, Ws[l]) * (acts[l] > 0)

    def base(pred, lab):
        """BaseLoss(pred, lab) and its gradients (with respect to pred, with respect to lab)"""
        d = pred - lab
        if loss == "nmse":
            N, D = tot(d * d), tot(lab * lab)
            denmin[0] = min(denmin[0], float(D) / lab.size)
            return N / D, 2 * d / D, -2 * d / D - 2 * (N / (D * D)) * lab
        w = np.empty(lab.shape[1], dt)
        with np.errstate(divide="ignore"):
            w[:3], w[3:] = dt(1) / (30 * n), dt(9) / (10 * dt(n) * (lab.shape[1] - 3))
        return (mean(d[:, :3] ** 2) + 9 * mean(d[:, 3:] ** 2)) / 10, 2 * w * d, -2 * w * d

    beta = [dt(GAMMA) ** i for i in range(P)]
    cont = sum(beta)
    z0, acts0 = psi(x[0])
    zh, g, enc = [z0], [None], []
    sk = sp = sd = sa = dt(0)
    for i in range(P):
        zn = mm(zh[i], A.T) + mm(u[i], B.T)
        for c in cs:
            zn = zn + mm(u[i][:, c:c + 1] * zh[i], Hc[c].T)
        zt, acts = psi(x[i + 1])
        lk, gk, gz = base(zn, zt)
        lp, gp, _ = base(zn[:, :XD], x[i + 1])
        sk += beta[i] * lk
        sp += beta[i] * lp
        sd += beta[i] * base(zn[:, :npos], x[i + 1][:, :npos])[0]
        sa += beta[i] * base(zn[:, npos:XD], x[i + 1][:, npos:])[0]
        c_i = beta[i] / cont
        gi = c_i * gk
        gi[:, :XD] += c_i * gp
        enc.append((acts, c_i * gz[:, XD:]))  # (the x columns of the label are data)
        zh.append(zn), g.append(gi)
    koop, pred = sk / cont, sp / cont
    losses = np.array([koop + pred, koop, pred, dt(0), sd / cont, sa / cont], dt)
    dW, db = [np.zeros_like(w) for w in Ws], [np.zeros_like(b) for b in bs]
    dA, dB, dHc = np.zeros_like(A), np.zeros_like(B), [np.zeros_like(A) for _ in Hc]
    lam = g[P]
    for i in range(P - 1, -1, -1):
        dA += mm(lam.T, zh[i])
        dB += mm(lam.T, u[i])
        nxt = mm(lam, A)
        for c in cs:
            uc = u[i][:, c:c + 1]
            dHc[c] += mm(lam.T, uc * zh[i])
            nxt = nxt + uc * mm(lam, Hc[c])
        lam = nxt + (g[i] if i > 0 else 0)
    for acts, gam in enc:
        psi_backward(acts, gam, dW, db)
    psi_backward(acts0, lam[:, XD:], dW, db)
    parts = [np.concatenate([w.ravel(), b]) for w, b in zip(dW, db)] + [dA.ravel(), dB.ravel()]
    if model == DBKN:
        dH = np.zeros((nz, nz * UD), dt)
        for c in range(UD):
            if u_z:
                dH[:, c * nz:(c + 1) * nz] = dHc[c]
            else:
                dH[:, c::UD] = dHc[c]
        parts.append(dH.ravel())
    return losses, np.concatenate(parts), premin[0], denmin[0]


def nan_pattern(loss, npos):
    """which of the six losses are NaN: under weighted_mse a slice of three columns or fewer"""
    return [False] * 4 + [loss == "weighted_mse" and npos <= 3, loss == "weighted_mse" and XD - npos <= 3]


def loss_spread(l64, others, loss, npos):
    """max relative spread over the losses that are neither NaN nor recon; asserts the NaN pattern of each"""
    nan = nan_pattern(loss, npos)
    keep = [k for k in (0, 1, 2, 4, 5) if not nan[k]]
    for o in (l64,) + tuple(others):
        assert np.isnan(o.astype(np.float64)).tolist() == nan, (o, nan)
    return max(float(np.abs((l64[keep] - o[keep].astype(np.float64)) / l64[keep]).max()) for o in others), keep


def assert_losses(got, want, ls, loss, npos, what="losses"):
    nan = nan_pattern(loss, npos)
    keep = [k for k in (0, 1, 2, 4, 5) if not nan[k]]
    assert got[3] == 0.0
    assert np.isnan(got).tolist() == nan, (got, nan)
    lerr = float(np.abs((got[keep] - want[keep]) / want[keep]).max())
    lbar = min(100 * max(ls, F64EPS), BAR)
    print(f"{what}: err {lerr:.2e} bar {lbar:.2e} spread {ls:.2e}")
    assert lerr <= lbar


def make_net(model, seed, layers, u_z):
    return tb.make_net(seed, layers, u_z) if model == DBKN else tk.make_net(seed, layers)


_REF = {}


def reference(model, layers, n, P, t0, use_idx, u_z, loss, npos=3, seed=1):
    """(rows, idx or None, params, losses f64, grad f64, grad spread per block, loss spread), computed once
    per case and shared.  The conditions on the inputs are asserted here."""
    key = (model, layers, n, P, t0, use_idx, u_z, loss, npos, seed)
    if key not in _REF:
        from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net
        N = n + 5 if use_idx else n
        rows = tk.make_rows(N, seed + 10)
        idx = tk.make_idx(n, N, seed + 20) if use_idx else None
        p = params_from_net(make_net(model, seed, layers, u_z))
        x, u = tk.window(rows, idx if use_idx else np.arange(n), t0, P)
        l64, g64, premin, denmin = ref_loss_grad(p, model, layers, u_z, loss, npos, x, u, P)
        assert premin >= PRE_MIN, f"a hidden pre-activation of {premin:.2e} is within rounding of zero: change the seed"
        assert denmin >= DEN_MIN, f"an nmse normaliser of {denmin:.2e} per summand: change the seed"
        lld, gld, _, _ = ref_loss_grad(p, model, layers, u_z, loss, npos, x, u, P, np.longdouble)
        lrv, grv, _, _ = ref_loss_grad(p, model, layers, u_z, loss, npos, x, u, P, reverse=True)
        bl = blocks(model, layers)
        gs = tb.block_spread(bl, g64, [gld, grv])
        ls, _ = loss_spread(l64, (lld, lrv), loss, npos)
        assert ls < SPREAD, f"reference loss spread {ls:.2e}"
        print(f"reference {key}: premin {premin:.2e} denmin {denmin:.2e} loss spread {ls:.2e} grad spread {max(gs.values()):.2e}")
        for a in (rows, p, l64, g64):
            a.setflags(write=False)
        _REF[key] = (rows, idx, p, l64, g64, gs, ls)
    return _REF[key]


# ------------------------------------------------------------------------------------------- CPU
def torch_losses(net, x, u, P, loss, npos):
    """k_linear_loss's six values with a literal BaseLoss, on this project's net (float64 torch)"""
    import torch
    import torch.nn.functional as F

    def base(preds, labels):
        if loss == "nmse":
            return F.mse_loss(preds, labels) / torch.square(labels).mean()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return (F.mse_loss(preds[:, :3], labels[:, :3]) + 9 * F.mse_loss(preds[:, 3:], labels[:, 3:])) / 10

    beta = [GAMMA ** i for i in range(P)]
    cont = sum(beta)
    z = net.x_encoder(x[0])
    koop = pred = recon = dis = ang = 0.0
    for i in range(P):
        z = net.koopman_operation(z, u[i])
        x1, xp = x[i + 1], net.x_decoder(z)
        z1 = net.x_encoder(x1)
        recon = recon + beta[i] * base(net.x_decoder(z1), x1)
        koop = koop + beta[i] * base(z, z1)
        dis = dis + beta[i] * base(xp[:, :npos], x1[:, :npos])
        ang = ang + beta[i] * base(xp[:, npos:], x1[:, npos:])
        pred = pred + beta[i] * base(xp, x1)
    return [(koop + pred + recon) / cont, koop / cont, pred / cont, recon / cont, dis / cont, ang / cont]


CPU_CASES = [(m, uz, layers, n, P, loss, 3) for m, uz in ((DKUC, 0), (DBKN, 0), (DBKN, 1))
             for layers, n, P in ((LAYERS, 17, 5), (LAYERS3, 5, 1), (LAYERS, 1, 5)) for loss in LOSSES]
CPU_CASES += [(DKUC, 0, LAYERS3, 5, 5, "weighted_mse", 4), (DBKN, 1, LAYERS3, 5, 5, "weighted_mse", 5)]


@pytest.mark.parametrize("model,u_z,layers,n,P,loss,npos", CPU_CASES,
                         ids=[f"{c[0]}-uz{c[1]}-{'ref' if c[2] is LAYERS else 'nl3'}-n{c[3]}-P{c[4]}-{c[5]}-npos{c[6]}"
                              for c in CPU_CASES])
def test_reference_gradient_equals_autograd(model, u_z, layers, n, P, loss, npos):
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net
    rows, _, p, l64, g64, _, _ = reference(model, layers, n, P, 1, False, u_z, loss, npos)
    net = make_net(model, 1, layers, u_z)
    x, u = tk.window(rows, np.arange(n), 1, P)
    net.zero_grad()
    six = torch_losses(net, torch.as_tensor(x.astype(np.float64)), torch.as_tensor(u.astype(np.float64)), P, loss, npos)
    six[0].backward()
    gnet = (tb.make_net if model == DBKN else tk.make_net).__wrapped__(*((1, layers, u_z) if model == DBKN else (1, layers)))
    with torch.no_grad():  # a second net to carry the gradients as parameters
        for a, b in zip(gnet.parameters(), net.parameters()):
            a.copy_(b.grad if b.grad is not None else torch.zeros_like(b))
    want = params_from_net(gnet)
    net.zero_grad()
    t6 = np.array([float(v.detach()) for v in six])
    assert abs(t6[0] - l64[0]) <= 1e-13 * abs(l64[0])
    nan = nan_pattern(loss, npos)
    assert np.isnan(t6).tolist() == nan == np.isnan(l64).tolist()  # dis is NaN at npos = 3 under weighted_mse, finite at 4
    assert abs(t6[3]) <= 1e-30 and l64[3] == 0.0                   # recon: lC Psi(x) = x
    for k in (1, 2, 4, 5):
        assert nan[k] or abs(t6[k] - l64[k]) <= 1e-13 * abs(l64[k]), k
    assert want.size == g64.size
    for name, s, e in blocks(model, layers):
        scale = np.abs(want[s:e]).max()
        assert scale > 0 and np.abs(g64[s:e] - want[s:e]).max() <= 1e-12 * scale, name


def test_loss_entry_points_are_exported():
    import os
    from lerobot_mujoco_sim2real_amd import abi, build
    for name in ("sim_koopman_trainer_set_loss", "sim_koopman_trainer_get_loss"):
        assert name in abi.EXPORTS
    header = open(os.path.join(os.path.dirname(abi.PKG_DIR), "include", "koopman_mpc.h")).read()
    assert "int sim_koopman_trainer_set_loss(sim_koopman_trainer* tr, int loss);" in header
    assert "int sim_koopman_trainer_get_loss(const sim_koopman_trainer* tr);" in header
    for name, v in KLOSS.items():
        assert f"#define SIM_KLOSS_{name.upper()} {v}" in header and abi.KLOSS[name] == v
    build.build()
    lib = abi.load_lib()
    assert len(lib.sim_koopman_trainer_set_loss.argtypes) == 2 and len(lib.sim_koopman_trainer_get_loss.argtypes) == 1
    assert lib.sim_koopman_trainer_set_loss(None, KLOSS["nmse"]) == abi.E_ARG
    assert lib.sim_koopman_trainer_get_loss(None) == abi.E_ARG
    assert C.sizeof(abi.KoopmanTrainOpts) == 48  # the loss is the trainer's, not the options'


def test_loss_names_accepted_and_refused():
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import BilinearKoopmanTrainer, KoopmanTrainer
    for cls, net in ((KoopmanTrainer, tk.make_net()), (BilinearKoopmanTrainer, tb.make_net())):
        for bad in ("huber", "mae", "NMSE"):
            with pytest.raises(NotImplementedError, match="'mse', 'nmse', 'weighted_mse'"):
                cls(net, 16, loss_name=bad)
        if not torch.cuda.is_available():  # a built name gets as far as the device
            for name in LOSSES:
                with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
                    cls(net, 16, loss_name=name)


# ------------------------------------------------------------------------------------------- GPU
def _trainer(model, layers=LAYERS, max_batch=130, P=5, u_z=0, loss="mse", npos=3, seed=1, hscale=tb.HSCALE):
    from lerobot_mujoco_sim2real_amd.control.koopman_train import BilinearKoopmanTrainer, KoopmanTrainer
    kw = dict(pre_length=P, npos=npos, gamma=GAMMA, betas=(BETA1, BETA2), eps=EPS, loss_name=loss)
    if model == DBKN:
        return BilinearKoopmanTrainer(tb.make_net(seed, layers, u_z, hscale), max_batch, **kw)
    return KoopmanTrainer(tk.make_net(seed, layers), max_batch, **kw)


def _cases():
    """(loss, model, layers, n, P, last, u_z, use_idx, alt, npos): every (loss, model, encoder, n, P) once, the
    four alternatives as parities of the indices so that each value of each meets every n, both P, both
    encoders, both models and both losses; then weighted_mse at npos = 4 (dis and angle finite) and 5 (angle
    NaN)."""
    ns, out = (1, 16, 17, 65, 130), []
    for li, loss in enumerate(LOSSES):
        for mi, model in enumerate((DKUC, DBKN)):
            for ei, layers in enumerate((LAYERS, LAYERS3)):
                for k, n in enumerate(ns):
                    for pi, P in enumerate((1, 5)):
                        out.append((loss, model, layers, n, P, (pi + ei + (k >> 1) + li) % 2, (k + pi + ei + li) % 2,
                                    (k + pi + mi) % 2, (k + ei + mi + li) % 2, 3))
    for j, name in ((5, "last"), (6, "u_z"), (7, "use_idx"), (8, "alt")):  # the coverage the docstring promises
        for v in (0, 1):
            for loss in LOSSES:
                for model in (DKUC, DBKN):
                    got = [c for c in out if c[j] == v and c[0] == loss and c[1] == model]
                    assert {c[3] for c in got} == set(ns) and {c[4] for c in got} == {1, 5}, (name, v, loss, model)
                    assert {c[2] for c in got} == {LAYERS, LAYERS3}, (name, v, loss, model)
    out.append(("weighted_mse", DKUC, LAYERS, 65, 5, 0, 0, 1, 0, 4))
    out.append(("weighted_mse", DBKN, LAYERS3, 17, 5, 1, 1, 0, 1, 5))
    return out


CASES = _cases()


@pytest.mark.gpu
@pytest.mark.parametrize("loss,model,layers,n,P,last,u_z,use_idx,alt,npos", CASES,
                         ids=[f"{c[0]}-{c[1]}-{'ref' if c[2] is LAYERS else 'nl3'}-n{c[3]}-P{c[4]}-{'tail' if c[5] else 't0'}-uz{c[6]}-"
                              f"{'idx' if c[7] else 'all'}-{'ld16' if c[8] else 'ld13'}-npos{c[9]}" for c in CASES])
def test_loss_grad_matches_reference(loss, model, layers, n, P, last, u_z, use_idx, alt, npos):
    """n: one lane, a full wave, one past it (nmse: the normaliser crosses waves), one past a workgroup (it
    crosses workgroups), several workgroups; the window at row 0 and ending on row T; u_z, traj_idx NULL / a
    permutation with a repeat into a larger N, and the in-place / ld = 16 layout alternate (see _cases)."""
    t0 = T - P if last else 0
    rows, idx, p, l64, g64, gs, ls = reference(model, layers, n, P, t0, bool(use_idx), u_z, loss, npos)
    tr = _trainer(model, layers, 130, P, u_z, loss, npos)
    assert tr.loss_name == loss and tr.nparam == p.size and np.array_equal(tr.get_params(), p)
    r, *layout = tk.relayout(rows) if alt else (rows, 13, UD, 0)
    losses, grad = tk._loss_grad(tr, r, idx, t0, tuple(layout))
    assert_losses(losses, l64, ls, loss, npos)
    tb.assert_blocks(blocks(model, layers), grad, g64, gs, "grad")
    assert np.array_equal(tr.get_params(), p)  # loss_grad changes no state


STEPS = tk.STEPS


@functools.lru_cache(maxsize=None)
def adam_reference(model, layers, n, nsteps, u_z, loss, seed=1):
    """parameters after 1 .. nsteps reference steps in float64, and their spread per block against the same
    steps in longdouble and with reversed sums"""
    rows, idx, p0, *_ = reference(model, layers, n, 5, 0, True, u_z, loss, 3, seed)
    runs = []
    for dt, rev in ((np.float64, False), (np.longdouble, False), (np.float64, True)):
        p, m, v, traj = p0.astype(dt), np.zeros_like(p0, dtype=dt), np.zeros_like(p0, dtype=dt), []
        for t, (t0, lr) in enumerate(STEPS[:nsteps], 1):
            x, u = tk.window(rows, idx, t0, 5)
            _, g, premin, denmin = ref_loss_grad(p, model, layers, u_z, loss, 3, x, u, 5, dt, rev)
            assert premin >= PRE_MIN and denmin >= DEN_MIN
            p, m, v = tk.ref_adam(p, m, v, g, t, lr)
            traj.append(p)
        runs.append(traj)
    bl = blocks(model, layers)
    return rows, idx, [(runs[0][k], tb.block_spread(bl, runs[0][k], [runs[1][k], runs[2][k]])) for k in range(nsteps)]


@pytest.mark.gpu
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("model,u_z", [(DKUC, 0), (DBKN, 1)])
def test_train_steps_match_reference_adam(model, u_z, loss):
    import torch
    n, layers = 65, LAYERS
    rows, idx, want = adam_reference(model, layers, n, 5, u_z, loss)
    tr = _trainer(model, layers, n, 5, u_z, loss)
    r = torch.as_tensor(np.array(rows), device=tr.device)
    ix = torch.as_tensor(idx, device=tr.device)
    bl = blocks(model, layers)
    for k, (t0, lr) in enumerate(STEPS):
        tr.step(r, ix, t0, lr)
        if k in (0, 4):
            tb.assert_blocks(bl, tr.get_params(), want[k][0], want[k][1], f"params after {k + 1} steps")
    # the fragment copies follow the master vector: the next gradient is that of the updated parameters
    p5 = tr.get_params()
    x, u = tk.window(rows, idx, 1, 5)
    l64, g64, premin, denmin = ref_loss_grad(p5, model, layers, u_z, loss, 3, x, u, 5)
    assert premin >= PRE_MIN and denmin >= DEN_MIN
    losses, grad = tr.loss_grad(r, ix, 1)
    others = [ref_loss_grad(p5, model, layers, u_z, loss, 3, x, u, 5, np.longdouble),
              ref_loss_grad(p5, model, layers, u_z, loss, 3, x, u, 5, reverse=True)]
    tb.assert_blocks(bl, grad.cpu().numpy(), g64, tb.block_spread(bl, g64, [o[1] for o in others]), "grad after 5 steps")
    ls, _ = loss_spread(l64, [o[0] for o in others], loss, 3)
    assert_losses(losses.cpu().numpy(), l64, ls, loss, 3, "losses after 5 steps")


@pytest.mark.gpu
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("model,u_z", [(DKUC, 0), (DBKN, 1)])
def test_bitwise_reproducible_and_keeps_to_its_buffers(model, u_z, loss):
    import torch
    rows, idx, p0, *_ = reference(model, LAYERS, 130, 5, 2, True, u_z, loss)
    tr = _trainer(model, LAYERS, 130, 5, u_z, loss)
    l1, g1 = tk._loss_grad(tr, rows, idx, 2, pad=64)
    l2, g2 = tk._loss_grad(tr, rows, idx, 2, pad=64)
    assert l1.tobytes() == l2.tobytes() and g1.tobytes() == g2.tobytes()
    assert np.all(g1[tr.nparam:] == SENTINEL) and not np.any(g1[:tr.nparam] == SENTINEL)
    # grad and losses may be NULL
    r = torch.as_tensor(np.array(rows), device=tr.device)
    ix = torch.as_tensor(idx, device=tr.device)
    assert tr.lib.sim_koopman_loss_grad(tr._h, 130, rows.shape[1], T, C.c_void_p(r.data_ptr()), 13, UD, 0,
                                        C.c_void_p(ix.data_ptr()), 0, None, None, tr._stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(tr.get_params(), p0)
    # queued steps equal synchronised steps
    a, b = tr, _trainer(model, LAYERS, 130, 5, u_z, loss)
    la, lb = [], []
    for t0, lr in STEPS:
        la.append(a.step(r, ix, t0, lr))
    for t0, lr in STEPS:
        lb.append(b.step(r, ix, t0, lr))
        torch.cuda.synchronize()
    pa, pb = a.get_params(), b.get_params()
    assert pa.tobytes() == pb.tobytes() and not np.array_equal(pa, p0)
    assert torch.stack(la).cpu().numpy().tobytes() == torch.stack(lb).cpu().numpy().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("model,u_z", [(DKUC, 0), (DBKN, 1)])
def test_no_leakage_between_losses(model, u_z):
    """nmse -> weighted_mse -> mse on one trainer: the last equals a fresh trainer's mse loss_grad byte for byte"""
    rows, idx, p0, *_ = reference(model, LAYERS, 130, 5, 1, True, u_z, "nmse")
    tr, fresh = _trainer(model, LAYERS, 130, 5, u_z), _trainer(model, LAYERS, 130, 5, u_z)
    lib = tr.lib
    assert lib.sim_koopman_trainer_get_loss(tr._h) == 0 and tr.loss_name == "mse"
    seen = {}
    for name in ("nmse", "weighted_mse", "mse"):
        assert lib.sim_koopman_trainer_set_loss(tr._h, KLOSS[name]) == 0
        assert lib.sim_koopman_trainer_get_loss(tr._h) == KLOSS[name] and tr.loss_name == name
        seen[name] = tk._loss_grad(tr, rows, idx, 1)
        assert np.array_equal(tr.get_params(), p0)
    lf, gf = tk._loss_grad(fresh, rows, idx, 1)
    assert seen["mse"][0].tobytes() == lf.tobytes() and seen["mse"][1].tobytes() == gf.tobytes()
    for name in LOSSES:  # (and the other two were not the mse step)
        assert not np.array_equal(seen[name][1], gf)
        _, _, _, l64, g64, gs, ls = reference(model, LAYERS, 130, 5, 1, True, u_z, name)
        assert_losses(seen[name][0], l64, ls, name, 3, f"{name} after set_loss")
        tb.assert_blocks(blocks(model, LAYERS), seen[name][1], g64, gs, f"{name} grad after set_loss")


@pytest.mark.gpu
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("u_z", [0, 1])
def test_zero_h_equals_the_linear_trainer(u_z, loss):
    """H = 0: DBKN is DKUC.  Losses and the W, b, A, B gradient blocks are those of KoopmanTrainer under the
    same loss on the same linear part and inputs, bit for bit (the H terms add exact zeros)."""
    from lerobot_mujoco_sim2real_amd.control.koopman_train import KoopmanTrainer, params_to_net
    n, P, t0 = 65, 5, 1
    rows, idx, p, l64, g64, gs, ls = reference(DBKN, LAYERS, n, P, t0, True, u_z, loss)
    tb_ = _trainer(DBKN, LAYERS, 130, P, u_z, loss, hscale=0.0)
    nlin = tk.blocks(LAYERS)[-1][2]
    pz = tb_.get_params()
    assert not pz[nlin:].any()
    lin = params_to_net(np.array(pz[:nlin]), tk.make_net.__wrapped__(5, LAYERS))
    tl = KoopmanTrainer(lin, 130, pre_length=P, npos=3, gamma=GAMMA, betas=(BETA1, BETA2), eps=EPS, loss_name=loss)
    ll, gl = tk._loss_grad(tl, rows, idx, t0)
    lb, gb = tk._loss_grad(tb_, rows, idx, t0)
    assert np.array_equal(lb, ll, equal_nan=True)
    assert np.array_equal(gb[:nlin], gl) and np.abs(gb[nlin:]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("model", [DKUC, DBKN])
def test_train_end_to_end(model, loss):
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net, train
    from lerobot_mujoco_sim2real_amd.control.MPC_Controler import MPCController
    net = tk.make_net.__wrapped__(2, LAYERS) if model == DKUC else tb.make_net.__wrapped__(2, LAYERS, 0, 0.0)
    p0 = params_from_net(net)
    rows = torch.as_tensor(tk.make_rows(40, 5), device=torch.device("cuda", 0))
    hist = train(net, rows, epochs=2, batch_size=32, lr=1e-3, seed=3, eval_interval=1, loss_name=loss)
    tl = np.array(hist["train_loss"])
    assert tl.shape == (2, 6) and np.isnan(tl).tolist() == [nan_pattern(loss, 3)] * 2 and np.all(tl[:, 3] == 0)
    assert len(hist["eval"]) == 2 and hist["best_epoch"] in (0, 1) and np.isfinite(hist["best_error"])
    assert np.array_equal(params_from_net(net), hist["best_params"]) and not np.array_equal(hist["best_params"], p0)
    assert np.all(np.isfinite(hist["best_params"]))

    class args:  # noqa: N801
        x_dim, u_dim, MPC_type = XD, UD, "delta_mpc"
    ctl = MPCController(net, args)
    e = ctl.evaluate(rows)
    assert np.isfinite(e["avg_error"]) and e["avg_error"] == pytest.approx(hist["best_error"], rel=1e-12)


@pytest.mark.gpu
def test_set_loss_refusals():
    import torch
    from lerobot_mujoco_sim2real_amd import abi
    from lerobot_mujoco_sim2real_amd.control.koopman import Koopmanlinear
    from lerobot_mujoco_sim2real_amd.control.koopman_train import KoopmanTrainer
    rows, idx, p0, l64, g64, gs, ls = reference(DKUC, LAYERS, 17, 5, 0, False, 0, "nmse")
    tr = _trainer(DKUC, LAYERS, 130, 5, 0, "nmse")
    lib = tr.lib
    for bad in (3, -1, 100):  # an unknown id: refused, and the trainer still runs nmse
        assert lib.sim_koopman_trainer_set_loss(tr._h, bad) == abi.E_ARG and b"loss" in lib.sim_last_error()
        assert lib.sim_koopman_trainer_get_loss(tr._h) == KLOSS["nmse"]
    losses, grad = tk._loss_grad(tr, rows, idx, 0)
    assert_losses(losses, l64, ls, "nmse", 3)
    tb.assert_blocks(blocks(DKUC, LAYERS), grad, g64, gs, "grad after a refused set_loss")
    # weighted_mse splits x at column 3: x_dim = 3 is refused, through the C ABI and through Python
    torch.manual_seed(4)
    small = Koopmanlinear(3, UD, [3, 64, 24]).double()
    with pytest.raises(ValueError, match="x_dim >= 4"):
        KoopmanTrainer(small, 16, npos=1, loss_name="weighted_mse")
    ts, fresh = KoopmanTrainer(small, 16, npos=1), KoopmanTrainer(small, 16, npos=1)
    assert lib.sim_koopman_trainer_set_loss(ts._h, KLOSS["weighted_mse"]) == abi.E_ARG
    assert b"x_dim" in lib.sim_last_error() and lib.sim_koopman_trainer_get_loss(ts._h) == KLOSS["mse"]
    r3 = np.random.default_rng(3).uniform(-0.5, 0.5, (T + 1, 16, UD + 3)).astype(np.float32)
    r3 = torch.as_tensor(r3, device=ts.device)
    (la, ga), (lb, gb) = ts.loss_grad(r3, None, 1), fresh.loss_grad(r3, None, 1)
    assert torch.equal(la, lb) and torch.equal(ga, gb) and bool(torch.isfinite(ga).all())  # its mse step, untouched
    assert lib.sim_koopman_trainer_set_loss(ts._h, KLOSS["nmse"]) == 0  # nmse has no such limit
    ln, gn = ts.loss_grad(r3, None, 1)
    assert bool(torch.isfinite(ln).all()) and bool(torch.isfinite(gn).all()) and not torch.equal(gn, ga)
