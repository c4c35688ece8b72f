"""The float64 reference of the Koopman training step, for every model and loss, and what the tests of
test_koopman_train*.py share.  Not collected: it holds no test.

The reference (train(), train.py:89-266, over k_linear_loss, models/losses.py:54-129, with torch.optim.Adam):
n windows of P = pre_length steps; z^_0 = Psi(x_t0), and with H_c (nz x nz) the block of H that multiplies
u_c z -- columns c nz + j for u_z = 1, columns j u_dim + c for u_z = 0; DKUC has no H (models/KoopmanBase.py:62-78)
    forward   z^_{i+1} = A z^_i + B u_i + sum_c H_c (u_{i,c} z^_i)
    reverse   dH_c += lambda_{i+1} (u_{i,c} z^_i)'   (beside dA, dB)
              lambda_i = g_i + A' lambda_{i+1} + sum_c u_{i,c} (H_c' lambda_{i+1}).
BaseLoss(loss_name) (losses.py:35-52) is applied to four pairs per step i -- koopman (z^_{i+1}, Psi(x_{t0+i+1})),
pred (z^_{i+1}[:x_dim], x_{t0+i+1}), dis and angle (pred's columns < npos / >= npos) -- and summed with
beta_i = gamma^i over cont = sum beta_i; total = koopman + pred (recon is identically 0: lC Psi(x) = x):
    mse           the mean of (preds - labels)^2;
    nmse          mse(preds, labels) / mean(labels^2) = sum (preds - labels)^2 / sum labels^2;
    weighted_mse  (mse(preds[:, :3], labels[:, :3]) + 9 mse(preds[:, 3:], labels[:, 3:])) / 10, the split at
                  column 3 of the pair's own slice: dis (npos columns) has no column past its third at the
                  default npos = 3 and is NaN -- the mean of an empty array, which the restatement takes
                  literally -- and angle is NaN when x_dim - npos <= 3.
`ref_loss_grad` is that forward and its hand-written backward in numpy from the flat parameter vector
[W_0 | b_0 | ... | A | B (| H)]; `ref_adam` the update; no product code computes them.  With c_i = beta_i / cont,
e = z^_{i+1} - Psi(x), ex its x columns, n d the entries of a d-column pair (d = nz for koopman, x_dim for pred):
    mse           g_{i+1} = c_i 2 e / (n nz) (+ c_i 2 ex / (n x_dim) on the x columns);
    nmse          g_{i+1} = c_i 2 e / D^k_i (+ c_i 2 ex / D^p_i on the x columns), D^k_i = sum Psi(x)^2,
                  D^p_i = sum x^2; the label is not detached, so the target encode's output gradient is
                  c_i (-2 e_f / D^k_i - 2 N^k_i / (D^k_i)^2 z_f), N^k_i = sum e^2;
    weighted_mse  g_{i+1} = c_i 2 w(column) e with w = 1 / (30 n) for columns < 3 and 9 / (10 n (d - 3)) for the others.
A CPU test checks it against torch.autograd over a literal BaseLoss (`torch_losses`, F.mse_loss) on this project's
Koopmanlinear / KoopmanBlinear in float64.  The nets: the constructor under torch.manual_seed(seed), and for DBKN
H.weight overwritten with 0.05 randn of a seeded generator (a zero H exercises neither H' lambda nor the forward term).

The tolerance rule, the only one of these tests: per test input the reference's own spread is measured -- per
parameter block (W_l, b_l, A, B, H), max |float64 - np.longdouble| and max |float64 - reversed summation order|
(every contraction, the sum over c and every loss sum) over the block, divided by the block's max -- and asserted
below SPREAD (1e-12: an ill-conditioned input cannot hide a failure).  The product is held to
min(100 max(spread, 2.2e-16), 1e-9) of the block's max: two decades above the spread, the spread taken no smaller
than float64's epsilon, below which it cannot be resolved, and never looser than the control step's bar.  The
losses that are not NaN: the same rule as an rtol; the parameters after Adam steps: the same rule on the parameters.
Conditions on the inputs, asserted by every reference with no sample excluded: a ReLU whose pre-activation is
within rounding of zero may take either branch, so min |hidden pre-activation| >= PRE_MIN (1e-9); and every nmse
normaliser >= DEN_MIN (1e-3) times its number of summands.
"""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import soarm_pkg  # noqa: F401

LAYERS = (8, 64, 64, 64, 64, 24)   # the reference's encoder (args.py:103): two last-layer tiles
LAYERS3 = (8, 64, 64, 40)          # three last-layer tiles, nl = 3
XD, UD, NPOS, GAMMA = 8, 5, 3, 0.8
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
SPREAD, BAR, F64EPS = 1e-12, 1e-9, 2.220446049250313e-16
PRE_MIN = 1e-9
DEN_MIN = 1e-3  # an nmse normaliser per summand
SENTINEL = -7777.25
T = 7
HSCALE = 0.05
STEPS = [(0, 1e-3), (2, 5e-4), (1, 2e-3), (2, 1e-3), (0, 7e-4)]  # (t0, lr) per step
KLOSS = {"mse": 0, "nmse": 1, "weighted_mse": 2}
DKUC, DBKN = "dkuc", "dbkn"


# ------------------------------------------------------------------------------------ the reference
def blocks(model, layers):
    """[(name, start, stop)] of the flat parameter vector [W_0 | b_0 | ... | A | B (| H for DBKN)]."""
    out, o = [], 0
    for l, (a, b) in enumerate(zip(layers[:-1], layers[1:])):
        out.append((f"W{l}", o, o + a * b)), out.append((f"b{l}", o + a * b, o + a * b + b))
        o += a * b + b
    nz = XD + layers[-1]
    out.append(("A", o, o + nz * nz)), out.append(("B", o + nz * nz, o + nz * nz + nz * UD))
    o += nz * nz + nz * UD
    return out + [("H", o, o + nz * nz * UD)] if model == DBKN else out


def unpack(p, layers):
    """(Ws, bs, A, B) of the linear part of p"""
    bl = {n: p[a:b] for n, a, b in blocks(DKUC, layers)}
    nl, nz = len(layers) - 1, XD + layers[-1]
    Ws = [bl[f"W{l}"].reshape(layers[l + 1], layers[l]) for l in range(nl)]
    return Ws, [bl[f"b{l}"] for l in range(nl)], bl["A"].reshape(nz, nz), bl["B"].reshape(nz, UD)


def h_blocks(H, u_z):
    """[H_c (nz x nz) for c < u_dim]: H_c[:, j] multiplies u_c z_j"""
    nz = H.shape[0]
    return [H[:, c * nz:(c + 1) * nz] if u_z else H[:, c::UD] for c in range(UD)]


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

    nlin = blocks(DKUC, layers)[-1][2]
    Ws, bs, A, B = [[w.astype(dt) for w in g] if isinstance(g, list) else g.astype(dt) for g in unpack(p, layers)]
    nl, n, nz = len(Ws), x.shape[1], A.shape[0]
    Hc = h_blocks(p[nlin:].astype(dt).reshape(nz, nz * UD), u_z) if model == DBKN else []
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

    def base(pred, lab, c):
        """BaseLoss(pred, lab) and c times its gradients (with respect to pred, with respect to lab)"""
        d = pred - lab
        if loss == "mse":
            g = c * 2 * d / (n * lab.shape[1])
            return mean(d ** 2), g, -g
        if loss == "nmse":
            N, D = tot(d * d), tot(lab * lab)
            denmin[0] = min(denmin[0], float(D) / lab.size)
            return N / D, c * (2 * d / D), c * (-2 * d / D - 2 * (N / (D * D)) * lab)
        w = np.empty(lab.shape[1], dt)
        with np.errstate(divide="ignore"):
            w[:3], w[3:] = dt(1) / (30 * n), dt(9) / (10 * dt(n) * (lab.shape[1] - 3))
        return (mean(d[:, :3] ** 2) + 9 * mean(d[:, 3:] ** 2)) / 10, c * (2 * w * d), c * (-2 * w * d)

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
        c_i = beta[i] / cont
        lk, gi, gz = base(zn, zt, c_i)
        lp, gp, _ = base(zn[:, :XD], x[i + 1], c_i)
        sk += beta[i] * lk
        sp += beta[i] * lp
        sd += beta[i] * base(zn[:, :npos], x[i + 1][:, :npos], c_i)[0]
        sa += beta[i] * base(zn[:, npos:XD], x[i + 1][:, npos:], c_i)[0]
        gi[:, :XD] += gp
        enc.append((acts, gz[:, XD:]))  # (the x columns of the label are data)
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


def ref_adam(p, m, v, g, t, lr):
    """torch.optim.Adam's update (no weight decay), step count t >= 1, in g's dtype."""
    dt = g.dtype.type
    m = dt(BETA1) * m + (1 - dt(BETA1)) * g
    v = dt(BETA2) * v + (1 - dt(BETA2)) * g * g
    bc1, bc2 = 1 - dt(BETA1) ** t, 1 - dt(BETA2) ** t
    return p - (dt(lr) / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + dt(EPS)), m, v


def block_spread(bl, a, others):
    """per block: max over `others` of max |a - o| / max |a|"""
    return {name: max(float(np.abs(a[s:e] - o[s:e].astype(np.float64)).max()) for o in others) / float(np.abs(a[s:e]).max())
            for name, s, e in bl}


def assert_blocks(bl, got, want, spread, what, scale_from=None):
    """got == want per block within min(100 * max(spread, eps), 1e-9) * max |scale_from or want|; prints
    each figure"""
    bad = []
    ref = want if scale_from is None else scale_from
    for name, s, e in bl:
        assert spread[name] < SPREAD, f"{what}: reference spread {spread[name]:.2e} in block {name}"
        scale = float(np.abs(ref[s:e]).max())
        bar = min(100 * max(spread[name], F64EPS), BAR)
        err = float(np.abs(got[s:e] - want[s:e]).max()) / scale
        print(f"{what} {name}: err {err:.2e} bar {bar:.2e} spread {spread[name]:.2e}")
        if not err <= bar:
            bad.append((name, err, bar))
    assert not bad, f"{what}: {bad}"


def nan_pattern(loss, npos):
    """which of the six losses are NaN: under weighted_mse a slice of three columns or fewer"""
    return [False] * 4 + [loss == "weighted_mse" and npos <= 3, loss == "weighted_mse" and XD - npos <= 3]


def loss_spread(l64, others, loss, npos):
    """max relative spread over the losses that are neither NaN nor recon; asserts the NaN pattern of each"""
    nan = nan_pattern(loss, npos)
    keep = [k for k in (0, 1, 2, 4, 5) if not nan[k]]
    for o in (l64,) + tuple(others):
        assert np.isnan(o.astype(np.float64)).tolist() == nan, (o, nan)
    return max(float(np.abs((l64[keep] - o[keep].astype(np.float64)) / l64[keep]).max()) for o in others)


def assert_losses(got, want, ls, loss, npos, what="losses"):
    nan = nan_pattern(loss, npos)
    keep = [k for k in (0, 1, 2, 4, 5) if not nan[k]]
    assert got[3] == 0.0
    assert np.isnan(got).tolist() == nan, (got, nan)
    lerr = float(np.abs((got[keep] - want[keep]) / want[keep]).max())
    lbar = min(100 * max(ls, F64EPS), BAR)
    print(f"{what}: err {lerr:.2e} bar {lbar:.2e} spread {ls:.2e}")
    assert lerr <= lbar


def fresh_net(model=DKUC, seed=1, layers=LAYERS, u_z=0, hscale=HSCALE):
    """a new float64 net: torch.manual_seed(seed), the constructor, then for DBKN the seeded hscale randn H"""
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman import KoopmanBlinear, Koopmanlinear
    torch.manual_seed(seed)
    if model == DKUC:
        return Koopmanlinear(XD, UD, list(layers)).double()
    net = KoopmanBlinear(XD, UD, list(layers), bool(u_z)).double()
    if hscale:
        g = torch.Generator().manual_seed(seed + 100)
        with torch.no_grad():
            net.H.weight.copy_(hscale * torch.randn(net.H.weight.shape, generator=g, dtype=torch.float64))
    return net


@functools.lru_cache(maxsize=None)
def make_net(model=DKUC, seed=1, layers=LAYERS, u_z=0, hscale=HSCALE):
    """fresh_net, made once per argument list and shared: not to be written to"""
    return fresh_net(model, seed, layers, u_z, hscale)


def make_rows(N, seed):
    """[T+1, N, 13] fp32 rows [u | x]: x from the control tests' state sampler, u ~ U(-0.5, 0.5)."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform([0.1, -0.2, 0.0], [0.45, 0.2, 0.35], (T + 1, N, 3)),
                        rng.uniform(-1.0, 1.0, (T + 1, N, 5))], -1)
    u = rng.uniform(-0.5, 0.5, (T + 1, N, UD))
    return np.concatenate([u, x], -1).astype(np.float32)


def make_idx(n, N, seed):
    """a permutation of 0..N-1 cut to n, with a repeat (entry 0 copied over entry 2)"""
    idx = np.random.default_rng(seed).permutation(N)[:n].astype(np.int32)
    if n > 2:
        idx[2] = idx[0]
    return idx


def window(rows, idx, t0, P):
    w = rows[t0:t0 + P + 1][:, idx]
    return w[:, :, UD:], w[:P, :, :UD]


def relayout(rows):
    """the rows in a second layout: ld = 16, [pad 2 | x 8 | pad 1 | u 5], padding filled with junk"""
    out = np.full(rows.shape[:2] + (16,), 9.75e3, np.float32)
    out[:, :, 2:10], out[:, :, 11:16] = rows[:, :, UD:], rows[:, :, :UD]
    return out, 16, 2, 11


def three_evaluations(p, model, layers, u_z, loss, npos, x, u, P):
    """ref_loss_grad in float64, and its spread against longdouble and reversed sums -> (losses, grad, grad
    spread per block, loss spread).  The conditions on the inputs and on the spread of the losses are asserted
    here; that on the spread of the blocks where they are compared (assert_blocks)."""
    l64, g64, premin, denmin = ref_loss_grad(p, model, layers, u_z, loss, npos, x, u, P)
    assert premin >= PRE_MIN, f"a hidden pre-activation of {premin:.2e} is within rounding of zero: change the seed"
    assert denmin >= DEN_MIN, f"an nmse normaliser of {denmin:.2e} per summand: change the seed"
    others = [ref_loss_grad(p, model, layers, u_z, loss, npos, x, u, P, np.longdouble),
              ref_loss_grad(p, model, layers, u_z, loss, npos, x, u, P, reverse=True)]
    bl = blocks(model, layers)
    gs = block_spread(bl, g64, [o[1] for o in others])
    ls = loss_spread(l64, [o[0] for o in others], loss, npos)
    assert ls < SPREAD, f"reference loss spread {ls:.2e}"
    print(f"reference {model} {loss} n {x.shape[1]} P {P}: premin {premin:.2e} denmin {denmin:.2e} loss spread {ls:.2e} "
          f"grad spread {max(gs.values()):.2e}"
          + (f" (H {gs['H']:.2e}) max |dH| {np.abs(g64[bl[-1][1]:]).max():.2e}" if model == DBKN else ""))
    return l64, g64, gs, ls


_REF = {}


def reference(model, layers, n, P, t0, use_idx, u_z=0, loss="mse", npos=NPOS, seed=1, hscale=HSCALE):
    """(rows, idx or None, params, losses f64, grad f64, grad spread per block, loss spread), computed once
    per case and shared, read-only."""
    key = (model, layers, n, P, t0, use_idx, u_z, loss, npos, seed, hscale)
    if key not in _REF:
        from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net
        N = n + 5 if use_idx else n
        rows = make_rows(N, seed + 10)
        idx = make_idx(n, N, seed + 20) if use_idx else None
        p = params_from_net(make_net(model, seed, layers, u_z, hscale))
        x, u = window(rows, idx if use_idx else np.arange(n), t0, P)
        l64, g64, gs, ls = three_evaluations(p, model, layers, u_z, loss, npos, x, u, P)
        for a in (rows, p, l64, g64):
            a.setflags(write=False)
        _REF[key] = (rows, idx, p, l64, g64, gs, ls)
    return _REF[key]


@functools.lru_cache(maxsize=None)
def adam_reference(model, layers, n, nsteps, u_z=0, loss="mse", seed=1):
    """(rows, idx, [(parameters after k reference steps in float64, their spread per block against the same
    steps in longdouble and with reversed sums) for k = 1 .. nsteps])"""
    rows, idx, p0, *_ = reference(model, layers, n, 5, 0, True, u_z, loss, NPOS, seed)
    runs = []
    for dt, rev in ((np.float64, False), (np.longdouble, False), (np.float64, True)):
        p, m, v, traj = p0.astype(dt), np.zeros_like(p0, dtype=dt), np.zeros_like(p0, dtype=dt), []
        for t, (t0, lr) in enumerate(STEPS[:nsteps], 1):
            x, u = window(rows, idx, t0, 5)
            _, g, premin, denmin = ref_loss_grad(p, model, layers, u_z, loss, NPOS, x, u, 5, dt, rev)
            assert premin >= PRE_MIN and denmin >= DEN_MIN
            p, m, v = ref_adam(p, m, v, g, t, lr)
            traj.append(p)
        runs.append(traj)
    bl = blocks(model, layers)
    return rows, idx, [(runs[0][k], block_spread(bl, runs[0][k], [runs[1][k], runs[2][k]])) for k in range(nsteps)]


def torch_losses(net, x, u, P, loss, npos):
    """k_linear_loss's six values with a literal BaseLoss, on this project's net (float64 torch)"""
    import torch
    import torch.nn.functional as F

    def base(preds, labels):
        if loss == "mse":
            return F.mse_loss(preds, labels)
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


# ---------------------------------------------------------------------------------- the C ABI's side
def desc_opts(layers=LAYERS, P=5):
    from lerobot_mujoco_sim2real_amd import abi
    d = abi.KoopmanDesc()
    d.x_dim, d.u_dim, d.nlayer, d.horizon, d.u_clip = XD, UD, len(layers) - 1, 10, 0.5
    for i, w in enumerate(layers):
        d.width[i] = w
    o = abi.KoopmanTrainOpts()
    o.pre_length, o.npos, o.gamma, o.beta1, o.beta2, o.eps = P, NPOS, GAMMA, BETA1, BETA2, EPS
    return d, o


def trainer(model=DKUC, layers=LAYERS, max_batch=130, P=5, u_z=0, loss="mse", npos=NPOS, seed=1, hscale=HSCALE, net=None):
    from lerobot_mujoco_sim2real_amd.control.koopman_train import BilinearKoopmanTrainer, KoopmanTrainer
    net = make_net(model, seed, layers, u_z, hscale) if net is None else net
    return (BilinearKoopmanTrainer if model == DBKN else KoopmanTrainer)(
        net, max_batch, pre_length=P, npos=npos, gamma=GAMMA, betas=(BETA1, BETA2), eps=EPS, loss_name=loss)


def abi_loss_grad(tr, rows, idx, t0, layout=(13, UD, 0), pad=0):
    """sim_koopman_loss_grad through ctypes -> (losses [6], grad [nparam + pad]) numpy; grad is
    filled with SENTINEL first"""
    import torch
    dev = tr.device
    r = torch.as_tensor(np.array(rows), device=dev)
    ix = None if idx is None else torch.as_tensor(idx, device=dev)
    n = rows.shape[1] if idx is None else len(idx)
    losses = torch.full((6,), SENTINEL, dtype=torch.float64, device=dev)
    grad = torch.full((tr.nparam + pad,), SENTINEL, dtype=torch.float64, device=dev)
    ld, xo, uo = layout
    rc = tr.lib.sim_koopman_loss_grad(tr._h, n, rows.shape[1], rows.shape[0] - 1, C.c_void_p(r.data_ptr()), ld, xo, uo,
                                      None if ix is None else C.c_void_p(ix.data_ptr()), t0,
                                      C.c_void_p(losses.data_ptr()), C.c_void_p(grad.data_ptr()), tr._stream())
    assert rc == 0, tr.lib.sim_last_error().decode()
    torch.cuda.synchronize()
    return losses.cpu().numpy(), grad.cpu().numpy()


# ------------------------------------------------------- test bodies that more than one file runs
def check_reference_gradient_equals_autograd(model, u_z, layers, n, P, loss, npos=NPOS):
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net
    rows, _, p, l64, g64, _, _ = reference(model, layers, n, P, 1, False, u_z, loss, npos)
    net = make_net(model, 1, layers, u_z)
    x, u = window(rows, np.arange(n), 1, P)
    net.zero_grad()
    six = torch_losses(net, torch.as_tensor(x.astype(np.float64)), torch.as_tensor(u.astype(np.float64)), P, loss, npos)
    six[0].backward()
    gnet = fresh_net(model, 1, layers, u_z)  # a second net to carry the gradients as parameters
    with torch.no_grad():
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


def check_loss_grad_matches_reference(model, layers, n, P, last, u_z, use_idx, alt, loss="mse", npos=NPOS):
    """n: one lane, a full wave, one past it (nmse: the normaliser crosses waves), one past a workgroup (it
    crosses workgroups), several workgroups; the window at row 0 and ending on row T; u_z, traj_idx NULL / a
    permutation with a repeat into a larger N, and the in-place / ld = 16 layout alternate over the cases."""
    t0 = T - P if last else 0
    rows, idx, p, l64, g64, gs, ls = reference(model, layers, n, P, t0, bool(use_idx), u_z, loss, npos)
    tr = trainer(model, layers, 130, P, u_z, loss, npos)
    assert tr.loss_name == loss and tr.nparam == p.size and np.array_equal(tr.get_params(), p)
    r, *layout = relayout(rows) if alt else (rows, 13, UD, 0)
    losses, grad = abi_loss_grad(tr, r, idx, t0, tuple(layout))
    assert_losses(losses, l64, ls, loss, npos)
    assert_blocks(blocks(model, layers), grad, g64, gs, "grad")
    assert np.array_equal(tr.get_params(), p)  # loss_grad changes no state


def check_reproducible_and_keeps_to_its_buffer(model, u_z, loss="mse"):
    """two loss_grad calls agree byte for byte and leave the tail of a longer buffer alone -> (trainer, rows, idx, p0)"""
    rows, idx, p0, *_ = reference(model, LAYERS, 130, 5, 2, True, u_z, loss)
    tr = trainer(model, LAYERS, 130, 5, u_z, loss)
    l1, g1 = abi_loss_grad(tr, rows, idx, 2, pad=64)
    l2, g2 = abi_loss_grad(tr, rows, idx, 2, pad=64)
    assert l1.tobytes() == l2.tobytes() and g1.tobytes() == g2.tobytes()
    assert np.all(g1[tr.nparam:] == SENTINEL) and not np.any(g1[:tr.nparam] == SENTINEL)
    assert tr.nparam == blocks(model, LAYERS)[-1][2]
    return tr, rows, idx, p0


def check_null_outputs(tr, rows, n, idx):
    """grad and losses may be NULL -> the rows (and idx) on the device"""
    import torch
    r = torch.as_tensor(np.array(rows), device=tr.device)
    ix = None if idx is None else torch.as_tensor(idx, device=tr.device)
    assert tr.lib.sim_koopman_loss_grad(tr._h, n, rows.shape[1], T, C.c_void_p(r.data_ptr()), 13, UD, 0,
                                        None if ix is None else C.c_void_p(ix.data_ptr()), 0, None, None, tr._stream()) == 0
    torch.cuda.synchronize()
    return r, ix


def check_queued_equal_synchronised(a, b, r, ix, p0):
    """STEPS on a queued back to back, on b each followed by a synchronisation: the same bytes"""
    import torch
    la, lb = [], []
    for t0, lr in STEPS:
        la.append(a.step(r, ix, t0, lr))
    for t0, lr in STEPS:
        lb.append(b.step(r, ix, t0, lr))
        torch.cuda.synchronize()
    pa, pb = a.get_params(), b.get_params()
    assert pa.tobytes() == pb.tobytes() and not np.array_equal(pa, p0)
    assert torch.stack(la).cpu().numpy().tobytes() == torch.stack(lb).cpu().numpy().tobytes()


def check_queued_steps_and_reset(model):
    """-> (a, b, fresh, r, ix, p0): a reset and stepped once as fresh was, b after STEPS"""
    import torch
    rows, idx, p0, *_ = reference(model, LAYERS, 65, 5, 0, True, 0)
    a, b, fresh = (trainer(model, LAYERS, 65, 5) for _ in range(3))
    r, ix = torch.as_tensor(np.array(rows), device=a.device), torch.as_tensor(idx, device=a.device)
    check_queued_equal_synchronised(a, b, r, ix, p0)
    # set_params(..., reset_optimizer=1) then a step == the first step of a fresh trainer
    fresh.step(r, ix, 2, 1e-3)
    a.set_params(p0, reset_optimizer=True)
    assert np.array_equal(a.get_params(), p0)
    a.step(r, ix, 2, 1e-3)
    assert a.get_params().tobytes() == fresh.get_params().tobytes()
    return a, b, fresh, r, ix, p0


def check_train_steps_match_reference_adam(model, layers, u_z, loss="mse"):
    import torch
    n = 65
    rows, idx, want = adam_reference(model, layers, n, 5, u_z, loss)
    tr = trainer(model, layers, n, 5, u_z, loss)
    r = torch.as_tensor(np.array(rows), device=tr.device)
    ix = torch.as_tensor(idx, device=tr.device)
    bl = blocks(model, layers)
    for k, (t0, lr) in enumerate(STEPS):
        tr.step(r, ix, t0, lr)
        if k in (0, 4):
            assert_blocks(bl, tr.get_params(), want[k][0], want[k][1], f"params after {k + 1} steps")
    # the fragment copies (both of H's among them) follow the master vector: the next gradient is that of the
    # updated parameters
    p5 = tr.get_params()
    if model == DBKN:
        assert np.abs(p5[bl[-1][1]:] - make_net(model, 1, layers, u_z).H.weight.detach().numpy().ravel()).max() > 0
    x, u = window(rows, idx, 1, 5)
    l64, g64, gs, ls = three_evaluations(p5, model, layers, u_z, loss, NPOS, x, u, 5)
    losses, grad = tr.loss_grad(r, ix, 1)
    assert_blocks(bl, grad.cpu().numpy(), g64, gs, "grad after 5 steps")
    assert_losses(losses.cpu().numpy(), l64, ls, loss, NPOS, "losses after 5 steps")


def check_train_end_to_end(net, loss="mse"):
    """train() on a fresh net, then the controller's evaluate of it -> (hist, controller, evaluation, rows)"""
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net, train
    from lerobot_mujoco_sim2real_amd.control.MPC_Controler import MPCController
    p0 = params_from_net(net)
    rows = torch.as_tensor(make_rows(40, 5), device=torch.device("cuda", 0))
    hist = train(net, rows, epochs=2, batch_size=32, lr=1e-3, seed=3, eval_interval=1, loss_name=loss)
    tl = np.array(hist["train_loss"])
    assert tl.shape == (2, 6) and np.isnan(tl).tolist() == [nan_pattern(loss, NPOS)] * 2 and np.all(tl[:, 3] == 0)
    assert len(hist["eval"]) == 2 and hist["best_epoch"] in (0, 1) and np.isfinite(hist["best_error"])
    assert np.array_equal(params_from_net(net), hist["best_params"]) and not np.array_equal(hist["best_params"], p0)
    assert np.all(np.isfinite(hist["best_params"])) and hist["best_params"].size == p0.size

    class args:  # noqa: N801
        x_dim, u_dim, MPC_type = XD, UD, "delta_mpc"
    ctl = MPCController(net, args)
    e = ctl.evaluate(rows)
    assert np.isfinite(e["avg_error"]) and e["avg_error"] == pytest.approx(hist["best_error"], rel=1e-12)
    return hist, ctl, e, rows


def check_argument_errors(model):
    import torch
    from lerobot_mujoco_sim2real_amd import abi
    u_z = int(model == DBKN)
    tr = trainer(model, LAYERS, 16, 5, u_z)
    lib = tr.lib
    rows = torch.as_tensor(make_rows(20, 1), device=tr.device)
    rp, st = C.c_void_p(rows.data_ptr()), tr._stream()
    losses = torch.zeros(6, dtype=torch.float64, device=tr.device)
    lp = C.c_void_p(losses.data_ptr())

    def both(n, N, Tt, r, ld, xo, uo, t0, h=tr._h):
        return (lib.sim_koopman_loss_grad(h, n, N, Tt, r, ld, xo, uo, None, t0, lp, None, st),
                lib.sim_koopman_train_step(h, n, N, Tt, r, ld, xo, uo, None, t0, 1e-3, lp, st))

    p0 = tr.get_params()
    E = (abi.E_ARG, abi.E_ARG)
    assert both(4, 20, T, rp, 13, UD, 0, 0, h=None) == E      # NULL tr
    assert both(4, 20, T, None, 13, UD, 0, 0) == E            # NULL rows
    assert both(17, 20, T, rp, 13, UD, 0, 0) == E             # n > max_batch
    assert both(-1, 20, T, rp, 13, UD, 0, 0) == E             # n < 0
    assert both(4, 20, T, rp, 13, UD, 0, -1) == E             # t0 < 0
    assert both(4, 20, T, rp, 13, UD, 0, T - 5 + 1) == E      # t0 + pre_length > T
    assert both(4, 20, T, rp, 13, 6, 0, 0) == E               # x columns past ld
    assert both(4, 20, T, rp, 13, UD, 9, 0) == E              # u columns past ld
    assert both(4, 3, T, rp, 13, UD, 0, 0) == E               # n > N without traj_idx
    assert b"ld" in lib.sim_last_error() or b"N" in lib.sim_last_error()
    assert both(0, 20, T, rp, 13, UD, 0, 0) == (0, 0)         # n == 0: a no-op
    assert np.array_equal(tr.get_params(), p0)                # none of the above touched the parameters
    assert both(4, 20, T, rp, 13, UD, 0, T - 5) == (0, 0)     # the last valid window
    torch.cuda.synchronize()
    # a bad struct header, a model past the kernel's plan
    d, o = desc_opts()
    h = C.c_void_p()
    pp = p0.ctypes.data_as(C.c_void_p)

    def create(u_z=1):
        if model == DBKN:
            return lib.sim_koopman_trainer_create_bilinear(C.byref(d), pp, u_z, 16, C.byref(o), 0, C.byref(h))
        return lib.sim_koopman_trainer_create(C.byref(d), pp, 16, C.byref(o), 0, C.byref(h))

    o.struct_size -= 8
    assert create() == abi.E_ARG and not h
    o.struct_size += 8
    o.abi_version += 1
    assert create() == abi.E_ARG and not h
    o.abi_version -= 1
    o.pre_length = 0
    assert create() == abi.E_ARG and not h
    o.pre_length = 5
    if model == DBKN:
        assert create(2) == abi.E_ARG and not h
    d.nlayer, d.width[6] = 6, 24
    d.width[5] = 64
    assert create() == abi.E_MODEL and not h
    assert b"nlayer" in lib.sim_last_error()
