"""The bilinear (DBKN) Koopman training step (include/koopman_mpc.h sim_koopman_trainer_create_bilinear,
sim_koopman_trainer_nparam_bilinear; control/koopman_train.py BilinearKoopmanTrainer) against a numpy
restatement of the reference.

The reference trains DBKN with the train() and k_linear_loss of DKUC (test_koopman_train.py's docstring);
only koopman_operation differs (models/KoopmanBase.py:62-78): z^_{i+1} = A z^_i + B u_i + H vec(z^_i (x) u_i)
(u_z: vec(u_i (x) z^_i)).  With H_c (nz x nz) the block of H that multiplies u_c z -- columns c nz + j
for u_z = 1, columns j u_dim + c for u_z = 0 --
    forward   z^_{i+1} = A z^_i + B u_i + sum_c H_c (u_{i,c} z^_i)
    reverse   dH_c += lambda_{i+1} (u_{i,c} z^_i)'   (beside dA, dB)
              lambda_i = g_i + A' lambda_{i+1} + sum_c u_{i,c} (H_c' lambda_{i+1}).
`ref_loss_grad` below is that forward and its hand-written backward in numpy from the flat parameter
vector [W_0 | b_0 | ... | A | B | H]; no product code computes it.  A CPU test checks it against
torch.autograd on this project's KoopmanBlinear for both u_z.  The nets: KoopmanBlinear under
torch.manual_seed(seed), H.weight overwritten with 0.05 randn of a seeded generator (a zero H exercises
neither H' lambda nor the forward term).

Tolerances are test_koopman_train.py's rule with one more block, H: per test input the reference's own
spread per block (max |float64 - longdouble| and max |float64 - reversed summation|, over the block's
max |g|) is asserted below 1e-12, and the product is held to min(100 max(spread, 2.2e-16), 1e-9) of the
block's max; losses and post-Adam parameters likewise.  Every reference asserts min |hidden
pre-activation| >= 1e-9, no sample excluded.

Measured on the CPU over the GPU tests' inputs (both encoders, both u_z, n = 1 .. 130, P = 1 and 5):
gradient spreads <= 1.03e-15 per block (H: <= 9.2e-16), so the bars are 2.2e-14 .. 1.03e-13; loss spreads
<= 4.0e-16 (bar <= 4.0e-14); parameter spreads after 1 and after 5 Adam steps <= 1.6e-14 per block (H: 5.1e-16;
bars <= 1.6e-12); the least pre-activation 3.9e-7; max |dH| >= 3.8e-3 in every case (not a near-zero block).
Measured on an MI355X against those bars:
gradient error <= 1.6e-15 (H: 1.5e-15), loss error <= 6.1e-16, parameter error <= 1.1e-14 (H: 5.1e-16) -- at
most 5% of its bar in every block.  With H = 0 the losses and the W, b, A, B blocks equal the DKUC trainer's
bit for bit (the test asks only for the bar).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import soarm_pkg  # noqa: F401
import test_koopman_train as tk

LAYERS, LAYERS3 = tk.LAYERS, tk.LAYERS3
XD, UD, NPOS, GAMMA = tk.XD, tk.UD, tk.NPOS, tk.GAMMA
BETA1, BETA2, EPS = tk.BETA1, tk.BETA2, tk.EPS
SPREAD, BAR, F64EPS, PRE_MIN, SENTINEL, T = tk.SPREAD, tk.BAR, tk.F64EPS, tk.PRE_MIN, tk.SENTINEL, tk.T
HSCALE = 0.05
NZL = [0, 1, 2, 4, 5]  # the losses that are not identically zero


# ------------------------------------------------------------------------------------ the reference
def blocks(layers):
    """[(name, start, stop)] of the flat parameter vector [W_0 | b_0 | ... | A | B | H]."""
    out = tk.blocks(layers)
    nz, o = XD + layers[-1], out[-1][2]
    return out + [("H", o, o + nz * nz * UD)]


def h_blocks(H, u_z):
    """[H_c (nz x nz) for c < u_dim]: H_c[:, j] multiplies u_c z_j"""
    nz = H.shape[0]
    return [H[:, c * nz:(c + 1) * nz] if u_z else H[:, c::UD] for c in range(UD)]


def ref_loss_grad(p, layers, u_z, x, u, P, dt=np.float64, reverse=False):
    """x [P+1, n, x_dim], u [P, n, u_dim] (float32 data, widened) -> (losses [6], grad [nparam],
    min |hidden pre-activation|) in dtype dt.  reverse: every contraction, and the sum over c, in
    the opposite order."""
    fl = (lambda a, ax: np.ascontiguousarray(np.flip(a, ax))) if reverse else (lambda a, ax: a)

    def mm(a, b):  # a [m, k] @ b [k, q]
        return fl(a, 1) @ fl(b, 0)

    nlin = tk.blocks(layers)[-1][2]
    Ws, bs, A, B = [[w.astype(dt) for w in g] if isinstance(g, list) else g.astype(dt) for g in tk.unpack(p[:nlin], layers)]
    nl, n, nz = len(Ws), x.shape[1], A.shape[0]
    Hc = h_blocks(p[nlin:].astype(dt).reshape(nz, nz * UD), u_z)
    cs = list(range(UD))[::-1] if reverse else list(range(UD))
    x, u = x.astype(dt), u.astype(dt)
    premin = [np.inf]

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
        e, ex = zn - zt, zn[:, :XD] - x[i + 1]
        sk += beta[i] * (e ** 2).mean()
        sp += beta[i] * (ex ** 2).mean()
        sd += beta[i] * (ex[:, :NPOS] ** 2).mean()
        sa += beta[i] * (ex[:, NPOS:] ** 2).mean()
        gi = (beta[i] / cont) * 2 * e / (n * nz)
        enc.append((acts, -gi[:, XD:]))
        gi = gi.copy()
        gi[:, :XD] += (beta[i] / cont) * 2 * ex / (n * XD)
        zh.append(zn), g.append(gi)
    koop, pred = sk / cont, sp / cont
    losses = np.array([koop + pred, koop, pred, dt(0), sd / cont, sa / cont], dt)
    dW, db = [np.zeros_like(w) for w in Ws], [np.zeros_like(b) for b in bs]
    dA, dB, dHc = np.zeros_like(A), np.zeros_like(B), [np.zeros_like(A) for _ in range(UD)]
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
    dH = np.zeros((nz, nz * UD), dt)
    for c in range(UD):
        if u_z:
            dH[:, c * nz:(c + 1) * nz] = dHc[c]
        else:
            dH[:, c::UD] = dHc[c]
    grad = np.concatenate([np.concatenate([w.ravel(), b]) for w, b in zip(dW, db)] + [dA.ravel(), dB.ravel(), dH.ravel()])
    return losses, grad, premin[0]


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


def assert_losses(got, want, ls, what="losses"):
    assert got[3] == 0.0
    lerr = float(np.abs((got[NZL] - want[NZL]) / want[NZL]).max())
    lbar = min(100 * max(ls, F64EPS), BAR)
    print(f"{what}: err {lerr:.2e} bar {lbar:.2e} spread {ls:.2e}")
    assert lerr <= lbar


@functools.lru_cache(maxsize=None)
def make_net(seed=1, layers=LAYERS, u_z=0, hscale=HSCALE):
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman import KoopmanBlinear
    torch.manual_seed(seed)
    net = KoopmanBlinear(XD, UD, list(layers), bool(u_z)).double()
    if hscale:
        g = torch.Generator().manual_seed(seed + 100)
        with torch.no_grad():
            net.H.weight.copy_(hscale * torch.randn(net.H.weight.shape, generator=g, dtype=torch.float64))
    return net


_REF = {}


def reference(layers, n, P, t0, use_idx, u_z, seed=1, hscale=HSCALE):
    """(rows, idx or None, params, losses f64, grad f64, grad spread per block, loss spread), computed
    once per case and shared.  The ReLU condition is asserted here."""
    key = (layers, n, P, t0, use_idx, u_z, seed, hscale)
    if key not in _REF:
        from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net
        N = n + 5 if use_idx else n
        rows = tk.make_rows(N, seed + 10)
        idx = tk.make_idx(n, N, seed + 20) if use_idx else None
        p = params_from_net(make_net(seed, layers, u_z, hscale))
        x, u = tk.window(rows, idx if use_idx else np.arange(n), t0, P)
        l64, g64, premin = ref_loss_grad(p, layers, u_z, x, u, P)
        assert premin >= PRE_MIN, f"a hidden pre-activation of {premin:.2e} is within rounding of zero: change the seed"
        lld, gld, _ = ref_loss_grad(p, layers, u_z, x, u, P, np.longdouble)
        lrv, grv, _ = ref_loss_grad(p, layers, u_z, x, u, P, reverse=True)
        gs = block_spread(blocks(layers), g64, [gld, grv])
        ls = max(float(np.abs((l64[NZL] - o[NZL].astype(np.float64)) / l64[NZL]).max()) for o in (lld, lrv))
        assert ls < SPREAD, f"reference loss spread {ls:.2e}"
        print(f"reference {key}: premin {premin:.2e} loss spread {ls:.2e} grad spread {max(gs.values()):.2e} "
              f"(H {gs['H']:.2e}) max |dH| {np.abs(g64[blocks(layers)[-1][1]:]).max():.2e}")
        for a in (rows, p, l64, g64):
            a.setflags(write=False)
        _REF[key] = (rows, idx, p, l64, g64, gs, ls)
    return _REF[key]


# ------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("u_z", [0, 1])
@pytest.mark.parametrize("layers,n,P", [(LAYERS, 17, 5), (LAYERS3, 5, 1), (LAYERS, 1, 5)])
def test_reference_gradient_equals_autograd(layers, n, P, u_z):
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net
    rows, _, p, l64, g64, _, _ = reference(layers, n, P, 1, False, u_z)
    net = make_net(1, layers, u_z)
    x, u = tk.window(rows, np.arange(n), 1, P)
    net.zero_grad()
    loss = tk.torch_loss(net, torch.as_tensor(x.astype(np.float64)), torch.as_tensor(u.astype(np.float64)), P)
    loss.backward()
    gnet = make_net.__wrapped__(1, layers, u_z)  # a second net to carry the gradients as parameters
    with torch.no_grad():
        for a, b in zip(gnet.parameters(), net.parameters()):
            a.copy_(b.grad if b.grad is not None else torch.zeros_like(b))
    want = params_from_net(gnet)
    net.zero_grad()
    assert abs(float(loss.detach()) - l64[0]) <= 1e-13 * abs(l64[0])
    assert want.size == g64.size
    for name, s, e in blocks(layers):
        scale = np.abs(want[s:e]).max()
        assert scale > 0 and np.abs(g64[s:e] - want[s:e]).max() <= 1e-12 * scale, name


@pytest.mark.parametrize("u_z", [0, 1])
def test_params_round_trip(u_z):
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net, params_to_net
    net = make_net(3, LAYERS3, u_z)
    p = params_from_net(net)
    bl = blocks(LAYERS3)
    nz = XD + LAYERS3[-1]
    assert p.dtype == np.float64 and p.size == bl[-1][2] == tk.blocks(LAYERS3)[-1][2] + nz * nz * UD
    assert np.array_equal(p[bl[-1][1]:].reshape(nz, nz * UD), net.H.weight.detach().numpy())
    assert np.abs(p[bl[-1][1]:]).max() > 0
    _, _, A, B = tk.unpack(p[:bl[-2][2]], LAYERS3)
    assert np.array_equal(A, net.lA.weight.detach().numpy()) and np.array_equal(B, net.lB.weight.detach().numpy())
    other = make_net.__wrapped__(4, LAYERS3, u_z)
    assert not np.array_equal(params_from_net(other)[bl[-1][1]:], p[bl[-1][1]:])
    params_to_net(p, other)
    assert np.array_equal(params_from_net(other), p)
    assert torch.equal(other.H.weight, net.H.weight) and torch.equal(other.lC.weight, net.lC.weight)
    with pytest.raises(ValueError):
        params_to_net(p[:-1], other)
    with pytest.raises(ValueError):  # a DKUC vector is too short for a DBKN net
        params_to_net(p[:bl[-2][2]], other)
    # a Koopmanlinear's vector is what it was: no H block
    lin = tk.make_net(3, LAYERS3)
    pl = params_from_net(lin)
    assert pl.size == tk.blocks(LAYERS3)[-1][2]
    with pytest.raises(ValueError):
        params_to_net(p, tk.make_net.__wrapped__(4, LAYERS3))


def _desc_opts(layers=LAYERS, P=5):
    from lerobot_mujoco_sim2real_amd import abi
    d = abi.KoopmanDesc()
    d.x_dim, d.u_dim, d.nlayer, d.horizon, d.u_clip = XD, UD, len(layers) - 1, 10, 0.5
    for i, w in enumerate(layers):
        d.width[i] = w
    o = abi.KoopmanTrainOpts()
    o.pre_length, o.npos, o.gamma, o.beta1, o.beta2, o.eps = P, NPOS, GAMMA, BETA1, BETA2, EPS
    return d, o


def test_bilinear_entry_points_are_exported():
    from lerobot_mujoco_sim2real_amd import abi, build
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net
    for name in ("sim_koopman_trainer_nparam_bilinear", "sim_koopman_trainer_create_bilinear"):
        assert name in abi.EXPORTS
    build.build()
    lib = abi.load_lib()
    assert len(lib.sim_koopman_trainer_create_bilinear.argtypes) == 7
    d, o = _desc_opts()
    assert C.sizeof(abi.KoopmanTrainOpts) == 48 and abi.ABI_VERSION == 2
    nlin = lib.sim_koopman_trainer_nparam(C.byref(d))
    assert nlin == tk.blocks(LAYERS)[-1][2]
    assert lib.sim_koopman_trainer_nparam_bilinear(C.byref(d)) == nlin + 32 * 32 * 5 == blocks(LAYERS)[-1][2]
    assert lib.sim_koopman_trainer_nparam_bilinear(None) == abi.E_ARG
    p, h = params_from_net(make_net()), C.c_void_p()
    pp = p.ctypes.data_as(C.c_void_p)
    for bad in (2, -1):  # u_z is 0 or 1
        assert lib.sim_koopman_trainer_create_bilinear(C.byref(d), pp, bad, 16, C.byref(o), 0, C.byref(h)) == abi.E_ARG
        assert not h and b"u_z" in lib.sim_last_error()
    import torch
    if not torch.cuda.is_available():  # no GPU: creation fails loudly, as sim_koopman_trainer_create does
        for u_z in (0, 1):
            assert lib.sim_koopman_trainer_create_bilinear(C.byref(d), pp, u_z, 16, C.byref(o), 0, C.byref(h)) == -4
            assert not h


def test_bilinear_trainer_refuses_other_nets_and_losses():
    from lerobot_mujoco_sim2real_amd.control.koopman_train import BilinearKoopmanTrainer, KoopmanTrainer
    assert issubclass(BilinearKoopmanTrainer, KoopmanTrainer)
    with pytest.raises(NotImplementedError, match="KoopmanBlinear"):
        BilinearKoopmanTrainer(tk.make_net(), 16)
    with pytest.raises(NotImplementedError, match="mse"):
        BilinearKoopmanTrainer(make_net(), 16, loss_name="mae")
    with pytest.raises(NotImplementedError, match="DBKN"):  # and the DKUC trainer still refuses a net with H
        KoopmanTrainer(make_net(), 16)


# ------------------------------------------------------------------------------------------- GPU
def _trainer(layers=LAYERS, max_batch=130, P=5, u_z=0, seed=1, hscale=HSCALE):
    from lerobot_mujoco_sim2real_amd.control.koopman_train import BilinearKoopmanTrainer
    return BilinearKoopmanTrainer(make_net(seed, layers, u_z, hscale), max_batch, pre_length=P, npos=NPOS, gamma=GAMMA,
                                  betas=(BETA1, BETA2), eps=EPS)


def _cases():
    """(layers, n, P, last, u_z, use_idx, alt): every (encoder, n, P) once, the four alternatives as parities
    of the three indices chosen so that each value of each meets every n, both P and both encoders;
    then four more with the window position and u_z flipped."""
    ns, out = (1, 16, 17, 65, 130), []
    for ei, layers in enumerate((LAYERS, LAYERS3)):
        for k, n in enumerate(ns):
            for pi, P in enumerate((1, 5)):
                out.append((layers, n, P, (pi + ei + (k >> 1)) % 2, (k + pi + ei) % 2, (k + pi) % 2, (k + ei) % 2))
    for layers, n, P in ((LAYERS, 130, 5), (LAYERS3, 130, 1), (LAYERS, 17, 1), (LAYERS3, 65, 5)):
        c = next(c for c in out if c[:3] == (layers, n, P))
        out.append((layers, n, P, 1 - c[3], 1 - c[4], c[5], c[6]))
    for j, name in ((3, "last"), (4, "u_z"), (5, "use_idx"), (6, "alt")):  # the coverage the docstring promises
        for v in (0, 1):
            got = [c for c in out if c[j] == v]
            assert {c[1] for c in got} == set(ns) and {c[2] for c in got} == {1, 5} and {c[0] for c in got} == {LAYERS, LAYERS3}, name
    return out


CASES = _cases()


@pytest.mark.gpu
@pytest.mark.parametrize("layers,n,P,last,u_z,use_idx,alt", CASES,
                         ids=[f"{'ref' if c[0] is LAYERS else 'nl3'}-n{c[1]}-P{c[2]}-{'tail' if c[3] else 't0'}-uz{c[4]}-"
                              f"{'idx' if c[5] else 'all'}-{'ld16' if c[6] else 'ld13'}" for c in CASES])
def test_loss_grad_matches_reference(layers, n, P, last, u_z, use_idx, alt):
    """n: one lane, a full wave, one past it, one past a workgroup, several workgroups; the window at
    row 0 and ending on row T; u_z, traj_idx NULL / a permutation with a repeat into a larger N, and the
    in-place / ld = 16 layout alternate over the cases (see _cases)."""
    t0 = T - P if last else 0
    rows, idx, p, l64, g64, gs, ls = reference(layers, n, P, t0, bool(use_idx), u_z)
    tr = _trainer(layers, 130, P, u_z)
    assert tr.nparam == p.size and np.array_equal(tr.get_params(), p)
    r, *layout = tk.relayout(rows) if alt else (rows, 13, UD, 0)
    losses, grad = tk._loss_grad(tr, r, idx, t0, tuple(layout))
    assert_losses(losses, l64, ls)
    assert_blocks(blocks(layers), grad, g64, gs, "grad")
    assert np.array_equal(tr.get_params(), p)  # loss_grad changes no state


@pytest.mark.gpu
def test_loss_grad_is_reproducible_and_keeps_to_its_buffer():
    rows, idx, p, *_ = reference(LAYERS, 130, 5, 2, True, 1)
    tr = _trainer(u_z=1)
    l1, g1 = tk._loss_grad(tr, rows, idx, 2, pad=64)
    l2, g2 = tk._loss_grad(tr, rows, idx, 2, pad=64)
    assert l1.tobytes() == l2.tobytes() and g1.tobytes() == g2.tobytes()
    assert np.all(g1[tr.nparam:] == SENTINEL) and not np.any(g1[:tr.nparam] == SENTINEL)
    assert tr.nparam == blocks(LAYERS)[-1][2]


STEPS = tk.STEPS


@functools.lru_cache(maxsize=None)
def adam_reference(layers, n, nsteps, u_z, seed=1):
    """parameters after 1 .. nsteps reference steps in float64, and their spread per block against
    the same steps in longdouble and with reversed sums"""
    rows, idx, p0, *_ = reference(layers, n, 5, 0, True, u_z, seed)
    runs = []
    for dt, rev in ((np.float64, False), (np.longdouble, False), (np.float64, True)):
        p, m, v, traj = p0.astype(dt), np.zeros_like(p0, dtype=dt), np.zeros_like(p0, dtype=dt), []
        for t, (t0, lr) in enumerate(STEPS[:nsteps], 1):
            x, u = tk.window(rows, idx, t0, 5)
            _, g, premin = ref_loss_grad(p, layers, u_z, x, u, 5, dt, rev)
            assert premin >= PRE_MIN
            p, m, v = tk.ref_adam(p, m, v, g, t, lr)
            traj.append(p)
        runs.append(traj)
    bl = blocks(layers)
    return rows, idx, [(runs[0][k], block_spread(bl, runs[0][k], [runs[1][k], runs[2][k]])) for k in range(nsteps)]


@pytest.mark.gpu
@pytest.mark.parametrize("u_z", [0, 1])
def test_train_steps_match_reference_adam(u_z):
    import torch
    n, layers = 65, LAYERS
    rows, idx, want = adam_reference(layers, n, 5, u_z)
    tr = _trainer(layers, n, 5, u_z)
    r = torch.as_tensor(np.array(rows), device=tr.device)
    ix = torch.as_tensor(idx, device=tr.device)
    bl = blocks(layers)
    for k, (t0, lr) in enumerate(STEPS):
        tr.step(r, ix, t0, lr)
        if k in (0, 4):
            assert_blocks(bl, tr.get_params(), want[k][0], want[k][1], f"params after {k + 1} steps")
    # both fragment copies of H (and the others') follow the master vector: the next gradient is that of
    # the updated parameters
    p5 = tr.get_params()
    assert np.abs(p5[bl[-1][1]:] - make_net(1, layers, u_z).H.weight.detach().numpy().ravel()).max() > 0
    x, u = tk.window(rows, idx, 1, 5)
    l64, g64, premin = ref_loss_grad(p5, layers, u_z, x, u, 5)
    assert premin >= PRE_MIN
    losses, grad = tr.loss_grad(r, ix, 1)
    sp = block_spread(bl, g64, [ref_loss_grad(p5, layers, u_z, x, u, 5, np.longdouble)[1],
                                ref_loss_grad(p5, layers, u_z, x, u, 5, reverse=True)[1]])
    assert_blocks(bl, grad.cpu().numpy(), g64, sp, "grad after 5 steps")


@pytest.mark.gpu
def test_queued_steps_equal_synchronised_steps_and_reset():
    import torch
    rows, idx, p0, *_ = reference(LAYERS, 65, 5, 0, True, 0)
    a, b = _trainer(LAYERS, 65, 5), _trainer(LAYERS, 65, 5)
    r = torch.as_tensor(np.array(rows), device=a.device)
    ix = torch.as_tensor(idx, device=a.device)
    la, lb = [], []
    for t0, lr in STEPS:  # queued back to back
        la.append(a.step(r, ix, t0, lr))
    for t0, lr in STEPS:  # each followed by a synchronisation
        lb.append(b.step(r, ix, t0, lr))
        torch.cuda.synchronize()
    pa, pb = a.get_params(), b.get_params()
    assert pa.tobytes() == pb.tobytes()
    assert torch.stack(la).cpu().numpy().tobytes() == torch.stack(lb).cpu().numpy().tobytes()
    assert not np.array_equal(pa, p0)
    fresh = _trainer(LAYERS, 65, 5)
    fresh.step(r, ix, 2, 1e-3)
    a.set_params(p0, reset_optimizer=True)
    assert np.array_equal(a.get_params(), p0)
    a.step(r, ix, 2, 1e-3)
    assert a.get_params().tobytes() == fresh.get_params().tobytes()
    with pytest.raises(ValueError):  # a DKUC-sized vector is not this trainer's
        a.set_params(p0[:tk.blocks(LAYERS)[-1][2]])


@pytest.mark.gpu
@pytest.mark.parametrize("u_z", [0, 1])
def test_zero_h_agrees_with_the_linear_trainer(u_z):
    """H = 0: DBKN is DKUC.  Losses and the W, b, A, B gradient blocks against KoopmanTrainer on the same
    linear part and inputs, within the bar of the bilinear reference; the H block (not zero: dH does not
    depend on H at P = 1 and only through lambda beyond) against the reference's."""
    from lerobot_mujoco_sim2real_amd.control.koopman_train import KoopmanTrainer, params_to_net
    n, P, t0 = 65, 5, 1
    rows, idx, p, l64, g64, gs, ls = reference(LAYERS, n, P, t0, True, u_z, hscale=0.0)
    nlin = tk.blocks(LAYERS)[-1][2]
    assert not p[nlin:].any() and np.abs(g64[nlin:]).max() > 0
    lin = params_to_net(np.array(p[:nlin]), tk.make_net.__wrapped__(5, LAYERS))
    tl = KoopmanTrainer(lin, 130, pre_length=P, npos=NPOS, gamma=GAMMA, betas=(BETA1, BETA2), eps=EPS)
    tb = _trainer(LAYERS, 130, P, u_z, hscale=0.0)
    assert np.array_equal(tl.get_params(), tb.get_params()[:nlin])
    ll, gl = tk._loss_grad(tl, rows, idx, t0)
    lb, gb = tk._loss_grad(tb, rows, idx, t0)
    assert_losses(lb, ll, ls, "losses (H = 0) against the linear trainer")
    assert_losses(lb, l64, ls, "losses (H = 0)")
    assert_blocks(tk.blocks(LAYERS), gb, gl, gs, "grad(H=0) against the linear trainer", scale_from=g64)
    assert_blocks(blocks(LAYERS), gb, g64, gs, "grad(H=0)")


@pytest.mark.gpu
def test_trained_dbkn_model_feeds_the_controller():
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net, train
    from lerobot_mujoco_sim2real_amd.control.MPC_Controler import MPCController
    net = make_net.__wrapped__(2, LAYERS, 0, 0.0)  # H starts at zero, as the reference's does
    assert not net.H.weight.any()
    p0 = params_from_net(net)
    dev = torch.device("cuda", 0)
    rows = torch.as_tensor(tk.make_rows(40, 5), device=dev)
    hist = train(net, rows, epochs=2, batch_size=32, lr=1e-3, seed=3, eval_interval=1)
    assert len(hist["train_loss"]) == 2 and len(hist["eval"]) == 2 and hist["best_epoch"] in (0, 1)
    assert hist["best_params"].size == blocks(LAYERS)[-1][2]
    assert np.array_equal(params_from_net(net), hist["best_params"])
    assert not np.array_equal(hist["best_params"], p0)
    Hw = net.H.weight.detach()
    assert float(Hw.abs().max()) > 0 and bool(torch.isfinite(Hw).all())

    class args:  # noqa: N801
        x_dim, u_dim, MPC_type = XD, UD, "delta_mpc"
    ctl = MPCController(net, args)
    assert ctl.bilinear
    e = ctl.evaluate(rows)
    assert np.isfinite(e["avg_error"]) and e["avg_error"] == pytest.approx(hist["best_error"], rel=1e-12)
    # one control step of the trained model through k_bilinear
    n = 40
    zref = ctl.lift_reference(rows[:, :, UD:])                       # [T+1, nz, n]
    window = torch.zeros((ctl.H, ctl.Nkoopman, n), dtype=torch.float64, device=dev)
    window[:T] = zref[1:T + 1]
    u_prev = torch.zeros((UD, n), dtype=torch.float64, device=dev)
    action = ctl.step_bilinear(rows[0, :, UD:], window, u_prev)
    torch.cuda.synchronize()
    assert tuple(action.shape) == (n, UD) and bool(torch.isfinite(action).all()) and bool(torch.isfinite(u_prev).all())


@pytest.mark.gpu
def test_argument_errors():
    import torch
    from lerobot_mujoco_sim2real_amd import abi
    tr = _trainer(LAYERS, 16, 5, 1)
    lib = tr.lib
    rows = torch.as_tensor(tk.make_rows(20, 1), device=tr.device)
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
    d, o = _desc_opts()
    h = C.c_void_p()
    pp = p0.ctypes.data_as(C.c_void_p)

    def create(u_z=1):
        return lib.sim_koopman_trainer_create_bilinear(C.byref(d), pp, u_z, 16, C.byref(o), 0, C.byref(h))

    o.struct_size -= 8
    assert create() == abi.E_ARG and not h
    o.struct_size += 8
    o.abi_version += 1
    assert create() == abi.E_ARG and not h
    o.abi_version -= 1
    o.pre_length = 0
    assert create() == abi.E_ARG and not h
    o.pre_length = 5
    assert create(2) == abi.E_ARG and not h
    d.nlayer, d.width[6] = 6, 24
    d.width[5] = 64
    assert create() == abi.E_MODEL and not h
    assert b"nlayer" in lib.sim_last_error()
