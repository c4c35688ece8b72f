"""The Koopman training step (include/koopman_mpc.h sim_koopman_trainer_*, sim_koopman_loss_grad,
sim_koopman_train_step; control/koopman_train.py) against a numpy restatement of the reference.

The reference (train(), train.py:89-266, over k_linear_loss, models/losses.py:54-129, "mse", with
torch.optim.Adam): n windows of P = pre_length steps; z^_0 = Psi(x_t0), z^_{i+1} = A z^_i + B u_i;
koopman / pred / dis / angle are gamma^i-weighted means of squared errors against Psi(x_{t0+i+1})
and x_{t0+i+1}; total = koopman + pred (recon is identically 0: lC Psi(x) = x).  `ref_loss_grad`
below is that forward and its hand-written backward in numpy from the flat parameter vector,
`ref_adam` the update; no product code computes them.  A CPU test checks the float64 gradient
against torch.autograd on this project's Koopmanlinear.

Tolerances follow test_koopman_predict.py: per test input the reference's own spread is measured
-- per parameter block (W_l, b_l, A, B), max |float64 - np.longdouble| and max |float64 - reversed
summation order| over the block, divided by the block's max |g| -- and asserted below SPREAD
(1e-12: an ill-conditioned input cannot hide a failure).  The product is held to two decades above
that spread (the spread taken no smaller than float64's epsilon, 2.2e-16, below which it cannot be
resolved), and never looser than 1e-9, the control step's bar, relative to the block's max |g|.
Losses: the same rule as an rtol; parameters after Adam steps: the same rule on the parameters.
Measured on the CPU over the GPU tests' inputs (reference encoder and [8, 64, 64, 40], n = 1 .. 130,
P = 1 and 5): gradient spreads 5e-17 .. 1.4e-15 per block, so the bars are 2.2e-14 .. 1.4e-13; loss
spreads <= 5.3e-16 (bar 5.3e-14); parameter spreads after 1 and after 5 Adam steps <= 6.1e-15 per block
(bars <= 6.1e-13).  Measured on an MI355X against those bars: gradient error <= 1.3e-15, loss error
<= 8.0e-16, parameter error <= 3.1e-15 -- at most 3% of its bar in every block.

Condition on the inputs: a ReLU whose pre-activation is within rounding of zero may take either
branch, so every reference asserts min |pre-activation| over all hidden units and samples >= 1e-9
(no sample excluded; measured: 7.8e-8 at the least over these inputs).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import soarm_pkg  # noqa: F401

LAYERS = (8, 64, 64, 64, 64, 24)   # the reference's encoder (args.py:103): two last-layer tiles
LAYERS3 = (8, 64, 64, 40)          # three last-layer tiles, nl = 3
XD, UD, NPOS, GAMMA = 8, 5, 3, 0.8
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
SPREAD, BAR, F64EPS = 1e-12, 1e-9, 2.220446049250313e-16
PRE_MIN = 1e-9
SENTINEL = -7777.25
T = 7


# ------------------------------------------------------------------------------------ the reference
def blocks(layers):
    """[(name, start, stop)] of the flat parameter vector [W_0 | b_0 | ... | A | B]."""
    out, o = [], 0
    for l, (a, b) in enumerate(zip(layers[:-1], layers[1:])):
        out.append((f"W{l}", o, o + a * b)), out.append((f"b{l}", o + a * b, o + a * b + b))
        o += a * b + b
    nz = XD + layers[-1]
    out.append(("A", o, o + nz * nz)), out.append(("B", o + nz * nz, o + nz * nz + nz * UD))
    return out


def unpack(p, layers):
    bl = {n: p[a:b] for n, a, b in blocks(layers)}
    nl, nz = len(layers) - 1, XD + layers[-1]
    Ws = [bl[f"W{l}"].reshape(layers[l + 1], layers[l]) for l in range(nl)]
    return Ws, [bl[f"b{l}"] for l in range(nl)], bl["A"].reshape(nz, nz), bl["B"].reshape(nz, UD)


def ref_loss_grad(p, layers, x, u, P, dt=np.float64, reverse=False):
    """x [P+1, n, x_dim], u [P, n, u_dim] (float32 data, widened) -> (losses [6], grad [nparam],
    min |hidden pre-activation|) in dtype dt.  reverse: every contraction summed in the opposite order."""
    fl = (lambda a, ax: np.ascontiguousarray(np.flip(a, ax))) if reverse else (lambda a, ax: a)

    def mm(a, b):  # a [m, k] @ b [k, q]
        return fl(a, 1) @ fl(b, 0)

    Ws, bs, A, B = [[w.astype(dt) for w in g] if isinstance(g, list) else g.astype(dt) for g in unpack(p, layers)]
    x, u = x.astype(dt), u.astype(dt)
    nl, n, nz = len(Ws), x.shape[1], A.shape[0]
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
    dA, dB = np.zeros_like(A), np.zeros_like(B)
    lam = g[P]
    for i in range(P - 1, -1, -1):
        dA += mm(lam.T, zh[i])
        dB += mm(lam.T, u[i])
        lam = mm(lam, A) + (g[i] if i > 0 else 0)
    for acts, gam in enc:
        psi_backward(acts, gam, dW, db)
    psi_backward(acts0, lam[:, XD:], dW, db)
    grad = np.concatenate([np.concatenate([w.ravel(), b]) for w, b in zip(dW, db)] + [dA.ravel(), dB.ravel()])
    return losses, grad, premin[0]


def ref_adam(p, m, v, g, t, lr):
    """torch.optim.Adam's update (no weight decay), step count t >= 1, in g's dtype."""
    dt = g.dtype.type
    m = dt(BETA1) * m + (1 - dt(BETA1)) * g
    v = dt(BETA2) * v + (1 - dt(BETA2)) * g * g
    bc1, bc2 = 1 - dt(BETA1) ** t, 1 - dt(BETA2) ** t
    return p - (dt(lr) / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + dt(EPS)), m, v


def block_spread(layers, a, others):
    """per block: max over `others` of max |a - o| / max |a|"""
    out = {}
    for name, s, e in blocks(layers):
        out[name] = max(float(np.abs(a[s:e] - o[s:e].astype(np.float64)).max()) for o in others) / float(np.abs(a[s:e]).max())
    return out


def assert_blocks(layers, got, want, spread, what):
    """got == want per block within min(100 * max(spread, eps), 1e-9) * max |want|; prints each figure"""
    bad = []
    for name, s, e in blocks(layers):
        assert spread[name] < SPREAD, f"{what}: reference spread {spread[name]:.2e} in block {name}"
        scale = float(np.abs(want[s:e]).max())
        bar = min(100 * max(spread[name], F64EPS), BAR)
        err = float(np.abs(got[s:e] - want[s:e]).max()) / scale
        print(f"{what} {name}: err {err:.2e} bar {bar:.2e} spread {spread[name]:.2e}")
        if not err <= bar:
            bad.append((name, err, bar))
    assert not bad, f"{what}: {bad}"


@functools.lru_cache(maxsize=None)
def make_net(seed=1, layers=LAYERS):
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman import Koopmanlinear
    torch.manual_seed(seed)
    return Koopmanlinear(XD, UD, list(layers)).double()


def make_rows(N, seed):
    """[T+1, N, 13] fp32 rows [u | x]: x from the control tests' state sampler, u ~ U(-0.5, 0.5)."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform([0.1, -0.2, 0.0], [0.45, 0.2, 0.35], (T + 1, N, 3)),
                        rng.uniform(-1.0, 1.0, (T + 1, N, 5))], -1)
    u = rng.uniform(-0.5, 0.5, (T + 1, N, UD))
    return np.concatenate([u, x], -1).astype(np.float32)


def make_idx(n, N, seed):
    """a permutation of 0..N-1 cut to n, with repeats (entry 0 copied over the odd entries' second)"""
    idx = np.random.default_rng(seed).permutation(N)[:n].astype(np.int32)
    if n > 2:
        idx[2] = idx[0]
    return idx


def window(rows, idx, t0, P):
    w = rows[t0:t0 + P + 1][:, idx]
    return w[:, :, UD:], w[:P, :, :UD]


_REF = {}


def reference(layers, n, P, t0, use_idx, seed=1):
    """(rows, idx or None, params, losses f64, grad f64, grad spread per block, loss spread), computed
    once per case and shared.  The ReLU condition is asserted here."""
    key = (layers, n, P, t0, use_idx, seed)
    if key not in _REF:
        from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net
        N = n + 5 if use_idx else n
        rows = make_rows(N, seed + 10)
        idx = make_idx(n, N, seed + 20) if use_idx else None
        p = params_from_net(make_net(seed, layers))
        x, u = window(rows, idx if use_idx else np.arange(n), t0, P)
        l64, g64, premin = ref_loss_grad(p, layers, x, u, P)
        assert premin >= PRE_MIN, f"a hidden pre-activation of {premin:.2e} is within rounding of zero: change the seed"
        lld, gld, _ = ref_loss_grad(p, layers, x, u, P, np.longdouble)
        lrv, grv, _ = ref_loss_grad(p, layers, x, u, P, reverse=True)
        gs = block_spread(layers, g64, [gld, grv])
        nzl = [0, 1, 2, 4, 5]
        ls = max(float(np.abs((l64[nzl] - o[nzl].astype(np.float64)) / l64[nzl]).max()) for o in (lld, lrv))
        assert ls < SPREAD, f"reference loss spread {ls:.2e}"
        for a in (rows, p, l64, g64):
            a.setflags(write=False)
        _REF[key] = (rows, idx, p, l64, g64, gs, ls)
    return _REF[key]


# ------------------------------------------------------------------------------------------- CPU
def torch_loss(net, x, u, P):
    """the section-2 loss on this project's Koopmanlinear (float64 torch), for autograd"""
    import torch
    beta = [GAMMA ** i for i in range(P)]
    cont = sum(beta)
    z = net.x_encoder(x[0])
    koop = pred = 0.0
    for i in range(P):
        z = net.koopman_operation(z, u[i])
        koop = koop + beta[i] * torch.mean((z - net.x_encoder(x[i + 1])) ** 2)
        pred = pred + beta[i] * torch.mean((net.x_decoder(z) - x[i + 1]) ** 2)
    return koop / cont + pred / cont


@pytest.mark.parametrize("layers,n,P", [(LAYERS, 17, 5), (LAYERS3, 5, 1), (LAYERS, 1, 5)])
def test_reference_gradient_equals_autograd(layers, n, P):
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net
    rows, _, p, l64, g64, _, _ = reference(layers, n, P, 1, False)
    net = make_net(1, layers)
    x, u = window(rows, np.arange(n), 1, P)
    net.zero_grad()
    loss = torch_loss(net, torch.as_tensor(x.astype(np.float64)), torch.as_tensor(u.astype(np.float64)), P)
    loss.backward()
    gnet = make_net.__wrapped__(1, layers)  # a second net to carry the gradients as parameters
    with torch.no_grad():
        for a, b in zip(gnet.parameters(), net.parameters()):
            a.copy_(b.grad if b.grad is not None else torch.zeros_like(b))
    want = params_from_net(gnet)
    net.zero_grad()
    assert abs(float(loss.detach()) - l64[0]) <= 1e-13 * abs(l64[0])
    for name, s, e in blocks(layers):
        scale = np.abs(want[s:e]).max()
        assert np.abs(g64[s:e] - want[s:e]).max() <= 1e-12 * scale, name


def test_params_round_trip():
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net, params_to_net
    net = make_net(3, LAYERS3)
    p = params_from_net(net)
    assert p.dtype == np.float64 and p.size == blocks(LAYERS3)[-1][2]
    Ws, bs, A, B = unpack(p, LAYERS3)
    assert np.array_equal(A, net.lA.weight.detach().numpy()) and np.array_equal(B, net.lB.weight.detach().numpy())
    assert np.array_equal(Ws[1], net.x_encode_net.linear_1.weight.detach().numpy())
    assert np.array_equal(bs[2], net.x_encode_net.linear_2.bias.detach().numpy())
    other = make_net.__wrapped__(4, LAYERS3)
    assert not np.array_equal(params_from_net(other), p)
    params_to_net(p, other)
    assert np.array_equal(params_from_net(other), p)
    assert torch.equal(other.lC.weight, net.lC.weight)
    with pytest.raises(ValueError):
        params_to_net(p[:-1], other)


def test_schedule_is_a_pure_function_of_its_seed():
    from lerobot_mujoco_sim2real_amd.control.koopman_train import schedule
    a, b, c = schedule(5, 37, 20, 5, 16, 3), schedule(5, 37, 20, 5, 16, 3), schedule(6, 37, 20, 5, 16, 3)
    assert len(a) == 3 and all(len(ep) == 3 for ep in a)
    for ea, eb in zip(a, b):
        for (ia, ta), (ib, tb) in zip(ea, eb):
            assert np.array_equal(ia, ib) and ta == tb and ia.dtype == np.int32
    assert any(not np.array_equal(x[0], y[0]) for ea, ec in zip(a, c) for x, y in zip(ea, ec))
    for ep in a:
        assert sorted(np.concatenate([i for i, _ in ep]).tolist()) == list(range(37))
        assert [len(i) for i, _ in ep] == [16, 16, 5]
        assert all(0 <= t0 <= 20 - 5 - 1 for _, t0 in ep)
    assert a[0][0][0].tolist() != a[1][0][0].tolist()


def test_trainer_entry_points_are_exported():
    from lerobot_mujoco_sim2real_amd import abi, build
    names = ["sim_koopman_trainer_nparam", "sim_koopman_trainer_create", "sim_koopman_trainer_free",
             "sim_koopman_trainer_get_params", "sim_koopman_trainer_set_params", "sim_koopman_loss_grad",
             "sim_koopman_train_step"]
    for name in names:
        assert name in abi.EXPORTS
    build.build()
    lib = abi.load_lib()
    assert len(lib.sim_koopman_loss_grad.argtypes) == 13 and len(lib.sim_koopman_train_step.argtypes) == 13
    o = abi.KoopmanTrainOpts()
    assert o.struct_size == C.sizeof(abi.KoopmanTrainOpts) == 48 and o.abi_version == abi.ABI_VERSION
    o.pre_length, o.npos, o.gamma, o.beta1, o.beta2, o.eps = 5, NPOS, GAMMA, BETA1, BETA2, EPS
    d = abi.KoopmanDesc()
    d.x_dim, d.u_dim, d.nlayer, d.horizon, d.u_clip = XD, UD, len(LAYERS) - 1, 10, 0.5
    for i, w in enumerate(LAYERS):
        d.width[i] = w
    assert lib.sim_koopman_trainer_nparam(C.byref(d)) == blocks(LAYERS)[-1][2]
    import torch
    if not torch.cuda.is_available():  # no GPU: creation fails loudly, as sim_koopman_create does
        from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net
        p, h = params_from_net(make_net()), C.c_void_p()
        assert lib.sim_koopman_trainer_create(C.byref(d), p.ctypes.data_as(C.c_void_p), 16, C.byref(o), 0, C.byref(h)) == -4
        assert not h
    rows = np.zeros((2, 1, 13), np.float32)
    rp = rows.ctypes.data_as(C.c_void_p)
    assert lib.sim_koopman_loss_grad(None, 1, 1, 1, rp, 13, 5, 0, None, 0, None, None, None) == abi.E_ARG
    assert lib.sim_koopman_train_step(None, 1, 1, 1, rp, 13, 5, 0, None, 0, 1e-3, None, None) == abi.E_ARG


def test_unbuilt_models_and_losses_are_refused():
    from lerobot_mujoco_sim2real_amd.control.koopman import KoopmanBlinear
    from lerobot_mujoco_sim2real_amd.control.koopman_train import KoopmanTrainer
    with pytest.raises(NotImplementedError, match="DBKN"):
        KoopmanTrainer(KoopmanBlinear(XD, UD, list(LAYERS)).double(), 16)
    with pytest.raises(NotImplementedError, match="mse"):
        KoopmanTrainer(make_net(), 16, loss_name="mae")


# ------------------------------------------------------------------------------------------- GPU
def _trainer(layers=LAYERS, max_batch=130, P=5, seed=1):
    from lerobot_mujoco_sim2real_amd.control.koopman_train import KoopmanTrainer
    return KoopmanTrainer(make_net(seed, layers), max_batch, pre_length=P, npos=NPOS, gamma=GAMMA, betas=(BETA1, BETA2), eps=EPS)


def relayout(rows):
    """the rows in a second layout: ld = 16, [pad 2 | x 8 | pad 1 | u 5], padding filled with junk"""
    out = np.full(rows.shape[:2] + (16,), 9.75e3, np.float32)
    out[:, :, 2:10], out[:, :, 11:16] = rows[:, :, UD:], rows[:, :, :UD]
    return out, 16, 2, 11


def _loss_grad(tr, rows, idx, t0, layout=(13, UD, 0), pad=0):
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


CASES = [(layers, n, P, last) for layers in (LAYERS, LAYERS3) for n in (1, 16, 17, 65, 130) for P in (1, 5)
         for last in (0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("layers,n,P,last", CASES,
                         ids=[f"{'ref' if c[0] is LAYERS else 'nl3'}-n{c[1]}-P{c[2]}-{'tail' if c[3] else 't0'}" for c in CASES])
def test_loss_grad_matches_reference(layers, n, P, last):
    """n: one lane, a full wave, one past it, one past a workgroup, several workgroups; the window at
    row 0 and ending on row T; traj_idx NULL / a permutation with repeats into a larger N and the
    in-place / second layout alternate over the cases so that each meets every n and both P."""
    k = (1, 16, 17, 65, 130).index(n)
    use_idx, alt = bool((k + last) % 2), bool((k + P // 5 + (layers is LAYERS3)) % 2)
    t0 = T - P if last else 0
    rows, idx, p, l64, g64, gs, ls = reference(layers, n, P, t0, use_idx)
    tr = _trainer(layers, 130, P)
    assert np.array_equal(tr.get_params(), p)
    r, *layout = relayout(rows) if alt else (rows, 13, UD, 0)
    losses, grad = _loss_grad(tr, r, idx, t0, tuple(layout))
    assert losses[3] == 0.0
    nzl = [0, 1, 2, 4, 5]
    lerr = float(np.abs((losses[nzl] - l64[nzl]) / l64[nzl]).max())
    lbar = min(100 * max(ls, F64EPS), BAR)
    print(f"losses: err {lerr:.2e} bar {lbar:.2e} spread {ls:.2e}")
    assert lerr <= lbar
    assert_blocks(layers, grad, g64, gs, "grad")
    assert np.array_equal(tr.get_params(), p)  # loss_grad changes no state


@pytest.mark.gpu
def test_loss_grad_is_reproducible_and_keeps_to_its_buffer():
    rows, idx, p, *_ = reference(LAYERS, 130, 5, 2, True)
    tr = _trainer()
    l1, g1 = _loss_grad(tr, rows, idx, 2, pad=64)
    l2, g2 = _loss_grad(tr, rows, idx, 2, pad=64)
    assert l1.tobytes() == l2.tobytes() and g1.tobytes() == g2.tobytes()
    assert np.all(g1[tr.nparam:] == SENTINEL) and not np.any(g1[:tr.nparam] == SENTINEL)
    # grad and losses may be NULL
    import torch
    r = torch.as_tensor(np.array(rows), device=tr.device)
    assert tr.lib.sim_koopman_loss_grad(tr._h, 5, rows.shape[1], T, C.c_void_p(r.data_ptr()), 13, UD, 0, None, 0, None, None,
                                        tr._stream()) == 0
    torch.cuda.synchronize()


STEPS = [(0, 1e-3), (2, 5e-4), (1, 2e-3), (2, 1e-3), (0, 7e-4)]  # (t0, lr) per step


@functools.lru_cache(maxsize=None)
def adam_reference(layers, n, nsteps, seed=1):
    """parameters after 1 .. nsteps reference steps in float64, and their spread per block against
    the same steps in longdouble and with reversed sums"""
    rows, idx, p0, *_ = reference(layers, n, 5, 0, True, seed)
    runs = []
    for dt, rev in ((np.float64, False), (np.longdouble, False), (np.float64, True)):
        p, m, v, traj = p0.astype(dt), np.zeros_like(p0, dtype=dt), np.zeros_like(p0, dtype=dt), []
        for t, (t0, lr) in enumerate(STEPS[:nsteps], 1):
            x, u = window(rows, idx, t0, 5)
            _, g, premin = ref_loss_grad(p.astype(np.float64) if dt is np.float64 else p, layers, x, u, 5, dt, rev)
            assert premin >= PRE_MIN
            p, m, v = ref_adam(p, m, v, g, t, lr)
            traj.append(p)
        runs.append(traj)
    out = []
    for k in range(nsteps):
        out.append((runs[0][k], block_spread(layers, runs[0][k], [runs[1][k], runs[2][k]])))
    return rows, idx, out


@pytest.mark.gpu
@pytest.mark.parametrize("layers", [LAYERS, LAYERS3], ids=["ref", "nl3"])
def test_train_steps_match_reference_adam(layers):
    import torch
    n = 65
    rows, idx, want = adam_reference(layers, n, 5)
    tr = _trainer(layers, n, 5)
    r = torch.as_tensor(np.array(rows), device=tr.device)
    ix = torch.as_tensor(idx, device=tr.device)
    for k, (t0, lr) in enumerate(STEPS):
        tr.step(r, ix, t0, lr)
        if k in (0, 4):
            assert_blocks(layers, tr.get_params(), want[k][0], want[k][1], f"params after {k + 1} steps")
    # the fragment copies follow the master vector: the next gradient is that of the updated parameters
    p5 = tr.get_params()
    x, u = window(rows, idx, 1, 5)
    l64, g64, premin = ref_loss_grad(p5, layers, x, u, 5)
    assert premin >= PRE_MIN
    losses, grad = tr.loss_grad(r, ix, 1)
    sp = block_spread(layers, g64, [ref_loss_grad(p5, layers, x, u, 5, np.longdouble)[1], ref_loss_grad(p5, layers, x, u, 5, reverse=True)[1]])
    assert_blocks(layers, grad.cpu().numpy(), g64, sp, "grad after 5 steps")


@pytest.mark.gpu
def test_queued_steps_equal_synchronised_steps_and_reset():
    import torch
    rows, idx, p0, *_ = reference(LAYERS, 65, 5, 0, True)
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
    # set_params(..., reset_optimizer=1) then a step == the first step of a fresh trainer
    fresh = _trainer(LAYERS, 65, 5)
    fresh.step(r, ix, 2, 1e-3)
    a.set_params(p0, reset_optimizer=True)
    assert np.array_equal(a.get_params(), p0)
    a.step(r, ix, 2, 1e-3)
    assert a.get_params().tobytes() == fresh.get_params().tobytes()
    # without the reset the optimizer's state carries over
    b.set_params(p0, reset_optimizer=False)
    b.step(r, ix, 2, 1e-3)
    assert b.get_params().tobytes() != fresh.get_params().tobytes()


@pytest.mark.gpu
def test_round_trip_and_trained_model_feeds_the_controller():
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net, train
    from lerobot_mujoco_sim2real_amd.control.MPC_Controler import MPCController
    net = make_net.__wrapped__(2, LAYERS)
    from lerobot_mujoco_sim2real_amd.control.koopman_train import KoopmanTrainer
    tr = KoopmanTrainer(net, 32)
    assert np.array_equal(tr.get_params(), params_from_net(net))
    rows = torch.as_tensor(make_rows(40, 5), device=tr.device)
    hist = train(net, rows, epochs=2, batch_size=32, lr=1e-3, seed=3, eval_interval=1)
    assert len(hist["train_loss"]) == 2 and len(hist["eval"]) == 2 and hist["best_epoch"] in (0, 1)
    assert np.array_equal(params_from_net(net), hist["best_params"])
    assert not np.array_equal(hist["best_params"], tr.get_params())

    class args:  # noqa: N801
        x_dim, u_dim, MPC_type = XD, UD, "delta_mpc"
    e = MPCController(net, args).evaluate(rows)
    assert np.isfinite(e["avg_error"]) and e["avg_error"] == pytest.approx(hist["best_error"], rel=1e-12)
    assert tuple(e["all_preds"].shape) == (40, T + 1, XD)


@pytest.mark.gpu
def test_argument_errors():
    import torch
    from lerobot_mujoco_sim2real_amd import abi
    tr = _trainer(LAYERS, 16, 5)
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
    assert both(4, 20, T, rp, 13, UD, 0, T - 5)[0] == 0       # the last valid window
    torch.cuda.synchronize()
    # a bad struct header, a model past the kernel's plan
    d = abi.KoopmanDesc()
    d.x_dim, d.u_dim, d.nlayer, d.horizon, d.u_clip = XD, UD, len(LAYERS) - 1, 10, 0.5
    for i, w in enumerate(LAYERS):
        d.width[i] = w
    o = abi.KoopmanTrainOpts()
    o.pre_length, o.npos, o.gamma, o.beta1, o.beta2, o.eps = 5, NPOS, GAMMA, BETA1, BETA2, EPS
    h = C.c_void_p()
    pp = p0.ctypes.data_as(C.c_void_p)
    o.struct_size -= 8
    assert lib.sim_koopman_trainer_create(C.byref(d), pp, 16, C.byref(o), 0, C.byref(h)) == abi.E_ARG and not h
    o.struct_size += 8
    o.abi_version += 1
    assert lib.sim_koopman_trainer_create(C.byref(d), pp, 16, C.byref(o), 0, C.byref(h)) == abi.E_ARG and not h
    o.abi_version -= 1
    o.pre_length = 0
    assert lib.sim_koopman_trainer_create(C.byref(d), pp, 16, C.byref(o), 0, C.byref(h)) == abi.E_ARG and not h
    o.pre_length = 5
    d.nlayer, d.width[6] = 6, 24
    d.width[5] = 64
    assert lib.sim_koopman_trainer_create(C.byref(d), pp, 16, C.byref(o), 0, C.byref(h)) == abi.E_MODEL and not h
    assert b"nlayer" in lib.sim_last_error()
