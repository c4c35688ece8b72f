"""The shape table of tests/test_koopman_shapes.py with its nets, inputs and float64 references.
Not collected: it holds no test.

Every case of the shape tests takes its inputs from here, built once per process and frozen
(read-only arrays), so the CPU tests that measure the float64 noise floor of a case and the GPU
tests that hold the kernels to 1e-9 see the same numbers.  The references are the project's own:
oracle/koopman_mpc.py (encode, get_control, get_control_bilinear, lifted_window, cost, solve) for
the control step and `ref_predict` below -- test_koopman_predict.ref_predict with x_dim and u_dim
as arguments instead of module constants -- for the open-loop prediction.
"""
import collections
import functools

import numpy as np

import koopman_mpc as KO

import soarm_pkg  # noqa: F401

LDS_BYTES = 160 * 1024
KINDS = ("delta_mpc", "mpc")

# One row per encoder / u_dim / horizon.  nz = layers[0] + layers[-1], N = H u_dim.  `epw` is the envs
# (waves) per workgroup that sim_koopman_set_bilinear derives for the row (`bilinear_epw` below
# restates its formula; test_shape_table_reaches_every_path asserts these figures), and the kernel
# instantiation is k_bilinear<epw>.  With 20480 doubles of LDS, per_env = xreg + mreg doubles per
# env and nz (nz + 1) for A:
#   ref      xs 165  xreg 1650  mreg  512  per_env 2162  A 1056  ->  8 (18352 <= 20480)
#   nz48     xs 261  xreg 2610  mreg  768  per_env 3378  A 2352  ->  4 (6: 22620 > 20480)
#   nz40     xs 229  xreg 2290  mreg  640  per_env 2930  A 1640  ->  6 (8: 25080 > 20480)
#   nz45     xs 229  xreg 2290  mreg  720  per_env 3010  A 2070  ->  6 (8: 26150 > 20480)
#   nz64     xs 520  xreg 4160  mreg 1088  per_env 5248  A 4160  ->  2 (4: 25152 > 20480)
#   odd      xs  99  xreg  694  mreg  320  per_env 1014  A  870  ->  8
#   tiny     xs  33  xreg  660  mreg  400  per_env 1060  A  182  ->  8
#   h32      xs  66  xreg 2112  mreg 2048  per_env 4160  A 1056  ->  4 (6: 26016 > 20480)
#   deep     xs  68  xreg  666  mreg  324  per_env  990  A  210  ->  8
#   nz3      xs  34  xreg  102  mreg  256  per_env  358  A   12  ->  8
# seed: torch.manual_seed of the net's constructor and the stream of every input of the row.
# a_scale multiplies lA.weight (0.9 x an orthogonal matrix as constructed: spectral radius 0.9
# a_scale <= 1); h_std is the standard deviation of the DBKN layer H.weight (the reference
# zero-initialises it; test_koopman_mpc.make_bnet draws it with 0.02).  Both are 1.0 / 0.02 unless
# the row's float64 floor (module docstring of test_koopman_shapes.py) needed better conditioning.
Row = collections.namedtuple("Row", "name layers u_dim H seed a_scale h_std bilinear linear")
TABLE = [
    Row("ref", (8, 64, 64, 64, 64, 24), 5, 10, 101, 1.0, 0.02,
        "control row: the static instantiation k_bilinear<8, 10, 5, 32>; n = 8 epw: the chunked mapping, full",
        "control row: two last-layer tiles"),
    Row("nz48", (8, 64, 64, 40), 5, 10, 102, 1.0, 0.02,
        "nz 48 > 32: dotn, A's fragments from LDS, NTz 3; epw 4",
        "three last-layer tiles"),
    Row("nz40", (8, 50, 32), 5, 10, 103, 1.0, 0.02,
        "nz 40 > 32; epw 6",
        "hidden width 50 (not a multiple of 16)"),
    Row("nz45", (8, 64, 37), 5, 10, 104, 1.0, 0.02,
        "nz 45 > 32 and nz % 4 = 1: dotn's scalar tail in B_total; KSz 12 with a ragged last k-step; epw 6",
        "last width 37: not a multiple of 4, three tiles"),
    Row("nz64", (8, 64, 56), 8, 8, 105, 1.0, 0.02,
        "nz 64, NTz 4; N 64; nu 8; epw 2",
        "four last-layer tiles; u_dim 8"),
    Row("odd", (7, 33, 17, 22), 3, 7, 106, 1.0, 0.02,
        "nz 29: nz % 4 != 0 on the nz <= 32 path (B_total's j >= (nz & ~3) tail); N 21: N % 4 != 0",
        "x_dim 7; odd hidden widths 33, 17; last width 22 (not a multiple of 4)"),
    # ([3, 10] itself is ONE linear layer, which sim_koopman_create refuses: nlayer counts linear
    # layers, 2 .. 6.  The same x_dim, nz and "no hidden layer" need three widths.)
    Row("tiny", (3, 6, 10), 1, 20, 107, 1.0, 0.02,
        "nlayer 2; nz 13 < 16; nu 1; H 20 > 16: rhs by dotn (tail: 13 % 4), the t >= 16 window load",
        "nlayer 2 (the hidden-layer loop is empty); width 6; one last-layer tile; x_dim 3; u_dim 1"),
    Row("h32", (8, 64, 24), 2, 32, 108, 1.0, 0.02,
        "H 32, N 64 through the H > 16 path; epw 4",
        "H nz = 1024, the cap; gr_ks 256"),
    Row("deep", (5, 64, 64, 64, 64, 64, 9), 4, 9, 109, 1.0, 0.02,
        "nlayer 6; nz 14",
        "nlayer 6; H nz = 126, not a multiple of 16 (zero Gr fragments); nz 14: the (t, j) walk wraps"),
    Row("nz3", (2, 1, 1), 2, 3, 110, 1.0, 0.02,
        "nz 3; N 6",
        "nz 3 < 4: feedforward's inner while loops run more than once; width 1; x_dim 2"),
]
# shapes sim_koopman_create accepts and sim_koopman_set_bilinear refuses (N = 65; nz = 72), and one
# two that create refuses (H nz = 1040 > 1024; nlayer 1); not part of TABLE
REFUSED = [
    Row("n65", (8, 64, 64, 64, 64, 24), 5, 13, 111, 1.0, 0.02, "refused: N = 65 > 64", "accepted"),
    Row("nz72", (8, 32, 64), 5, 10, 112, 1.0, 0.02, "refused: nz = 72 > 64", "accepted: last width 64, four tiles"),
    Row("cap", (8, 64, 32), 2, 26, 113, 1.0, 0.02, "refused at create", "refused at create: H nz = 1040"),
    Row("nl1", (3, 10), 1, 20, 114, 1.0, 0.02, "refused at create", "refused at create: one linear layer"),
]
ROWS = {r.name: r for r in TABLE + REFUSED}
EPW = {"ref": 8, "nz48": 4, "nz40": 6, "nz45": 6, "nz64": 2, "odd": 8, "tiny": 8, "h32": 4, "deep": 8, "nz3": 8}
PREDICT_ROWS = ("odd", "tiny", "nz64", "deep")


def dims(row):
    """(x_dim, u_dim, nz, H)"""
    return row.layers[0], row.u_dim, row.layers[0] + row.layers[-1], row.H


def bilinear_epw(nz, nu, H):
    """A RESTATEMENT of sim_koopman_set_bilinear's LDS plan (csrc/koopman_bilinear.hip), not a readback:
    the envs (waves) per workgroup it gives k_bilinear, or 0 where it refuses.  The ABI exposes no
    such figure; the tests need it to pick batch sizes that give one, two and sixteen workgroups."""
    N = H * nu
    xs = nz * nu + ((nu - nz * nu) % 32 + 32) % 32
    xreg = (max(H * xs, N * (N + 1) // 2) + 1) & ~1
    mreg = (max(nz * nu + (H + 1) * nz, N * H, 256) + 1) & ~1
    for ep in (8, 6, 4, 2, 1):
        if ((xreg + mreg) * ep + nz * (nz + 1)) * 8 <= LDS_BYTES:
            return ep
    return 0


class Args:
    """What MPCController reads of the reference's args."""

    def __init__(self, row, kind="delta_mpc", model="DKUC"):
        self.x_dim, self.u_dim, self.layers = row.layers[0], row.u_dim, list(row.layers)
        self.MPC_type, self.model = kind, model


@functools.lru_cache(maxsize=None)
def make_net(name, model="DKUC", u_z=False):
    """The project's Koopmanlinear / KoopmanBlinear for a row, float64, with the reference's
    initialisers; lA scaled by a_scale, DBKN's H drawn from N(0, h_std)."""
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman import KoopmanBlinear, Koopmanlinear
    row = ROWS[name]
    torch.manual_seed(row.seed)
    if model == "DKUC":
        net = Koopmanlinear(row.layers[0], row.u_dim, list(row.layers)).double()
    else:
        net = KoopmanBlinear(row.layers[0], row.u_dim, list(row.layers), u_z).double()
        with torch.no_grad():
            net.H.weight.normal_(0.0, row.h_std)
    with torch.no_grad():
        net.lA.weight.mul_(row.a_scale)
    return net


def mats(net):
    """(A, B, encoder layers) float64 numpy"""
    return (net.lA.weight.detach().numpy().astype(np.float64), net.lB.weight.detach().numpy().astype(np.float64),
            net.encoder_layers())


def states(rng, n, xd):
    """[n, xd]: the first xd columns of test_koopman_mpc.sample_states' SO-ARM101 state (ee xyz,
    joint angles)."""
    s = np.concatenate([rng.uniform([0.1, -0.2, 0.0], [0.45, 0.2, 0.35], (n, 3)), rng.uniform(-1.0, 1.0, (n, 5))], 1)
    return np.ascontiguousarray(s[:, :xd])


def _rng(row, *tag):
    return np.random.default_rng([row.seed, *tag])


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, list):
            for f in v:
                _freeze(f)
    return d


# ------------------------------------------------------------------------ linear control
T_LIN, N_LIN = 20, 70  # nframe > 16: feedforward's second frame block; two workgroups, a ragged tail


def linear_frames(H):
    """Frames 0, 15, 16 (the frame blocks' seam), T - H where valid (the last full window), T - 1."""
    fr = {0, 15, 16, T_LIN - 1}
    if 0 <= T_LIN - H < T_LIN:
        fr.add(T_LIN - H)
    return sorted(fr)


@functools.lru_cache(maxsize=None)
def linear_case(name, kind):
    """The linear-control inputs of a row and the oracle's answer: sref [T, n, xd] float32 (the
    reference trajectory), zref its float64 lift, up0 [n, ud] and per checked frame k: x [n, xd]
    float32, z0, u0 and the clipped action of KO.get_control.  up0 reaches past +-0.5, but a
    delta_mpc first move hardly depends on u_prev (Gu is small), so every third env's state is also
    2 to 8 times larger: between 5% and 82% of the actions clip in every row and kind
    (test_linear_inputs_saturate_some_actions).  The inputs do not depend on `kind`."""
    row = ROWS[name]
    xd, ud, nz, H = dims(row)
    A, B, layers = mats(make_net(name))
    rng = _rng(row, 1)
    sref = states(rng, T_LIN * N_LIN, xd).reshape(T_LIN, N_LIN, xd).astype(np.float32)
    zref = KO.encode(layers, sref.reshape(-1, xd).astype(np.float64)).reshape(T_LIN, N_LIN, nz)
    up0 = rng.uniform(-0.6, 0.6, (N_LIN, ud))
    amp = np.where(np.arange(N_LIN) % 3 == 0, rng.uniform(2.0, 8.0, N_LIN), 1.0)[:, None]
    qp = KO.prepare(A, B, H, kind)
    frames = []
    for k in linear_frames(H):
        x = (amp * states(rng, N_LIN, xd)).astype(np.float32)
        z0 = KO.encode(layers, x.astype(np.float64))
        win = KO.lifted_window(zref, k, H)
        u0, a = KO.get_control(A, B, z0, win, up0, kind, H, qp=qp)
        frames.append(_freeze(dict(k=k, x=x, z0=z0, win=win, u0=u0, a=a)))
    return _freeze(dict(sref=sref, zref=zref, up0=up0, frames=frames))


def linear_floor(name, kind):
    """max |condensed_gains' u0 - KO.get_control's u0| over the case's frames: two independent
    float64 constructions of one minimiser."""
    from lerobot_mujoco_sim2real_amd.control.koopman import condensed_gains
    row = ROWS[name]
    A, B, _ = mats(make_net(name))
    c = linear_case(name, kind)
    Gr, Gz, Gu = condensed_gains(A, B, row.H, kind)
    return max(float(np.abs(f["win"].reshape(N_LIN, -1) @ Gr.T + f["z0"] @ Gz.T + c["up0"] @ Gu.T - f["u0"]).max())
               for f in c["frames"])


# ---------------------------------------------------------------------- bilinear control
def chunked_ragged(name):
    """The batch of 16 workgroups (a multiple of 8: the XCD-chunked mapping) with a ragged last one:
    16 epw - 3, or 16 epw - 1 where epw <= 3 (16 epw - 3 then fills only 15 workgroups)."""
    ep = EPW[name]
    return 16 * ep - (3 if ep > 3 else 1)


def bilinear_sizes(name):
    """One env; epw + 1: two workgroups, the second with one live wave; 16 epw - 3; chunked_ragged
    where that is another size; and at the control row 8 epw: the chunked mapping with full workgroups."""
    ep = EPW[name]
    sizes = [1, ep + 1, 16 * ep - 3]
    if chunked_ragged(name) not in sizes:
        sizes.append(chunked_ragged(name))
    return tuple(sizes) + ((8 * ep,) if name == "ref" else ())


@functools.lru_cache(maxsize=None)
def bilinear_case(name, kind, n):
    """The DBKN inputs of a row for n envs (x [n, xd] float32, ref [n, H, nz], up0 [n, ud], every
    env's own draw) and KO.get_control_bilinear's (u0, a)."""
    row = ROWS[name]
    xd, ud, nz, H = dims(row)
    net = make_net(name, "DBKN")
    A, B, layers = mats(net)
    rng = _rng(row, 2, n)
    x = states(rng, n, xd).astype(np.float32)
    z0 = KO.encode(layers, x.astype(np.float64))
    ref = KO.encode(layers, states(rng, n * H, xd)).reshape(n, H, nz)
    up0 = rng.uniform(-0.5, 0.5, (n, ud))
    u0, a = KO.get_control_bilinear(A, B, net.get_Hi_numpy(), z0, ref, up0, kind, H)
    return _freeze(dict(x=x, z0=z0, ref=ref, up0=up0, u0=u0, a=a))


def bilinear_floor(name, kind, n):
    """max |bilinear_first_move's u0 - KO.get_control_bilinear's u0| over the case's envs."""
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman import bilinear_first_move
    row = ROWS[name]
    net = make_net(name, "DBKN")
    A, B, _ = mats(net)
    c = bilinear_case(name, kind, n)
    u0 = bilinear_first_move(torch.as_tensor(A), torch.as_tensor(B), torch.as_tensor(np.stack(net.get_Hi_numpy())),
                             torch.as_tensor(c["z0"].T.copy()), torch.as_tensor(c["ref"].transpose(1, 2, 0).copy()),
                             torch.as_tensor(c["up0"].T.copy()), kind, row.H).numpy().T
    return float(np.abs(u0 - c["u0"]).max())


# ------------------------------------------------------------------- open-loop prediction
T_PRED = 6
SPREAD = 1e-13  # as test_koopman_predict: float64 against longdouble and against the reversed order


def predict_weights(net):
    """test_koopman_predict.weights for any u_dim: (layers, A, B, Hhat [j][i][c] or None) from the
    raw parameters (H vec(z (x) u): the coefficient of z_j u_c in column j u_dim + c; with u_z,
    vec(u (x) z): column c nz + j)."""
    sd = {k: v.detach().numpy().astype(np.float64) for k, v in net.state_dict().items()}
    nl = sum(1 for k in sd if k.startswith("x_encode_net") and k.endswith("weight"))
    layers = [(sd[f"x_encode_net.linear_{i}.weight"], sd[f"x_encode_net.linear_{i}.bias"]) for i in range(nl)]
    A, B = sd["lA.weight"], sd["lB.weight"]
    Hhat = None
    if "H.weight" in sd:
        nz, ud = B.shape
        Hw = sd["H.weight"]
        Hhat = (Hw.reshape(nz, ud, nz).transpose(2, 0, 1) if net.u_z else Hw.reshape(nz, nz, ud).transpose(1, 0, 2)).copy()
    return layers, A, B, Hhat


def ref_predict(w, x, u, relift, dt=np.float64, reverse=False):
    """test_koopman_predict.ref_predict with x_dim read from x: x [T+1, n, xd], u [T+1, n, ud] ->
    pred [T+1, n, xd] in dtype dt; reverse: every contraction summed in the opposite order."""
    layers, A, B, Hhat = w
    xd = x.shape[2]
    fl = (lambda a, ax: np.ascontiguousarray(np.flip(a, ax))) if reverse else (lambda a, ax: a)

    def mm(a, Wt):
        return fl(a, 1) @ fl(Wt, 0)

    def psi(xx):
        h = xx
        for i, (W, b) in enumerate(layers):
            h = mm(h, W.T.astype(dt)) + b.astype(dt)
            if i + 1 < len(layers):
                h = np.maximum(h, 0)
        return np.concatenate([xx, h], -1)

    x, u = x.astype(dt), u.astype(dt)
    At, Bt = A.T.astype(dt), B.T.astype(dt)
    xh = x[0]
    z = psi(xh)
    pred = [xh]
    for t in range(x.shape[0] - 1):
        zn = mm(z, At) + mm(u[t], Bt)
        if Hhat is not None:
            zu = (z[:, :, None] * u[t][:, None, :]).reshape(z.shape[0], -1)
            zn = zn + mm(zu, Hhat.transpose(0, 2, 1).reshape(-1, z.shape[1]).astype(dt))
        xh = zn[:, :xd]
        pred.append(xh)
        z = psi(xh) if relift else zn
    return np.stack(pred)


def ref_err(pred, x, npos):
    d = np.abs(pred[1:] - x[1:].astype(pred.dtype))
    return np.stack([d[:, :, :npos].sum((0, 2)), d[:, :, npos:].sum((0, 2))])


@functools.lru_cache(maxsize=None)
def predict_case(name, model, u_z, n, relift):
    """rows [T+1, n, ud + xd] float32 ([u | x], as the data generator's rollout), the float64
    prediction and its err [2, n] at npos = min(3, xd); the reference's own spread (float64 against
    longdouble and against the reversed summation order) is asserted below SPREAD first."""
    row = ROWS[name]
    xd, ud, _, _ = dims(row)
    w = predict_weights(make_net(name, model, u_z))
    rng = _rng(row, 3, n)
    x = states(rng, (T_PRED + 1) * n, xd).reshape(T_PRED + 1, n, xd)
    rows = np.concatenate([rng.uniform(-0.5, 0.5, (T_PRED + 1, n, ud)), x], -1).astype(np.float32)
    x, u = rows[:, :, ud:], rows[:, :, :ud]
    p64 = ref_predict(w, x, u, relift)
    for other in (ref_predict(w, x, u, relift, np.longdouble), ref_predict(w, x, u, relift, reverse=True)):
        spread = float(np.abs(p64 - other).max())
        assert spread < SPREAD, f"reference spread {spread:.2e}"
    npos = min(3, xd)
    return _freeze(dict(rows=rows, pred=p64, err=ref_err(p64, x, npos), npos=npos))
