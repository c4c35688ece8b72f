"""The Koopman controller kernels (csrc/koopman_mpc.hip: k_encode, k_feedforward, k_mpc_step;
koopman_bilinear.hip: k_bilinear; koopman_predict.hip: k_predict) across the shapes the ABI accepts,
against the float64 oracle.

test_koopman_mpc.py and test_koopman_predict.py run the kernels at the reference's shape (encoder
[8, 64, 64, 64, 64, 24], u_dim 5, horizon 10 or 7) and at [8, 64, 64, 40].  sim_koopman_create takes
x_dim 1..8, u_dim 1..8, 2..6 layers of width 1..64 and horizon 1..32 with H nz <= 1024, and
sim_koopman_set_bilinear nz <= 64 and N = H u_dim <= 64; the kernels pad everything to 16-row MFMA
tiles and 4-row k-steps, so the guards and the host packing matter exactly where widths are no
multiple of 4 or 16, x_dim < 8, u_dim != 5, nz > 32, H > 16 -- shapes the other modules never
visit.  tests/koopman_shapes_ref.py holds the table (one row per shape, each annotated with the
kernel path it is there for and the k_bilinear<epw> instantiation it yields), the nets, the frozen
inputs and the references; every test here is driven from it.

CPU tests pin the oracle at every row before the GPU is held to it: the literal cost loop has zero
gradient at KO.solve's answer, and two independent float64 constructions of the same minimiser --
control/koopman.condensed_gains (linear) and bilinear_first_move (DBKN) -- agree with
KO.get_control / get_control_bilinear.  Their disagreement over a case's own inputs is the float64
noise floor of that case.  The GPU tolerance stays the project's 1e-9 on u_prev (1e-6 on the
float32 action) wherever that floor is at most 1e-11, two decades of margin for the kernels'
different summation order; the CPU tests assert the floor, so a worse-conditioned row cannot be
added without noticing.  No row needed rescaling (a_scale 1, h_std 0.02 throughout).  Measured
floors, max over the row's checked frames (linear) or its batch sizes (bilinear):

    row    nz  nu   H    linear delta_mpc / mpc    bilinear delta_mpc / mpc
    ref    32   5  10    5.8e-14 / 4.9e-15         1.2e-14 / 8.9e-16
    nz48   48   5  10    3.8e-14 / 1.8e-15         8.0e-15 / 4.4e-16
    nz40   40   5  10    3.4e-14 / 4.4e-15         7.5e-15 / 6.1e-16
    nz45   45   5  10    8.7e-14 / 4.0e-15         1.1e-14 / 5.0e-16
    nz64   64   8   8    2.4e-14 / 3.1e-15         6.3e-15 / 6.7e-16
    odd    29   3   7    1.1e-14 / 3.6e-15         3.6e-15 / 5.0e-16
    tiny   13   1  20    3.3e-14 / 6.7e-16         3.4e-14 / 4.7e-16
    h32    32   2  32    2.8e-13 / 5.6e-15         3.9e-14 / 5.6e-16
    deep   14   4   9    2.2e-13 / 9.8e-15         9.1e-14 / 2.4e-15
    nz3     3   2   3    1.8e-14 / 5.8e-15         1.8e-14 / 3.6e-15

On an MI355X the kernels' largest deviation from the oracle over all these cases was 3.1e-13 on
u_prev, 3.4e-16 on the encoder's z and 6.7e-16 on the prediction: no row needed a kernel fix.

An encoder [3, 10] is one linear layer, which sim_koopman_create refuses (nlayer counts linear
layers, 2 .. 6; test_create_refuses_outside_the_limits), so the smallest row, `tiny`, is [3, 6, 10]:
nlayer 2, no hidden layer.  A batch of 16 epw - 3 envs fills only 15 workgroups at epw 2, so `nz64`
also runs 16 epw - 1.

The encoder keeps test_encode_gpu's rtol 1e-12 / atol 1e-13, the open-loop prediction
test_koopman_predict's atol 1e-11 on pred and rtol 1e-10 on err (T = 6 steps, fewer than that
module's 12), after the reference's own spread (float64 against longdouble and against the reversed
summation order) is asserted below 1e-13 on the same inputs.
"""
import ctypes as C

import numpy as np
import pytest

import koopman_mpc as KO
import koopman_shapes_ref as S

import soarm_pkg  # noqa: F401

NAMES = [r.name for r in S.TABLE]
FLOOR = 1e-11           # the float64 floor a row must meet to keep the 1e-9 bar
U_TOL, A_TOL = 1e-9, 1e-6
BIL_CASES = [(name, n) for name in NAMES for n in S.bilinear_sizes(name)]
BIL_IDS = [f"{name}-n{n}" for name, n in BIL_CASES]
MODELS = [("DKUC", False), ("DBKN", False), ("DBKN", True)]
SENTINEL = -7777.25


# ------------------------------------------------------------------------------------------ CPU
def test_shape_table_reaches_every_path():
    """The table's rows are inside the ABI's limits, yield the epw its comment states (by the
    restated LDS plan), and between them reach: epw 8, 6, 4 and 2; nz <= 32 and > 32, a multiple of 4
    and not, on both sides; H <= 16 and > 16; N % 4 != 0 and N = 64; x_dim < 8; u_dim 1 and 8; 2 and 6
    layers; one to four last-layer tiles; and batch sizes of 1, 2 and 16 workgroups (16: a multiple of
    8, the XCD-chunked mapping) with a ragged last one, 8 full ones at the control row."""
    for r in S.TABLE:
        xd, nu, nz, H = S.dims(r)
        assert 1 <= xd <= 8 and 1 <= nu <= 8 and 2 <= len(r.layers) - 1 <= 6 and 1 <= H <= 32
        assert all(1 <= w <= 64 for w in r.layers[1:]) and H * nz <= 1024 and nz <= 64 and H * nu <= 64
        ep = S.bilinear_epw(nz, nu, H)
        assert ep == S.EPW[r.name], (r.name, ep)
        sizes, ragged = S.bilinear_sizes(r.name), S.chunked_ragged(r.name)
        wg = lambda n: (n + ep - 1) // ep  # noqa: E731
        assert sizes[:3] == (1, ep + 1, 16 * ep - 3) and (wg(sizes[0]), wg(sizes[1])) == (1, 2) and sizes[1] % ep == 1
        assert ragged in sizes and wg(ragged) == 16 and ragged % ep != 0
    assert S.bilinear_sizes("ref")[3] == 64 and 64 // S.EPW["ref"] == 8
    d = [S.dims(r) for r in S.TABLE]
    assert {S.EPW[n] for n in NAMES} == {8, 6, 4, 2}
    for big in (False, True):
        assert {nz % 4 != 0 for _, _, nz, _ in d if (nz > 32) == big} == {False, True}
    assert {H > 16 for _, _, _, H in d} == {False, True}
    assert any((H * nu) % 4 for _, nu, _, H in d) and sum(H * nu == 64 for _, nu, _, H in d) >= 2
    assert any(H * nu == 64 and H > 16 for _, nu, _, H in d) and any(H * nu == 64 and nz == 64 for _, nu, nz, H in d)
    assert {xd for xd, _, _, _ in d} >= {2, 3, 5, 7, 8} and {nu for _, nu, _, _ in d} >= {1, 8}
    assert {len(r.layers) - 1 for r in S.TABLE} >= {2, 6}
    assert {(r.layers[-1] + 15) // 16 for r in S.TABLE} == {1, 2, 3, 4}
    assert any(nz < 4 for _, _, nz, _ in d) and any(H * nz == 1024 for _, _, nz, H in d)
    assert any((H * nz) % 16 for _, _, nz, H in d)
    for r in S.REFUSED[:2]:  # create takes them, set_bilinear must not
        xd, nu, nz, H = S.dims(r)
        assert H * nz <= 1024 and (nz > 64 or H * nu > 64)
    xd, nu, nz, H = S.dims(S.ROWS["cap"])
    assert H <= 32 and H * nz > 1024


def _assert_minimiser(A, B, z0, ref, up, kind, H):
    """test_oracle_minimises_the_reference_cost's check: the central-difference gradient of the
    literal cost loop is ~0 at KO.solve's answer and random perturbations cost more."""
    v = KO.solve(A, B, z0[None], ref[None], up[None], kind, H)[0].ravel()
    J0 = KO.cost(A, B, v, z0, ref, up, kind, H)
    h = 1e-6
    g = np.array([(KO.cost(A, B, v + h * e, z0, ref, up, kind, H) - KO.cost(A, B, v - h * e, z0, ref, up, kind, H)) / (2 * h)
                  for e in np.eye(v.size)])
    assert np.abs(g).max() < 1e-5 * max(1.0, abs(J0))
    rng = np.random.default_rng(v.size)
    for _ in range(20):
        assert KO.cost(A, B, v + rng.normal(0, 1e-3, v.size), z0, ref, up, kind, H) > J0


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_minimises_the_literal_cost_at_shapes(name, kind):
    """KO.solve minimises the reference's cost loop at the row's nz, u_dim and H, for the linear
    model and for the DBKN model's B_total(z0), on the first env of the GPU tests' own inputs."""
    H = S.ROWS[name].H
    A, B, _ = S.mats(S.make_net(name))
    c = S.linear_case(name, kind)
    f = c["frames"][0]
    _assert_minimiser(A, B, f["z0"][0], f["win"][0], c["up0"][0], kind, H)
    net = S.make_net(name, "DBKN")
    A, B, _ = S.mats(net)
    b = S.bilinear_case(name, kind, 1)
    _assert_minimiser(A, KO.b_total(B, net.get_Hi_numpy(), b["z0"][0]), b["z0"][0], b["ref"][0], b["up0"][0], kind, H)


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_condensed_gains_equal_oracle_at_shapes(name, kind):
    """The host closed form u0 = Gr r + Gz z0 + Gu u_prev == KO.get_control on the linear GPU test's
    inputs; their disagreement, the float64 floor of the case, is at most 1e-11."""
    floor = S.linear_floor(name, kind)
    print(f"{name} {kind}: linear float64 floor {floor:.2e}")
    assert floor <= FLOOR


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_bilinear_first_move_equals_oracle_at_shapes(name, kind):
    """control/koopman.bilinear_first_move == KO.get_control_bilinear on the bilinear GPU test's
    inputs, at every batch size; the float64 floor of the case is at most 1e-11."""
    floors = [S.bilinear_floor(name, kind, n) for n in S.bilinear_sizes(name)]
    print(f"{name} {kind}: bilinear float64 floors {['%.2e' % f for f in floors]}")
    assert max(floors) <= FLOOR


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_inputs_clip_some_actions_and_tell_envs_apart(name, kind):
    """What the GPU tests rely on: some, not all, linear actions saturate u_clip; and every env of the
    16-workgroup bilinear batch has its own answer, more than 1e-6 from every other env's, so a
    permuted workgroup -> env mapping cannot pass."""
    c = S.linear_case(name, kind)
    sat = np.mean([np.abs(f["u0"]) > KO.U_CLIP for f in c["frames"]])
    assert 0.03 < sat < 0.9, sat
    u0 = S.bilinear_case(name, kind, S.chunked_ragged(name))["u0"]
    dist = np.abs(u0[:, None, :] - u0[None, :, :]).max(-1) + np.eye(len(u0))
    assert dist.min() > 1e-6, dist.min()


def test_ref_predict_is_the_predict_tests_reference():
    """koopman_shapes_ref.ref_predict / predict_weights are test_koopman_predict's with x_dim and
    u_dim as arguments: at that module's shape they give the same bits."""
    import test_koopman_predict as P
    for key, relift in ((("DKUC", 0), 1), (("DBKN", 4, False), 0), (("DBKN", 4, True), 1)):
        net = P.make_net(*key)
        rows = P.make_rows(5, 6, 2)
        x, u = rows[:, :, P.UD:], rows[:, :, :P.UD]
        w0, w1 = P.weights(net), S.predict_weights(net)
        assert all(np.array_equal(a, b) for a, b in zip(w0[1:3], w1[1:3])) and (w0[3] is None) == (w1[3] is None)
        assert w0[3] is None or np.array_equal(w0[3], w1[3])
        np.testing.assert_array_equal(S.ref_predict(w1, x, u, relift), P.ref_predict(w0, x, u, relift))
        np.testing.assert_array_equal(S.ref_err(S.ref_predict(w1, x, u, relift), x, 3),
                                      P.ref_err(P.ref_predict(w0, x, u, relift), x))


@pytest.mark.parametrize("relift", [0, 1])
@pytest.mark.parametrize("model,u_z", MODELS, ids=["dkuc", "dbkn", "dbkn_uz"])
@pytest.mark.parametrize("name", S.PREDICT_ROWS)
def test_ref_predict_equals_open_loop_prediction_at_shapes(name, model, u_z, relift):
    """The numpy restatement == the torch loop over the model's own methods, 1e-12, at the rows of
    the GPU prediction test."""
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman import open_loop_prediction
    ud = S.ROWS[name].u_dim
    c = S.predict_case(name, model, u_z, 17, relift)
    r = torch.as_tensor(np.array(c["rows"])).transpose(0, 1)
    got = open_loop_prediction(S.make_net(name, model, u_z), r[:, :, ud:], r[:, :, :ud], relift=bool(relift))
    np.testing.assert_allclose(got.numpy().transpose(1, 0, 2), c["pred"], rtol=0, atol=1e-12)


def _desc(row):
    from lerobot_mujoco_sim2real_amd import abi
    d = abi.KoopmanDesc()
    d.x_dim, d.u_dim, d.nlayer, d.horizon, d.u_clip = row.layers[0], row.u_dim, len(row.layers) - 1, row.H, 0.5
    for i, w in enumerate(row.layers):
        d.width[i] = w
    return d


@pytest.mark.parametrize("name,msg", [("cap", b"horizon * nz"), ("nl1", b"nlayer")])
def test_create_refuses_outside_the_limits(name, msg):
    """H nz = 26 x 40 = 1040 > 1024, and an encoder of one linear layer ([3, 10]) -> SIM_E_MODEL with
    a message, before any device is touched."""
    from lerobot_mujoco_sim2real_amd import abi, build
    build.build()
    lib = abi.load_lib()
    row = S.ROWS[name]
    xd, nu, nz, H = S.dims(row)
    w, g, h = np.zeros(100000), np.zeros(nu * (H * nz + nz + nu)), C.c_void_p()
    rc = lib.sim_koopman_create(C.byref(_desc(row)), w.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), 0,
                                C.byref(h))
    assert rc == abi.E_MODEL and msg in lib.sim_last_error() and not h.value


# ------------------------------------------------------------------------------------------ GPU
def _ctl(name, kind="delta_mpc", model="DKUC", u_z=False):
    from lerobot_mujoco_sim2real_amd.control.MPC_Controler import MPCController
    row = S.ROWS[name]
    return MPCController(S.make_net(name, model, u_z), S.Args(row, kind, model), horizon=row.H)


def _dev(ctl, a):
    import torch
    return torch.as_tensor(np.array(a, order="C"), device=ctl.device)  # (a writable C-order copy of a frozen array)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_encode_shapes_gpu(gpu_lib, name):
    """k_encode == the numpy float64 MLP for one lane, a ragged wave, and two workgroups with a
    ragged tail; the x rows of z are x itself."""
    ctl = _ctl(name)
    xd = S.ROWS[name].layers[0]
    layers = S.make_net(name).encoder_layers()
    rng = np.random.default_rng([S.ROWS[name].seed, 4])
    for m in (1, 17, 70):
        x = S.states(rng, m, xd).astype(np.float32)
        z = ctl.encode(x).cpu().numpy().T
        want = KO.encode(layers, x.astype(np.float64))
        assert z.shape == want.shape
        print(f"{name} m={m}: max |z - ref| {np.abs(z - want).max():.3e}")
        np.testing.assert_array_equal(z[:, :xd], x.astype(np.float64))
        np.testing.assert_allclose(z, want, rtol=1e-12, atol=1e-13)


def _step_and_check(ctl, tag, up0, u0, a_want, **step):
    up = _dev(ctl, up0.T)
    a = ctl.step(step.pop("x", None), step.pop("ff"), up, **step).cpu().numpy()
    got = up.cpu().numpy().T
    print(f"{tag}: max |u0 - ref| {np.abs(got - u0).max():.3e}, max |a - ref| "
          f"{np.abs(a - a_want.astype(np.float32)).max():.3e}")
    np.testing.assert_allclose(got, u0, rtol=U_TOL, atol=U_TOL)
    np.testing.assert_allclose(a, a_want.astype(np.float32), atol=A_TOL)
    assert (np.abs(a) <= 0.5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_linear_control_shapes_gpu(gpu_lib, name, kind):
    """lift_reference -> feedforward -> step == KO.get_control at every row: T = 20 frames (the
    feedforward's second frame block), n = 70, frames 0, 15, 16, T - H and T - 1 (windows that run
    past the reference's end), some actions clipped."""
    c = S.linear_case(name, kind)
    ctl = _ctl(name, kind)
    zref_dev = ctl.lift_reference(_dev(ctl, c["sref"]))
    np.testing.assert_allclose(zref_dev.permute(0, 2, 1).cpu().numpy(), c["zref"], rtol=1e-12, atol=1e-13)
    ff = ctl.feedforward(zref_dev)
    assert tuple(ff.shape) == (S.T_LIN, S.ROWS[name].u_dim, S.N_LIN)
    for f in c["frames"]:
        _step_and_check(ctl, f"{name} {kind} frame {f['k']}", c["up0"], f["u0"], f["a"], x=_dev(ctl, f["x"]),
                        ff=ff[f["k"]])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("name", ["odd", "nz3", "deep"])
def test_linear_control_given_lifted_state_gpu(gpu_lib, name, kind):
    """step(z0=...) at x_dim 7, 2 and 5: the kernel reads the features at row x_dim + i of z0, not
    8 + i.  The z0 given is no encoder output (the encoder's plus noise), so it must be the one used."""
    row = S.ROWS[name]
    A, B, _ = S.mats(S.make_net(name))
    c = S.linear_case(name, kind)
    ctl = _ctl(name, kind)
    ff = ctl.feedforward(ctl.lift_reference(_dev(ctl, c["sref"])))
    f = c["frames"][1]
    z0 = f["z0"] + np.random.default_rng([row.seed, 5]).normal(0, 0.05, f["z0"].shape)
    u0, a = KO.get_control(A, B, z0, f["win"], c["up0"], kind, row.H)
    assert np.abs(u0 - f["u0"]).max() > 1e-3  # (the noise matters)
    _step_and_check(ctl, f"{name} {kind} z0 given", c["up0"], u0, a, ff=ff[f["k"]], z0=_dev(ctl, z0.T))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("name,n", BIL_CASES, ids=BIL_IDS)
def test_bilinear_control_shapes_gpu(gpu_lib, name, n, kind):
    """step_bilinear (k_encode + k_bilinear<epw>) == KO.get_control_bilinear at every row, for one
    env, epw + 1 envs (two workgroups, one live wave in the second), 16 epw - 3 (16 workgroups: the
    XCD-chunked mapping, a ragged last workgroup; every env's answer is its own; at epw 2 that is 15
    workgroups, so 16 epw - 1 runs too) and, at the control row, 8 epw (the chunked mapping with full
    workgroups, as the benchmark runs it)."""
    c = S.bilinear_case(name, kind, n)
    ctl = _ctl(name, kind, "DBKN")
    assert ctl.bilinear
    up = _dev(ctl, c["up0"].T)
    win = _dev(ctl, c["ref"].transpose(1, 2, 0))
    a = ctl.step_bilinear(_dev(ctl, c["x"]), win, up).cpu().numpy()
    got = up.cpu().numpy().T
    print(f"{name} {kind} n={n}: max |u0 - ref| {np.abs(got - c['u0']).max():.3e}")
    np.testing.assert_allclose(got, c["u0"], rtol=U_TOL, atol=U_TOL)
    np.testing.assert_allclose(a, c["a"].astype(np.float32), atol=A_TOL)


def _raw_predict(ctl, rows, relift, npos, xd, ud):
    """sim_koopman_predict on buffers one row longer than the kernel may write, sentinel-filled (as
    test_koopman_predict._raw_predict, any x_dim / u_dim)."""
    import torch
    T, n = rows.shape[0] - 1, rows.shape[1]
    r = _dev(ctl, rows)
    pred = torch.full(((T + 1) * n + 1, xd), SENTINEL, dtype=torch.float64, device=ctl.device)
    err = torch.full((2 * n + 1,), SENTINEL, dtype=torch.float64, device=ctl.device)
    rc = ctl.lib.sim_koopman_predict(ctl._h, n, T, C.c_void_p(r.data_ptr()), xd + ud, ud, 0, relift, npos,
                                     C.c_void_p(pred.data_ptr()), C.c_void_p(err.data_ptr()), None)
    torch.cuda.synchronize()
    p, e = pred.cpu().numpy(), err.cpu().numpy()
    return rc, p[:-1].reshape(T + 1, n, xd), e[:-1].reshape(2, n), bool((p[-1] == SENTINEL).all() and e[-1] == SENTINEL)


@pytest.mark.gpu
@pytest.mark.parametrize("relift", [0, 1])
@pytest.mark.parametrize("model,u_z", MODELS, ids=["dkuc", "dbkn", "dbkn_uz"])
@pytest.mark.parametrize("name", S.PREDICT_ROWS)
def test_predict_shapes_gpu(gpu_lib, name, model, u_z, relift):
    """k_predict == the float64 reference loop at x_dim 7 / 3 / 8 / 5, u_dim 3 / 1 / 8 / 4, one to
    four last-layer tiles, 2 and 6 layers; n = 1 and 17, T = 6.  Where set_model refuses the shape
    for LDS: SIM_E_MODEL and a message from set_model and predict, never a wrong answer."""
    from lerobot_mujoco_sim2real_amd import abi
    xd, ud, _, _ = S.dims(S.ROWS[name])
    ctl = _ctl(name, "delta_mpc", model, u_z)
    for n in (1, 17):
        c = S.predict_case(name, model, u_z, n, relift)
        if ctl._predict_refused is not None:
            r = _dev(ctl, c["rows"])
            rc = ctl.lib.sim_koopman_predict(ctl._h, n, S.T_PRED, C.c_void_p(r.data_ptr()), xd + ud, ud, 0, relift,
                                             c["npos"], None, None, None)
            assert rc == abi.E_MODEL and ctl.lib.sim_last_error() and "LDS" in ctl._predict_refused
            with pytest.raises(RuntimeError):
                ctl.predict(r)
            continue
        rc, pred, err, untouched = _raw_predict(ctl, c["rows"], relift, c["npos"], xd, ud)
        assert rc == 0, ctl.lib.sim_last_error()
        assert untouched, "a tail lane wrote past the n trajectories"
        print(f"{name} {model} u_z={u_z} n={n} relift={relift}: max |pred - ref| {np.abs(pred - c['pred']).max():.3e}")
        np.testing.assert_array_equal(pred[0], c["rows"][0, :, ud:].astype(np.float64))
        np.testing.assert_allclose(pred, c["pred"], rtol=0, atol=1e-11)
        np.testing.assert_allclose(err, c["err"], rtol=1e-10, atol=0)
        p2, e2 = ctl.predict(_dev(ctl, c["rows"]), relift=bool(relift), npos=c["npos"])  # the wrapper's ld / offsets
        assert np.array_equal(p2.cpu().numpy(), pred) and np.array_equal(e2.cpu().numpy(), err)


def _check_first_frame(ctl, name, kind="delta_mpc"):
    c = S.linear_case(name, kind)
    ff = ctl.feedforward(ctl.lift_reference(_dev(ctl, c["sref"])))
    f = c["frames"][0]
    _step_and_check(ctl, f"{name} {kind} frame 0", c["up0"], f["u0"], f["a"], x=_dev(ctl, f["x"]), ff=ff[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name,msg", [("n65", b"H * u_dim <= 64"), ("nz72", b"nz <= 64")])
def test_set_bilinear_refusal_leaves_the_linear_path_gpu(gpu_lib, name, msg):
    """N = 13 x 5 = 65 and nz = 8 + 64 = 72 on a live (linear) controller: sim_koopman_set_bilinear
    returns SIM_E_MODEL with a message, bilinear_step stays refused, and the controller's linear
    path still gives the oracle's answer."""
    import torch
    from lerobot_mujoco_sim2real_amd import abi
    xd, nu, nz, H = S.dims(S.ROWS[name])
    ctl = _ctl(name)
    A, B, _ = (np.ascontiguousarray(m) if isinstance(m, np.ndarray) else m for m in S.mats(S.make_net(name)))
    Hh = np.zeros((nz, nz, nu))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = ctl.lib.sim_koopman_set_bilinear(ctl._h, vp(A), vp(B), vp(Hh), 1, 50.0, 0.5)
    assert rc == abi.E_MODEL and msg in ctl.lib.sim_last_error()
    z0 = torch.zeros((nz, 1), dtype=torch.float64, device=ctl.device)
    win = torch.zeros((H, nz, 1), dtype=torch.float64, device=ctl.device)
    up = torch.zeros((nu, 1), dtype=torch.float64, device=ctl.device)
    act = torch.zeros((1, nu), dtype=torch.float32, device=ctl.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert ctl.lib.sim_koopman_bilinear_step(ctl._h, 1, p(z0), p(win), p(up), p(act), None) == abi.E_ARG
    _check_first_frame(ctl, name)


@pytest.mark.gpu
def test_create_refusal_then_a_controller_at_the_cap_gpu(gpu_lib):
    """H nz = 1040: MPCController raises with the library's message; the next controller, at
    H nz = 1024 exactly, is unaffected."""
    with pytest.raises(RuntimeError, match=r"horizon \* nz must be <= 1024"):
        _ctl("cap")
    _check_first_frame(_ctl("h32"), "h32")
