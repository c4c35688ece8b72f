"""The DBKN control step with input limits (csrc/koopman_bilinear.hip k_bilinear_box:
sim_koopman_set_bilinear_box, sim_koopman_bilinear_box_step; control/koopman.box_plan_bilinear;
MPCController.set_box_bilinear / step_box_bilinear; KoopmanMPCTracking(constrained=True) on a prepared
DBKN controller) against a float64 reference that uses no project code.

tests/koopman_box_bilinear_ref.py holds that reference -- per env the oracle's own quadratic at the
env's linearised input matrix (oracle/koopman_mpc.py: b_total, prepare), mapped to the model inputs w as
tests/koopman_box_ref.py maps the DKUC one and solved by its projected Gauss-Seidel to a natural residual
of 1e-14 -- on koopman_box_ref's frozen inputs: rows ref (both Kronecker orders; the static
instantiation), odd (N 21, nz 29), nz64 (N 64, u_dim 8, 2 envs per workgroup), tiny (H 20, u_dim 1) and
nz3 (N 6), both kinds, 130 envs (n = 1, 17 and 130).

What a solver's answer w is held to (box_plan_bilinear on the CPU, the kernel on the GPU), at tol = 1e-9:
ok = 1; lo <= w <= hi exactly; per env ||w - w_ref||_2 <= 2 (Lhat_e / mu_e) sqrt(N) tol + 1e-11 with the
env's own P_e; u0 as koopman_box_ref.applied; and where the reference's multiplier at an active bound
exceeds Lhat_e (tol + bound_e) the iterate IS the bound (every entry of a Gauss-Seidel iterate is a
projection, and within bound_e of the solution the gradient entry it is projected with is within
Lhat_e bound_e of that multiplier: it points out of the box, so the entry lands on the bound itself).

The kernel does not factorise (include/koopman_mpc.h): an env whose unconstrained minimiser is interior
is iterated like every other and is held to the error bound, not to iters = 0.  Its stop test runs after
every sweep, so the kernel's iters are held to box_plan_bilinear's exactly.

max_iter = 1: ok = 1 exactly on the envs whose natural residual after one sweep from clip(0) -- restated
here on the reference's P_e and g_e, in the kernel's order (the time blocks from the last to the first)
-- is <= tol; an env within 1e-12 of the threshold (the rounding of the restatement: 1e-16 |g| N) is not
asserted either way.
"""
import ctypes as C

import numpy as np
import pytest

import koopman_box_bilinear_ref as RB
import koopman_box_ref as R
import koopman_mpc as KO
import koopman_shapes_ref as S

import soarm_pkg  # noqa: F401

SENTINEL = -7777.25
cases = pytest.mark.parametrize("name,u_z,kind", RB.CASES, ids=RB.IDS)


def _held_to_the_reference(tag, c, w, u0, ok, n):
    """The assertions of the module docstring on a solver's plan w [n, N] for the case's leading n envs."""
    lo, hi, wr, bound = c["lo"][:n], c["hi"][:n], c["w"][:n], c["bound"][:n]
    err = np.linalg.norm(w - wr, axis=1)
    print(f"{tag}: ok {int(np.sum(ok))}/{n}  max |w - w_ref|_2 / bound {(err / bound).max():.3e} (bounds "
          f"{bound.min():.2e} .. {bound.max():.2e})")
    assert (np.asarray(ok) == 1).all()
    assert (w >= lo).all() and (w <= hi).all()
    assert (err <= bound).all()
    q0 = dict(kind=c["kind"], nu=c["nu"])
    np.testing.assert_array_equal(u0, R.applied(q0, w, c["up"][:n]))
    assert (np.abs(u0) <= RB.U_MAX).all()
    assert (np.abs(u0 - c["u0"][:n]).max(1) <= bound).all()
    grad, thr = c["grad"][:n], (c["Lhat"][:n] * (RB.TOL + bound))[:, None]
    at_lo, at_hi = (wr <= lo) & (grad > thr), (wr >= hi) & (-grad > thr)
    assert n < RB.N_ENV or at_lo.any() or at_hi.any()
    np.testing.assert_array_equal(w[at_lo], lo[at_lo])
    np.testing.assert_array_equal(w[at_hi], hi[at_hi])


def _plan(c, n=None, **kw):
    from lerobot_mujoco_sim2real_amd.control import koopman as K
    n = RB.N_ENV if n is None else n
    return K.box_plan_bilinear(c["A"], c["B"], c["Hhat"], c["z0"][:n], c["ref"][:n], c["up"][:n], c["kind"], c["H"],
                               RB.U_MAX, RB.TOL, **kw)


def _one_sweep_residual(c):
    """The natural residual after one sweep from clip(0) in the kernel's order, on the reference's
    problem (no project code)."""
    P, g, lo, hi, nu, H = c["P"], c["g"], c["lo"], c["hi"], c["nu"], c["H"]
    w = np.clip(np.zeros_like(g), lo, hi)
    dg = np.einsum("nii->ni", P)
    for a in range(c["N"]):
        i = (H - 1 - a // nu) * nu + a % nu
        w[:, i] = np.clip((g[:, i] - (w * P[:, i]).sum(1) + dg[:, i] * w[:, i]) / dg[:, i], lo[:, i], hi[:, i])
    return w, RB.residual(P, c["Lhat"], w, g, lo, hi)


# ------------------------------------------------------------------------------------------ CPU
@cases
def test_inputs_exercise_the_bounds(name, u_z, kind):
    """With the reference alone: >= 20% of envs have a bound active on the first move, >= 10% none at
    all, and at least one has a bound active at some t >= 1 but none at t = 0."""
    c = RB.case(name, u_z, kind)
    later = c["act_any"] & ~c["act0"]
    print(f"{name} {u_z} {kind}: first move {c['act0'].mean():.2f}, none {(~c['act_any']).mean():.2f}, later only "
          f"{later.sum()}, cond {(np.linalg.eigvalsh(c['P'])[:, -1] / c['mu']).max():.1f}")
    assert c["act0"].mean() >= 0.20 and (~c["act_any"]).mean() >= 0.10 and later.sum() >= 1
    assert c["act_any"][:17].any() and not c["act_any"][:17].all()


def test_batched_pgs_is_the_box_refs_pgs():
    """koopman_box_bilinear_ref.pgs (a matrix per env) against koopman_box_ref.pgs on single envs: an
    interior env, one active on the first move and one active only later."""
    c = RB.case("odd", False, "delta_mpc")
    for e in (int(np.argmax(~c["act_any"])), int(np.argmax(c["act0"])), int(np.argmax(c["act_any"] & ~c["act0"]))):
        Q = RB.env_quadratic(c["A"], c["B"], c["Hhat"], c["z0"][e], c["H"], c["kind"])
        np.testing.assert_array_equal(Q["P"], c["P"][e])
        w = R.pgs(Q, c["g"][e:e + 1], c["lo"][e:e + 1], c["hi"][e:e + 1])
        np.testing.assert_allclose(w[0], c["w"][e], rtol=0, atol=1e-13)


@cases
def test_box_plan_bilinear_against_the_reference(name, u_z, kind):
    """control/koopman.box_plan_bilinear (the kernel's iteration in numpy) is held to the reference at
    n = 1, 17 and 130 (the same iters at every n); max_iter = 1 by the module
    docstring's rule, the output still inside the box."""
    c = RB.case(name, u_z, kind)
    full = _plan(c)
    _held_to_the_reference(f"{name} {u_z} {kind} box_plan_bilinear (iters {full[3].min()} .. {full[3].max()})", c,
                           *full[:3], RB.N_ENV)
    assert full[3].min() >= 1 and full[3].max() <= 64  # (half the default cap, 128)
    for n in RB.SIZES[:2]:  # (numpy's own summation order depends on the batch: held to the reference, not bitwise)
        part = _plan(c, n)
        _held_to_the_reference(f"{name} {u_z} {kind} n={n}", c, *part[:3], n)
        np.testing.assert_array_equal(part[3], full[3][:n])
    w, u0, ok, iters = _plan(c, max_iter=1)
    assert (w >= c["lo"]).all() and (w <= c["hi"]).all() and (np.abs(u0) <= RB.U_MAX).all()
    np.testing.assert_array_equal(iters, 1)
    _, res = _one_sweep_residual(c)
    sure = np.abs(res - RB.TOL) > 1e-12
    np.testing.assert_array_equal(ok[sure], (res <= RB.TOL)[sure].astype(np.int32))
    assert (ok == 0).any()


def test_python_refusals_that_need_no_device():
    """The new methods refuse a DKUC net and point to set_box; set_box / step_box on a DBKN net keep
    raising 'DKUC only' and name the new methods.  (The refusals come before anything touches the
    library, so a controller object without one shows them.)"""
    from lerobot_mujoco_sim2real_amd.control.MPC_Controler import MPCController
    dk, bl = object.__new__(MPCController), object.__new__(MPCController)
    dk.bilinear, bl.bilinear = False, True
    dk.torch = bl.torch = None
    for call in (lambda: dk.set_box_bilinear(), lambda: dk.step_box_bilinear(None, None, None)):
        with pytest.raises(NotImplementedError, match="DBKN only.*set_box"):
            call()
    for call in (lambda: bl.set_box(), lambda: bl.step_box(None, None, None)):
        with pytest.raises(NotImplementedError, match="DKUC only.*set_box_bilinear"):
            call()


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctls(gpu_lib):
    """One DBKN controller per (row, u_z, kind, options), set_box_bilinear called."""
    made = {}

    def get(name, u_z, kind, **box):
        from lerobot_mujoco_sim2real_amd.control.MPC_Controler import MPCController
        key = (name, u_z, kind, tuple(sorted(box.items())))
        if key not in made:
            row = S.ROWS[name]
            made[key] = MPCController(S.make_net(name, "DBKN", u_z), S.Args(row, kind, "DBKN"), horizon=row.H)
            made[key].set_box_bilinear(**box)
        return made[key]
    return get


def _dev(ctl, a):
    import torch
    return torch.as_tensor(np.array(a, order="C"), device=ctl.device)


def _raw_step(ctl, c, sl, want=("plan", "ok", "iters")):
    """sim_koopman_bilinear_box_step on the case's envs sl, through the raw ABI on sentinel-padded
    buffers; `want`: which of the optional outputs are passed (the others NULL)."""
    import torch
    n = len(c["up"][sl])
    nu, H = ctl.u_dim, ctl.H
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def padded(a, dt):
        t = torch.full((a.size + 8,), SENTINEL, dtype=dt, device=ctl.device)
        t[:a.size] = torch.as_tensor(np.array(a, order="C").ravel(), device=ctl.device).to(dt)
        return t
    upd = padded(c["up"][sl].T, torch.float64)
    pl = padded(np.zeros((H * nu, n)), torch.float64)
    act = padded(np.zeros((n, nu)), torch.float32)
    ok = padded(np.zeros(n), torch.int32)
    it = padded(np.zeros(n), torch.int32)
    z0 = _dev(ctl, c["z0"][sl].T)
    win = _dev(ctl, c["ref"][sl].transpose(1, 2, 0))
    rc = ctl.lib.sim_koopman_bilinear_box_step(ctl._h, n, p(z0), p(win), p(upd), p(pl) if "plan" in want else None, p(act),
                                               p(ok) if "ok" in want else None, p(it) if "iters" in want else None, None)
    torch.cuda.synchronize()
    tails = [t[-8:].double().cpu().numpy() for t in (upd, pl, act, ok, it)]
    cut = lambda t, k: t[:k].cpu().numpy()  # noqa: E731
    return dict(rc=rc, plan=cut(pl, H * nu * n).reshape(H * nu, n).T.copy(), up=cut(upd, nu * n).reshape(nu, n).T.copy(),
                action=cut(act, n * nu).reshape(n, nu), ok=cut(ok, n), iters=cut(it, n),
                untouched=all(((t == SENTINEL) | (t == int(SENTINEL))).all() for t in tails))  # (int32: -7777)


@pytest.mark.gpu
@cases
def test_bilinear_box_step_against_the_reference_gpu(ctls, name, u_z, kind):
    """sim_koopman_bilinear_box_step at n = 1, 17 and 130: the plan (natural order) is held to the
    reference; iters equal box_plan_bilinear's and w is within the bound of its w; u_prev is the applied
    input, action its float32; nothing is written past n; the optional outputs may be NULL."""
    c, ctl = RB.case(name, u_z, kind), ctls(name, u_z, kind)
    wp, _, _, itp = _plan(c)
    for n in RB.SIZES:
        o = _raw_step(ctl, c, slice(0, n))
        assert o["rc"] == 0, ctl.lib.sim_last_error()
        assert o["untouched"], "a write past the n envs"
        _held_to_the_reference(f"{name} {u_z} {kind} n={n} (iters {o['iters'].min()} .. {o['iters'].max()})", c, o["plan"],
                               o["up"], o["ok"], n)
        np.testing.assert_array_equal(o["action"], o["up"].astype(np.float32))
        assert (np.abs(o["action"]) <= RB.U_MAX).all()
        np.testing.assert_array_equal(o["iters"], itp[:n])
        assert (np.linalg.norm(o["plan"] - wp[:n], axis=1) <= c["bound"][:n]).all()
        assert o["iters"].max() <= 64  # (half the default cap, 128)
    bare = _raw_step(ctl, c, slice(0, 17), want=())
    assert bare["rc"] == 0 and bare["untouched"]
    np.testing.assert_array_equal(bare["up"], o["up"][:17])
    assert (bare["plan"] == 0).all() and (bare["ok"] == 0).all() and (bare["iters"] == 0).all()  # (never passed)


@pytest.mark.gpu
@cases
def test_env_results_do_not_depend_on_n_gpu(ctls, name, u_z, kind):
    """Env k's outputs are bit-identical at n = 17 and n = 130."""
    c, ctl = RB.case(name, u_z, kind), ctls(name, u_z, kind)
    a, b = _raw_step(ctl, c, slice(0, 17)), _raw_step(ctl, c, slice(0, RB.N_ENV))
    for key in ("plan", "up", "action", "ok", "iters"):
        np.testing.assert_array_equal(a[key], b[key][:17], err_msg=key)


@pytest.mark.gpu
@cases
def test_failure_stays_safe_gpu(ctls, name, u_z, kind):
    """max_iter = 1: ok by the rule of the module docstring; iters = 1; every output inside the box."""
    c, ctl = RB.case(name, u_z, kind), ctls(name, u_z, kind, max_iter=1)
    o = _raw_step(ctl, c, slice(0, RB.N_ENV))
    assert o["rc"] == 0
    assert (o["plan"] >= c["lo"]).all() and (o["plan"] <= c["hi"]).all()
    assert (np.abs(o["up"]) <= RB.U_MAX).all() and (np.abs(o["action"]) <= RB.U_MAX).all()
    np.testing.assert_array_equal(o["iters"], 1)
    _, res = _one_sweep_residual(c)
    sure = np.abs(res - RB.TOL) > 1e-12
    np.testing.assert_array_equal(o["ok"][sure], (res <= RB.TOL)[sure].astype(np.int32))
    assert (o["ok"] == 0).any()


@pytest.mark.gpu
def test_refusals_on_the_device_gpu(gpu_lib):
    """bilinear_box_step before set_bilinear_box -> SIM_E_ARG; bad options -> SIM_E_ARG, the step then
    refused while bilinear_step still gives the oracle's answer; NULL arguments and n = -1 -> SIM_E_ARG;
    n = 0 -> 0; a set_bilinear after set_bilinear_box drops the box state; set_bilinear_box without
    set_bilinear (a DKUC controller) -> SIM_E_ARG."""
    import torch
    import test_koopman_shapes as TS
    from lerobot_mujoco_sim2real_amd import abi
    name, kind = "odd", "delta_mpc"
    ctl = TS._ctl(name, kind, "DBKN")
    lib, h = ctl.lib, ctl._h
    xd, nu, nz, H = S.dims(S.ROWS[name])
    c = S.bilinear_case(name, kind, 1)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    z0, win = _dev(ctl, c["z0"].T), _dev(ctl, c["ref"].transpose(1, 2, 0))
    up = _dev(ctl, c["up0"].T)
    act = torch.zeros((1, nu), dtype=torch.float32, device=ctl.device)
    step = lambda n=1, k=h, a=p(z0), b=p(win), u=p(up), ac=p(act): \
        lib.sim_koopman_bilinear_box_step(k, n, a, b, u, None, ac, None, None, None)  # noqa: E731

    def bilinear_step_is_the_oracles():
        u = _dev(ctl, c["up0"].T)
        assert lib.sim_koopman_bilinear_step(h, 1, p(z0), p(win), p(u), p(act), None) == 0
        torch.cuda.synchronize()
        np.testing.assert_allclose(u.cpu().numpy().T, c["u0"], rtol=1e-9, atol=1e-9)
    assert step() == abi.E_ARG and b"set_bilinear_box" in lib.sim_last_error()
    assert lib.sim_koopman_set_bilinear_box(h, None) == 0 and step() == 0
    for field, value in (("struct_size", 8), ("abi_version", 99)):
        o = abi.KoopmanBoxOpts()
        setattr(o, field, value)
        assert lib.sim_koopman_set_bilinear_box(h, C.byref(o)) == abi.E_ARG and b"struct_size" in lib.sim_last_error()
        assert step() == abi.E_ARG  # (the refusal took the earlier set_bilinear_box with it)
    for kw, msg in ((dict(u_max=0.0), b"u_max"), (dict(u_max=-0.5), b"u_max"), (dict(tol=0.0), b"tol"),
                    (dict(max_iter=0), b"max_iter")):
        assert lib.sim_koopman_set_bilinear_box(h, C.byref(abi.KoopmanBoxOpts(**kw))) == abi.E_ARG
        assert msg in lib.sim_last_error()
        assert step() == abi.E_ARG
    bilinear_step_is_the_oracles()
    assert lib.sim_koopman_set_bilinear_box(None, None) == abi.E_ARG
    assert lib.sim_koopman_set_bilinear_box(h, C.byref(abi.KoopmanBoxOpts())) == 0
    for kw in (dict(k=None), dict(a=None), dict(b=None), dict(u=None), dict(ac=None), dict(n=-1)):
        assert step(**kw) == abi.E_ARG
    assert step(n=0) == 0 and step() == 0
    torch.cuda.synchronize()
    A, B, Hh = RB.model(name, False)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.sim_koopman_set_bilinear(h, vp(A), vp(B), vp(Hh), 1, 50.0, 0.5) == 0
    assert step() == abi.E_ARG  # (a later set_bilinear drops the box state)
    bilinear_step_is_the_oracles()
    dk = TS._ctl(name, kind)  # (DKUC: set_bilinear was never called)
    assert dk.lib.sim_koopman_set_bilinear_box(dk._h, None) == abi.E_ARG and b"set_bilinear" in lib.sim_last_error()
    TS._check_first_frame(dk, name)
    # every row of the shape table is accepted
    for row in S.TABLE:
        ct = TS._ctl(row.name, kind, "DBKN")
        assert ct.lib.sim_koopman_set_bilinear_box(ct._h, None) == 0, row.name


@pytest.mark.gpu
@pytest.mark.parametrize("kind", S.KINDS)
def test_bilinear_step_is_unchanged_by_set_bilinear_box_gpu(gpu_lib, kind):
    """sim_koopman_bilinear_step after a set_bilinear_box (and a box step) gives the same u0 and action
    as before it, bit for bit, on row ref."""
    import torch
    import test_koopman_shapes as TS
    ctl = TS._ctl("ref", kind, "DBKN")
    c = RB.case("ref", False, kind)
    z0, win = _dev(ctl, c["z0"].T), _dev(ctl, c["ref"].transpose(1, 2, 0))
    out = []
    for rep in range(2):
        up = _dev(ctl, c["up"].T)
        act = ctl.step_bilinear(None, win, up, z0=z0)
        torch.cuda.synchronize()
        out.append((up.clone(), act.clone()))
        if rep == 0:
            ctl.set_box_bilinear()
            ctl.step_box_bilinear(None, win, _dev(ctl, c["up"].T), z0=z0)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", S.KINDS)
def test_get_control_constrained_gpu(ctls, kind):
    """get_control(p, constrained=True) on a prepared DBKN controller, single env, on an env with a
    bound active on the first move and one active only later: u0 is the reference's within the bound,
    inside the limit, a == u0; an unprepared DBKN controller raises as before."""
    import test_koopman_shapes as TS
    c, ctl = RB.case("ref", False, kind), ctls("ref", False, kind)
    for e in (int(np.argmax(c["act0"])), int(np.argmax(c["act_any"] & ~c["act0"]))):
        ctl.u_prev = c["up"][e].copy()  # ('mpc' reads the controller's own u_prev)
        p = np.concatenate([c["ref"][e].ravel(), c["z0"][e], c["up"][e]])
        u0, a = ctl.get_control(p, constrained=True)
        assert np.abs(u0 - c["u0"][e]).max() <= c["bound"][e]
        assert (np.abs(u0) <= RB.U_MAX).all() and np.array_equal(a, u0)
    with pytest.raises(NotImplementedError, match="DKUC only"):
        TS._ctl("ref", kind, "DBKN").get_control(p, constrained=True)


@pytest.mark.gpu
def test_tracking_constrained_gpu(gpu_lib, arm_model):
    """KoopmanMPCTracking(constrained=True) on a prepared DBKN controller, 6 frames, 4 envs, on a
    reference amplified until the unconstrained run's actions clip: every applied action is inside
    [-u_max, u_max] with no clip applied (u_prev, the unclipped u0, is inside too), ok is all 1, and at
    every frame the reference, fed the device's recorded state, window and u_prev, reproduces u0 within
    the bound."""
    import test_koopman_shapes as TS
    from lerobot_mujoco_sim2real_amd.Koopman_MPC import KoopmanMPCTracking
    kind, T, n, H = "delta_mpc", 10, 4, 10
    net = S.make_net("ref", "DBKN")
    A, B, Hhat = RB.model("ref", False)
    layers = net.encoder_layers()
    rng = np.random.default_rng(41)
    t = np.linspace(0, 2 * np.pi, T)
    phase = rng.uniform(0, 2 * np.pi, n)
    amp = np.array([1.0, 4.0, 8.0, 8.0])
    cart = np.stack([0.3 + 0.05 * amp * np.sin(2 * (t[:, None] + phase)), 0.1 * amp * np.cos(t[:, None] + phase),
                     0.15 + 0.05 * amp * np.sin(t[:, None] + phase)], -1)
    jq = rng.uniform(-0.3, 0.3, (1, n, 5)) + 0.1 * amp[None, :, None] * np.sin(t[:, None, None] + phase[None, :, None])
    free = KoopmanMPCTracking(TS._ctl("ref", kind, "DBKN"), arm_model, cart, jq)
    free.runBefore()
    clipped = 0
    for k in range(6):
        free.runFunc()
        clipped += int((free.u_prev.abs() > RB.U_MAX).sum())
    assert clipped > 0, "the unconstrained run never clips: amplify the reference"
    with pytest.raises(NotImplementedError, match="DKUC only unless set_box_bilinear"):
        KoopmanMPCTracking(TS._ctl("ref", kind, "DBKN"), arm_model, cart, jq, constrained=True)
    ctl = TS._ctl("ref", kind, "DBKN")
    ctl.set_box_bilinear()
    run = KoopmanMPCTracking(ctl, arm_model, cart, jq, constrained=True)
    sref = run.state_all_ref.cpu().numpy().astype(np.float64)
    zref = KO.encode(layers, sref.reshape(T * n, 8)).reshape(T, n, -1)
    run.runBefore()
    active = 0
    for k in range(6):
        x = run.state.cpu().numpy().astype(np.float64)
        up = run.u_prev.cpu().numpy().T.copy()
        run.runFunc()
        w, u0, bound = RB.solve(A, B, Hhat, KO.encode(layers, x), KO.lifted_window(zref, k, H), up, H, kind)
        got, a = run.u_prev.cpu().numpy().T, run.action.cpu().numpy()
        assert (run.ok.cpu().numpy() == 1).all()
        active += int((np.abs(w) >= RB.U_MAX).any(1).sum())
        assert (np.abs(got) <= RB.U_MAX).all() and (np.abs(a) <= RB.U_MAX).all()
        np.testing.assert_array_equal(a, got.astype(np.float32))
        assert (np.linalg.norm(run.plan.cpu().numpy().reshape(H * 5, n).T - w, axis=1) <= bound).all()
        assert (np.abs(got - u0).max(1) <= bound).all()
    print(f"tracking: env-frames with an active bound {active}/{6 * n}, max iters {int(run.iters.max())}")
    assert active > 0
