"""Shared checks of the contact-force readout (sim_contact_forces: mj_forward at the current state +
mj_contactForce of every contact; BatchSim.contact_forces / net_contact_force).

Every check takes `make_sim(cm, n)` and `load_state(S, st)` as the checks of contact_overflow_ref.py
do: tests/test_contact_forces.py runs them on the library's CPU backend without a GPU and, marked
`gpu`, on the device for the PGS and the Newton model.

Reference: the float64 oracle's efc_force of the same (fp32-rounded) state on the model compiled with
the same solver (Oracle.forward), its last 4 x ncon rows decoded here as mju_decodePyramid does for
condim 3.  Error of an env: the largest component error of its contacts' decoded forces (normal,
tangent 1, tangent 2), divided by the env's largest oracle normal force (floor: the cube's weight).
The oracle has no world vector of its own: the readout's is held to what the readout answers for,
force[3:6] = the library's own contact frame (mju_makeFrame of the normal it returns) applied to
force[0:3], to fp32 rounding (world_vector_gap); its direction against the oracle is the collide's
normal, which the contact tests bound, and the second-law check holds it to the cube's motion.
Yardstick: the oracle's own fp32-noise envelope -- the oracle run again with qpos, qvel and the warm
start moved by +-8 fp32 ulps (as conftest.fp32_noise_envelope does), the largest change of an edge force per env over the same divisor; the bar is 10 x that envelope at
p50 / p99 / max per set and solver (DESIGN §2's convention for fp32 against the fp64 oracle).
"""
import functools

import numpy as np

import contact_overflow_ref as R
from oracle import Oracle

WEIGHT = 0.2943  # N: the 0.03 kg cube under 9.81 m/s^2
MAXCON = R.MAXCON
H = 0.002        # the model's timestep


def to_np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def arm_model(solver="PGS"):
    from lerobot_mujoco_sim2real_amd import mjcf
    return mjcf.compile_mjcf(mjcf.SCENE_XML, solver=solver)


def pair_table(cm):
    d = cm.desc
    return {(d.pair_geom1[p], d.pair_geom2[p]): p for p in range(d.npair)}


def pair_mu(cm):
    """Sliding friction per pair: the larger of the two geoms' (MuJoCo's contact parameter mixing)."""
    d = cm.desc
    return np.array([max(d.geom_friction[d.pair_geom1[p]][0], d.geom_friction[d.pair_geom2[p]][0])
                     for p in range(d.npair)])


def make_frame(n):
    """mju_makeFrame of a unit normal: rows normal, tangent 1, tangent 2."""
    n = np.asarray(n, np.float64)
    y = np.array([0.0, 1.0, 0.0]) if abs(n[1]) < 0.5 else np.array([0.0, 0.0, 1.0])
    y = y - n * (n @ y)
    y /= np.linalg.norm(y)
    return np.stack([n, y, np.cross(n, y)])


def decode(edge, mu):
    """mju_decodePyramid, condim 3: edge [k, 4] -> (normal, tangent 1, tangent 2) [k, 3]."""
    edge = np.asarray(edge, np.float64).reshape(-1, 4)
    mu = np.broadcast_to(np.asarray(mu, np.float64), (len(edge),))
    return np.stack([edge.sum(1), mu * (edge[:, 0] - edge[:, 1]), mu * (edge[:, 2] - edge[:, 3])], 1)


def oracle_forward(orc, cm, st, e):
    """(pair ids [k], contact records [k, 9], edge forces [k, 4]) of env e of `st`."""
    fw = orc.forward(st["qpos"][e], st["qvel"][e], st["ctrl"][e], st["warm"][e])
    k = fw["contacts"]
    tab = pair_table(cm)
    pairs = np.array([tab[(int(c[7]), int(c[8]))] for c in k], int)
    edge = fw["efc_force"][len(fw["efc_force"]) - 4 * len(k):].reshape(-1, 4)
    return pairs, k, edge


def oracle_forces(cm, st):
    """Per env of the states `st` (fp32 values): dict(pair [k], con [k, 9], edge [k, 4], force [k, 6],
    fmax = the divisor).  The oracle is the one of `cm` (its solver)."""
    orc, mu = Oracle(cm), pair_mu(cm)
    out = []
    for e in range(len(st["qpos"])):
        pairs, k, edge = oracle_forward(orc, cm, st, e)
        loc = decode(edge, mu[pairs] if len(pairs) else 0.0)
        world = np.array([loc[i] @ make_frame(k[i, 4:7]) for i in range(len(k))]).reshape(-1, 3)
        fmax = max(WEIGHT, float(loc[:, 0].max()) if len(k) else 0.0)
        out.append(dict(pair=pairs, con=k, edge=edge, force=np.concatenate([loc, world], 1), fmax=fmax))
    return out


def oracle_envelope(cm, st, ref, kulp=8, trials=2, seed=0):
    """Per env: the largest change of an edge force when qpos, qvel and the warm start move by a
    random +-kulp fp32 ulps per component, over the env's divisor.  The contact list must not change."""
    orc = Oracle(cm)
    rng = np.random.default_rng(seed)
    env = np.zeros(len(ref))
    for _ in range(trials):
        c = {k: v.copy() for k, v in st.items()}
        for k in ("qpos", "qvel", "warm"):
            x = c[k].astype(np.float32)
            u = np.spacing(np.abs(x)).astype(np.float64)
            c[k] = x.astype(np.float64) + rng.integers(-kulp, kulp + 1, x.shape) * u
        for e in range(len(ref)):
            pairs, _, edge = oracle_forward(orc, cm, c, e)
            assert np.array_equal(pairs, ref[e]["pair"]), ("contact list moved under fp32 noise", e)
            if len(pairs):
                env[e] = max(env[e], np.abs(edge - ref[e]["edge"]).max() / ref[e]["fmax"])
    return env


def pct(x):
    x = np.asarray(x, np.float64)
    return np.array([np.median(x), np.percentile(x, 99), x.max()])


@functools.lru_cache(maxsize=None)
def golden_reference(solver, name):
    """(oracle forces per env, the bars 10 x envelope at p50 / p99 / max) of a golden set.  Shared, not
    to be modified."""
    cm, st = R.model(solver), R.fixture()[name]
    ref = oracle_forces(cm, st)
    env = oracle_envelope(cm, st, ref)
    return ref, 10.0 * pct(env), pct(env)


def readout(S):
    """(contacts, force, ncon) as numpy, and the pair ids [n, 16] (int32 bits of field 7)."""
    con, frc, nc = S.contact_forces()
    con, frc, nc = to_np(con), to_np(frc), to_np(nc)
    return con, frc, nc, np.ascontiguousarray(con[:, :, 7]).view(np.int32)


def world_vector_gap(con, frc):
    """Per contact: |force[3:6] - frame(returned normal)' force[0:3]| at its largest component, and
    the bound: the frame's rows come from an fp32 normalisation (a few ulps per entry) and the vector
    from three fp32 products and two sums, so 16 fp32 ulps of |f_n| + |f_t1| + |f_t2| cover it."""
    loc = frc[:, :3].astype(np.float64)
    want = np.array([loc[i] @ make_frame(con[i, 4:7]) for i in range(len(con))]).reshape(-1, 3)
    return np.abs(frc[:, 3:6].astype(np.float64) - want).max(1), 16 * 2.0 ** -24 * np.abs(loc).sum(1)


def force_errors(con, frc, nc, pair, ref):
    """Per env error against the oracle's decoded forces; ncon and the pair ids must match exactly
    (past the cap: the kept 16), and every world vector its own frame applied to the decoded force."""
    err = np.zeros(len(ref))
    for e, r in enumerate(ref):
        k = len(r["pair"])
        assert nc[e] == k, ("ncon", e, int(nc[e]), k)
        assert np.array_equal(pair[e, :k], r["pair"]), ("pair ids", e, pair[e, :k], r["pair"])
        assert not frc[e, k:].any() and not con[e, k:].any(), ("slots >= ncon are zero", e)
        if k:
            gap = np.abs(frc[e, :k, :3].astype(np.float64) - r["force"][:, :3]).max(1)
            wg, wtol = world_vector_gap(con[e, :k], frc[e, :k])
            assert (wg <= wtol).all(), ("world vector != own frame x decoded force", e, wg, wtol)
            err[e] = gap.max() / r["fmax"]
    return err


def assert_bars(err, bars, what):
    got = pct(err)
    print(what, "error p50/p99/max %.2e %.2e %.2e" % tuple(got), "bars %.2e %.2e %.2e" % tuple(bars))
    assert (got <= bars).all(), (what, "p50/p99/max", tuple(got), "bars", tuple(bars))


# ------------------------------------------------------------------------------------------ 1. parity
def check_parity(make_sim, load_state, solver, name):
    cm, st = R.model(solver), R.fixture()[name]
    ref, bars, env = golden_reference(solver, name)
    nk = np.array([len(r["pair"]) for r in ref])
    fn = np.array([r["force"][:, 0].max() for r in ref])
    print(f"{name} {solver}: {len(ref)} envs, contacts {nk.min()}..{nk.max()}, largest normal force median "
          f"{np.median(fn):.1f} N max {fn.max():.1f} N; envelope p50/p99/max %.2e %.2e %.2e" % tuple(env))
    S = R.start(make_sim, load_state, cm, st)
    err = force_errors(*readout(S), ref)
    assert_bars(err, bars, f"{name} {solver}")
    return err


# ------------------------------------------------------------------------------------ 2. resting cube
@functools.lru_cache(maxsize=None)
def resting_state(solver):
    """The pick scene after 30 oracle env-steps at zero action (fp32-rounded).  Not to be modified."""
    cm = R.model(solver)
    orc = Oracle(cm)
    st = orc.new_state(1)
    orc.reset(st)
    for _ in range(30):
        orc.step(st, np.zeros((1, cm.desc.nact)))
    st = R.f32(st)
    st["status"][:] = 0
    st["ncon"][:] = 0
    return st


def check_resting_cube(make_sim, load_state, solver):
    cm, st = R.model(solver), resting_state(solver)
    ref = oracle_forces(cm, st)
    bar = 10.0 * oracle_envelope(cm, st, ref).max()
    r = ref[0]
    assert len(r["pair"]) == 4 and np.allclose(r["con"][:, 4:7], [0, 0, 1], atol=1e-9)
    osum = r["force"][:, 0].sum()
    print(f"resting {solver}: oracle normals {r['force'][:, 0]}, sum {osum:.6f} N, bar {bar:.2e}")
    assert abs(osum - WEIGHT) < 2e-5  # (the input is what it claims: the cube rests, m g = 0.2943 N)
    if solver == "Newton":
        np.testing.assert_allclose(r["force"][:, 0], 0.073575, atol=2e-6)
    S = R.start(make_sim, load_state, cm, st)
    con, frc, nc, pair = readout(S)
    err = force_errors(con, frc, nc, pair, ref)
    f = frc[0, :4].astype(np.float64)
    mu = pair_mu(cm)[pair[0, :4]]
    print(f"resting {solver}: library normals {f[:, 0]}, sum {f[:, 0].sum():.6f} N, error {err[0]:.2e}")
    assert (f[:, 0] >= 0).all()
    assert (np.abs(f[:, 1:3]) <= mu[:, None] * f[:, 0:1] + 1e-9).all()  # inside the pyramid
    np.testing.assert_allclose(con[0, :4, 4:7], np.tile([0, 0, 1], (4, 1)), atol=1e-6)
    # m g within the parity bar (on top of how far the oracle's own sum is from m g on this state)
    assert abs(f[:, 0].sum() - WEIGHT) <= bar * WEIGHT + abs(osum - WEIGHT), (f[:, 0].sum(), WEIGHT, bar)
    assert err[0] <= bar, (err[0], bar)
    # the cube's net contact force is its weight, upwards; the table's (world body) its negative
    net = to_np(S.net_contact_force("cube"))[0].astype(np.float64)
    assert abs(net[2] - f[:, 0].sum()) <= 1e-6 * WEIGHT and np.abs(net[:2]).max() <= 2 * mu.max() * WEIGHT
    np.testing.assert_array_equal(to_np(S.net_contact_force(0)), -to_np(S.net_contact_force(cm.body("cube"))))


# --------------------------------------------------------------------------------- 3. Newton's second law
def check_second_law(make_sim, load_state, solver, randomised, bar):
    """m_eff (dv_lin / h - g) = net contact force on the cube + qfrc_applied[cube linear], dv from one
    substep of a twin batch started at the same state (the free joint's linear dofs are world-frame
    and undamped).  bar: the parity bar (relative to the env's largest normal force)."""
    import torch
    cm, st = R.model(solver), R.fixture()["deep"]
    n = len(st["qpos"])
    rng = np.random.default_rng(3)
    ms = rng.uniform(0.7, 1.4, n).astype(np.float32) if randomised else np.ones(n, np.float32)
    fr = rng.uniform(0.5, 1.3, n).astype(np.float32) if randomised else None
    push = np.zeros((n, cm.desc.nv), np.float32)
    if randomised:
        push[:, 8] = -rng.uniform(0.1, 2.0, n)  # N, downwards on the cube
    A, B = (R.start(make_sim, load_state, cm, st) for _ in range(2))
    for S in (A, B):
        if randomised:
            S.set_params(mass_scale=ms, friction=fr)
            S.enable_qfrc_applied().copy_(torch.as_tensor(push.T, device=S.device))
    con, frc, nc, pair = readout(A)
    net = to_np(A.net_contact_force("cube")).astype(np.float64)
    v0 = to_np(B.qvel).T[:, 6:9].astype(np.float64)
    B.substeps(1)
    v1 = to_np(B.qvel).T[:, 6:9].astype(np.float64)
    assert (to_np(B.status) & ~8 == 0).all()
    m = 0.03 * ms.astype(np.float64)
    g = np.array([0.0, 0.0, -9.81])
    lhs = m[:, None] * ((v1 - v0) / H - g)
    rhs = net + push[:, 6:9].astype(np.float64)
    fmax = np.maximum(WEIGHT, frc[:, :, 0].max(1).astype(np.float64))
    vmax = np.maximum(np.abs(v0), np.abs(v1)).max(1).astype(np.float32)
    tol = np.maximum(m * 4 * np.spacing(vmax).astype(np.float64) / H, bar * fmax)
    gap = np.abs(lhs - rhs).max(1)
    print(f"second law {solver} randomised={randomised}: gap / tolerance max {(gap / tol).max():.3f}, "
          f"gap max {gap.max():.2e} N, relative to the largest normal force max {(gap / fmax).max():.2e}")
    assert (gap <= tol).all(), (np.flatnonzero(gap > tol), gap[gap > tol], tol[gap > tol])


# ------------------------------------------------------------------------------------------ 4. shapes
def bits(S):
    """One readout as int32 bit patterns (contacts, force, ncon)."""
    import torch
    con, frc, nc = S.contact_forces()
    return [t.detach().contiguous().view(torch.int32).cpu().clone() for t in (con, frc, nc)]


def env_bits(b, i):
    return [t[i] for t in b]


def assert_same(a, b, what):
    import torch
    for x, y, k in zip(a, b, ("contacts", "force", "ncon")):
        assert torch.equal(x, y), (what, k)


def check_placements(make_sim, load_state, solver):
    """The same env gives the same bits alone (n = 1), first and last of 3 and of 5, last of 17 and of 68,
    and at every position of a lane group among resting-cube and lifted-cube envs."""
    cm, fx = R.model(solver), R.fixture()
    deep, fill = fx["deep"], fx["fill"]
    cen = R.fixture_census("deep")
    nd, nf = len(deep["qpos"]), len(fill["qpos"])
    targets = [int(np.flatnonzero(cen["ncon"] == 16)[0]), int(np.flatnonzero(cen["ncon"] == 9)[0])]
    for t in targets:
        x = R.take(deep, [t])
        others = [i for i in range(nd) if i != t]
        one = env_bits(bits(R.start(make_sim, load_state, cm, x)), 0)
        assert int(one[2]) == cen["ncon"][t]
        for k in (1, 3):  # n = 3 and n = 5: first and last
            b = bits(R.start(make_sim, load_state, cm, R.concat(x, R.take(deep, others[:k]), x)))
            assert_same(env_bits(b, 0), one, (t, "first of", k + 2))
            assert_same(env_bits(b, k + 1), one, (t, "last of", k + 2))
        for k in (16, 67):  # n = 17 and n = 68: last, many-contact envs before it
            b = bits(R.start(make_sim, load_state, cm, R.concat(R.take(deep, others[:k]), x)))
            assert_same(env_bits(b, k), one, (t, "last of", k + 1))
        pad = R.take(fill, [(7 * i) % nf for i in range(19)])
        mix = R.concat(R.take(pad, np.arange(0, 5)), x, R.take(pad, np.arange(5, 10)), x,
                       R.take(pad, np.arange(10, 14)), x, R.take(pad, np.arange(14, 19)), x)
        at = [5, 11, 16, 22]  # positions 1, 3, 0, 2 of their groups of 4 envs
        S = R.start(make_sim, load_state, cm, mix)
        b = bits(S)
        for k in at:
            assert_same(env_bits(b, k), one, (t, "among fill envs at", k))
        nc = b[2].numpy()
        keep = np.ones(len(nc), bool)
        keep[at] = False
        assert set(nc[keep]) == {0, 4}, nc  # (the fill envs are what they claim)
        assert_same(bits(S), b, (t, "a repeated call"))


def check_no_contacts(make_sim, load_state, solver):
    """Cube lifted, arm clear: ncon 0, every output zero."""
    cm, fill = R.model(solver), R.fixture()["fill"]
    S = R.start(make_sim, load_state, cm, R.take(fill, np.arange(16, 24)))
    con, frc, nc, _ = readout(S)
    assert not nc.any() and not con.any() and not frc.any()
    assert not to_np(S.net_contact_force("cube")).any()


@functools.lru_cache(maxsize=None)
def arm_states(solver, want=8):
    """Arm-only scene (no free body), the arm laid on the table: the first `want` of 64 drawn poses
    in which the oracle finds contacts, at rest, the position servo holding the pose."""
    cm = arm_model(solver)
    orc = Oracle(cm)
    q = R.overflow_poses(np.random.default_rng(11), 64)
    st = orc.new_state(64)
    st["qpos"][:] = q[:, :cm.desc.nq]
    st["ctrl"][:] = q[:, :cm.desc.nu]
    st = R.f32(st)
    keep = [e for e in range(64) if orc.forward(st["qpos"][e], st["qvel"][e], st["ctrl"][e], st["warm"][e])["ncon"] > 0]
    assert len(keep) >= want
    return R.take(st, keep[:want])


def check_arm_scene(make_sim, load_state, solver):
    cm, st = arm_model(solver), arm_states(solver)
    ref = oracle_forces(cm, st)
    bars = 10.0 * pct(oracle_envelope(cm, st, ref))
    S = R.start(make_sim, load_state, cm, st)
    err = force_errors(*readout(S), ref)
    print(f"arm scene {solver}: contacts {[len(r['pair']) for r in ref]}")
    assert_bars(err, bars, f"arm scene {solver}")


# ------------------------------------------------------------------------------------- 5. pure readout
def check_pure_readout(make_sim, load_state, solver, warmup_substeps):
    """The readout changes no bit of the state, and 3 env-steps after it equal 3 env-steps of a twin
    batch that never called it."""
    import torch
    cm, st = R.model(solver), R.fixture()["deep"]
    A, B = (R.start(make_sim, load_state, cm, st) for _ in range(2))
    for S in (A, B):
        if warmup_substeps:
            S.substeps(warmup_substeps)  # (Newton: the zone history of the last two substeps is filled)
        S.observe()
    before = R.snapshot(A)
    con, frc, nc = A.contact_forces()
    assert int(nc.max()) > 0
    A.contact_forces()
    R.assert_same_bits(R.snapshot(A), before, what="state before / after the readout")
    R.assert_same_bits(before, R.snapshot(B), what="twin batches before stepping")
    act = torch.zeros((A.n, A.nact), dtype=torch.float32, device=A.device)
    for k in range(3):
        A.step(act)
        B.step(act)
        if k == 0:
            A.contact_forces()  # (between env-steps too: the captured graph replays on the same buffers)
    R.assert_same_bits(R.snapshot(A), R.snapshot(B), what="3 env-steps after a readout / without one")


# ------------------------------------------------------------------------------------------- 6. errors
def check_errors(make_sim, load_state):
    import ctypes as C

    import torch
    from lerobot_mujoco_sim2real_amd import abi, mjcf
    cm = R.model("PGS")
    S = R.start(make_sim, load_state, cm, R.take(R.fixture()["fill"], [0, 16, 1]))
    con, frc, nc = S.contact_forces()
    assert con.shape == (3, 16, 8) and frc.shape == (3, 16, 6) and nc.shape == (3,)
    assert con.dtype == torch.float32 and frc.dtype == torch.float32 and nc.dtype == torch.int32
    assert con.device == S.qpos.device and frc.device == S.qpos.device
    net = S.net_contact_force("cube")
    assert net.shape == (3, 3) and net.dtype == torch.float32
    assert to_np(nc).tolist() == [4, 0, 4]
    with pytest_raises(ValueError):
        S.net_contact_force("no such body")
    with pytest_raises(ValueError):
        S.net_contact_force(99)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda c, f, k: S.lib.sim_contact_forces(S._batch, C.byref(S._state), c, f, k, S._stream())
    assert call(None, p(frc), p(nc)) == 0  # contacts may be null
    assert call(p(con), None, p(nc)) == abi.E_ARG
    assert call(p(con), p(frc), None) == abi.E_ARG
    assert S.lib.sim_contact_forces(None, C.byref(S._state), p(con), p(frc), p(nc), None) == abi.E_ARG
    D = make_sim(mjcf.compile_mjcf(mjcf.CUBE_SCENE_XML, disable_contact=True), 2)
    con, frc, nc = (torch.zeros(s, dtype=t, device=D.device) for s, t in
                    (((2, 16, 8), torch.float32), ((2, 16, 6), torch.float32), ((2,), torch.int32)))
    assert D.lib.sim_contact_forces(D._batch, C.byref(D._state), p(con), p(frc), p(nc), D._stream()) == abi.E_ARG
    assert b"contacts disabled" in D.lib.sim_last_error()


def pytest_raises(exc):
    import pytest
    return pytest.raises(exc)
