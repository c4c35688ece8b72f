"""Shared checks of the constraint solve at 7..16 contacts per env and past the cap of 16.

The contact substep keeps the rows of an env's first LDS_CON = 6 contacts in LDS; contacts 7..16 go
through the per-edge J/W rows of the global scratch slab ([row][env], soarm_pgs.h ContactRows and
scratch_rows, soarm_newton.h's overflow edges), and the 17th contact sets ST_CONOVERFLOW and is
dropped with every later one.  The bench states and the resting cube have 4 to 6 contacts, so these
checks bring their own states: tests/golden/contact_overflow_states.npz (make_golden.py
contact_overflow_states, from the float64 oracle alone).

Every check takes `make_sim(cm, n)` and `load_state(S, st)` (as
test_cpu_backend.check_acc_bad_retry_contact_scene does): tests/test_contact_overflow.py runs them
on the library's CPU backend without a GPU, and on the device for the RS kernel, the quad kernel
and the Newton model.

Classes of a many-contact env (census): the arm-table pairs precede the table-cube pair in pair
order, so the cube's 4 table contacts ("the block") sit wholly inside the first 6 list slots
(`lds`), straddle slot 6 (`straddle`) or lie wholly in the slab (`slab`); `full` is exactly 16
contacts with no overflow bit, `over` is past the cap.
"""
import functools
import os

import numpy as np

from oracle import Oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contact_overflow_states.npz")
QVEL_BARS = (2e-6, 3.5e-4, 2.5e-3)  # = test_gpu_parity.QVEL_BARS (one substep, fp32 vs the fp64 oracle)
FIELDS = ("qpos", "qvel", "qacc_warmstart", "ncon", "status", "obs")
SETS = ("shallow", "deep", "fill")
KEYS = ("qpos", "qvel", "warm", "ctrl")
LDS_CON, MAXCON = 6, 16  # soarm_pgs.h LDS_CON, soarm_sim.h SIM_MAXCON
CLASSES = ("lds", "straddle", "slab", "full", "over")
# depth bounds of test_gpu_parity.test_contacts_match_oracle: physically relevant, not grazing
DEEPEST, GRAZING = 5e-3, 2e-5


@functools.lru_cache(maxsize=None)
def model(solver="PGS"):
    from lerobot_mujoco_sim2real_amd import mjcf
    return mjcf.compile_mjcf(mjcf.CUBE_SCENE_XML, solver=solver)


def f32(st):
    return {k: (v.astype(np.float32).astype(np.float64) if v.dtype == np.float64 else v) for k, v in st.items()}


def take(st, ids):
    ids = np.asarray(ids)
    return {k: v[ids].copy() for k, v in st.items()}


def concat(*sts):
    return {k: np.concatenate([s[k] for s in sts]) for k in sts[0]}


def overflow_poses(rng, n):
    """Arm poses as test_gpu_parity._contact_poses, shoulder / elbow ranges widened so that the arm
    lies on the table with many links at once."""
    q = np.zeros((n, 6))
    q[:, 0] = rng.uniform(-1, 1, n)
    q[:, 1] = rng.uniform(0.6, 1.7, n)
    q[:, 2] = rng.uniform(-0.5, 1.6, n)
    q[:, 3] = rng.uniform(0.3, 1.6, n)
    q[:, 4] = rng.uniform(-2, 2, n)
    q[:, 5] = rng.uniform(0, 1.5, n)
    return q


def census(cm, orc, st):
    """Per env of the (fp32-rounded) states: the contact list of orc.forward (count, deepest and
    most grazing distance, the block's first slot and size), its largest constraint force, and
    status / ncon / qvel of one oracle substep from there.  `st` is left unchanged."""
    n = len(st["qpos"])
    names = cm.geom_names
    table, cube = names.index("table"), names.index("cube")
    c = np.zeros(n, int)
    deepest, graze = np.zeros(n), np.ones(n)
    first, nblk, fmax = np.full(n, -1), np.zeros(n, int), np.zeros(n)
    for e in range(n):
        fw = orc.forward(st["qpos"][e], st["qvel"][e], st["ctrl"][e], st["warm"][e])
        k = fw["contacts"]
        c[e] = len(k)
        fmax[e] = np.abs(fw["efc_force"]).max()
        if len(k):
            deepest[e], graze[e] = k[:, 0].min(), np.abs(k[:, 0]).min()
            b = [i for i in range(len(k)) if {int(k[i, 7]), int(k[i, 8])} == {table, cube}]
            nblk[e], first[e] = len(b), (b[0] if b else -1)
    a = {k: v.copy() for k, v in st.items()}
    a["status"][:] = 0
    a["ncon"][:] = 0
    orc.step(a, None, nsub=1, nthreads=8)
    return dict(ncon=c, deepest=deepest, graze=graze, first=first, nblk=nblk, fmax=fmax, status=a["status"].copy(),
                ncon_step=a["ncon"].copy(), qvel=a["qvel"].copy())


def classes(cen):
    """The class masks of a census (an env can be in `full` or `over` and in a block class)."""
    from lerobot_mujoco_sim2real_amd import abi
    c, first, blk = cen["ncon"], cen["first"], cen["nblk"] == 4
    over = (cen["status"] & abi.ST_CONOVERFLOW) != 0
    many = c > LDS_CON
    return dict(lds=many & blk & (first + 4 <= LDS_CON), straddle=many & blk & (first < LDS_CON) & (first + 4 > LDS_CON),
                slab=many & blk & (first >= LDS_CON), full=(c == MAXCON) & ~over, over=over)


@functools.lru_cache(maxsize=None)
def fixture():
    """The committed states {set: {qpos, qvel, warm, ctrl, status, ncon}}, float64 arrays of fp32
    values, row per env.  Not to be modified."""
    z = np.load(GOLDEN)
    out = {}
    for s in SETS:
        st = {k: z[f"{s}_{k}"].astype(np.float64) for k in KEYS}
        n = len(st["qpos"])
        st["status"], st["ncon"] = np.zeros(n, np.int32), np.zeros(n)
        out[s] = st
    return out


@functools.lru_cache(maxsize=None)
def fixture_census(name):
    cm = model()
    return census(cm, Oracle(cm), fixture()[name])


@functools.lru_cache(maxsize=None)
def oracle_substep(solver, name):
    """The set `name` after one substep of the float64 oracle on the `solver` model (status and ncon
    zeroed before: the oracle's status is sticky).  Not to be modified."""
    st = take(fixture()[name], np.arange(len(fixture()[name]["qpos"])))
    Oracle(model(solver)).step(st, None, nsub=1, nthreads=8)
    return st


def to_np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def snapshot(S):
    """The compared fields as int32 bit patterns (a float compare would pass -0 for +0)."""
    import torch
    if not S.cpu:
        torch.cuda.synchronize()
    return {k: getattr(S, k).detach().clone().contiguous().view(torch.int32).cpu() for k in FIELDS}


def rows(snap, idx):
    """The envs `idx` of a snapshot (the state is [field, env], ncon / status [env], obs [env, field])."""
    import torch
    idx = torch.as_tensor(np.asarray(idx))
    return {k: (v[idx] if k in ("ncon", "status", "obs") else v[:, idx]) for k, v in snap.items()}


def assert_same_bits(a, b, what=""):
    import torch
    for k in FIELDS:
        assert torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def assert_pct(err, p50, p99, mx, what=""):
    e = np.asarray(err, np.float64).ravel()
    got = (float(np.median(e)), float(np.percentile(e, 99)), float(e.max()))
    assert got[0] <= p50 and got[1] <= p99 and got[2] <= mx, (what, "p50/p99/max", got, "bars", (p50, p99, mx))


def start(make_sim, load_state, cm, st):
    """A fresh batch at the states `st`, ncon and status zeroed."""
    S = make_sim(cm, len(st["qpos"]))
    load_state(S, st)
    S.status.zero_()
    S.ncon.zero_()
    return S


def substep(make_sim, load_state, cm, st):
    """A fresh batch at `st` after one substep (and the observation of the new state)."""
    S = start(make_sim, load_state, cm, st)
    S.substeps(1)
    S.observe()
    return S, snapshot(S)


def qvel_gap(S, ref):
    return np.abs(to_np(S.qvel).T - ref["qvel"]).max(1)


def stats(dv):
    return "p50 %.2e p99 %.2e max %.2e over %.1e: %d of %d" % (
        np.median(dv), np.percentile(dv, 99), dv.max(), QVEL_BARS[2], int((dv > QVEL_BARS[2]).sum()), len(dv))


# ---------------------------------------------------------------------------------------- a. shallow
def check_shallow_parity(make_sim, load_state, solver):
    """One substep from the settled many-contact states (every contact between 20 um and 5 mm deep):
    the project's one-substep bars of the float64 oracle hold as they do at 4..6 contacts."""
    cm, st = model(solver), fixture()["shallow"]
    ref = oracle_substep(solver, "shallow")
    S, _ = substep(make_sim, load_state, cm, st)
    dv = qvel_gap(S, ref)
    print(f"shallow {solver}: ncon {np.bincount(ref['ncon'].astype(int))}, qpos gap max "
          f"{np.abs(to_np(S.qpos).T - ref['qpos']).max():.2e}, qvel gap {stats(dv)}")
    assert (ref["ncon"] > LDS_CON).all() and (ref["status"] == 0).all()  # (the input is what it claims)
    np.testing.assert_allclose(to_np(S.qpos).T, ref["qpos"], atol=5e-6)
    assert_pct(dv, *QVEL_BARS, what="qvel")
    assert (to_np(S.ncon) == ref["ncon"]).all(), (to_np(S.ncon), ref["ncon"])
    assert (to_np(S.status) == 0).all(), to_np(S.status)


# ------------------------------------------------------------------------------------------- b. deep
def check_deep_parity(make_sim, load_state, solver):
    """One substep from the deep set: ncon and the status bits per env equal the oracle's
    (ST_CONOVERFLOW exactly on the past-the-cap envs, where ncon is 16), and qvel against the oracle
    within bars taken from the CPU backend's gap on the same states -- an independent fp32 solve in
    MuJoCo's row order: p50 and p99 within max(the project's bar, 3 x the CPU backend's; for the
    Newton model the worse of the CPU backend's PGS and Newton solves), at most
    2 % of the envs over QVEL_BARS[2], and each of those over QVEL_BARS[2] / 10 on the CPU backend
    too (ill-conditioned in fp32 generally, not on this solver alone).  The oracle drops the 17th and
    later contacts in pair order, so the qvel parity of the `over` envs is the check that the same 16
    are kept.  Returns (device gaps, CPU-backend gaps) per env."""
    from lerobot_mujoco_sim2real_amd import abi
    from lerobot_mujoco_sim2real_amd.sim import BatchSim
    cm, st = model(solver), fixture()["deep"]
    ref = oracle_substep(solver, "deep")
    cls = classes(fixture_census("deep"))
    S, _ = substep(make_sim, load_state, cm, st)
    H = start(lambda m, n: BatchSim(m, n, -1), load_state_host, cm, st)
    H.substeps(1)
    dv, hv = qvel_gap(S, ref), qvel_gap(H, ref)
    print(f"deep {solver}: all      device {stats(dv)} | cpu backend {stats(hv)}")
    for k in CLASSES:
        print(f"deep {solver}: {k:8s} device {stats(dv[cls[k]])} | cpu backend {stats(hv[cls[k]])}")
    stat, ncon = to_np(S.status).astype(int), to_np(S.ncon)
    assert (ncon == ref["ncon"]).all(), np.flatnonzero(ncon != ref["ncon"])
    assert (stat == ref["status"]).all(), np.flatnonzero(stat != ref["status"])
    assert ((stat & abi.ST_CONOVERFLOW) != 0)[cls["over"]].all() and (stat[cls["full"]] == 0).all()
    assert (stat & ~abi.ST_CONOVERFLOW == 0).all() and (stat[~cls["over"]] == 0).all(), stat
    assert (ncon[cls["over"]] == MAXCON).all() and (ncon[cls["full"]] == MAXCON).all()
    assert np.isfinite(dv).all() and np.isfinite(hv).all()
    p50, p99 = max(QVEL_BARS[0], 3 * np.median(hv)), max(QVEL_BARS[1], 3 * np.percentile(hv, 99))
    if solver != "PGS":
        # The Newton model's yardstick is the worse of the CPU backend's two solves (each against the
        # oracle on its own solver): both solve the same convex problem, and the device's largest gaps
        # are the same envs on all three kernels (upstream of the solve), so how far fp32 generally
        # lands from the oracle on these states is what either CPU solve shows.  (The CPU backend's
        # Newton used to stop early, 1.05e-3 at p99 here, which set this bar at 3.15e-3; since the fix
        # of its stopping test it is at 2.35e-4, and 3 x that alone is under what the same device
        # geometry gives on every kernel.)
        P = start(lambda m, n: BatchSim(m, n, -1), load_state_host, model("PGS"), st)
        P.substeps(1)
        pv = qvel_gap(P, oracle_substep("PGS", "deep"))
        print(f"deep {solver}: all      cpu backend PGS {stats(pv)}")
        p50, p99 = max(p50, 3 * np.median(pv)), max(p99, 3 * np.percentile(pv, 99))
    assert np.median(dv) <= p50 and np.percentile(dv, 99) <= p99, (np.median(dv), np.percentile(dv, 99), p50, p99)
    tail = dv > QVEL_BARS[2]
    assert tail.sum() <= 0.02 * len(dv), (np.flatnonzero(tail), dv[tail])
    assert (hv[tail] > QVEL_BARS[2] / 10).all(), (np.flatnonzero(tail), dv[tail], hv[tail])
    return dv, hv


def load_state_host(S, st):
    import torch
    S.qpos.copy_(torch.as_tensor(st["qpos"].T, dtype=torch.float32))
    S.qvel.copy_(torch.as_tensor(st["qvel"].T, dtype=torch.float32))
    S.qacc_warmstart.copy_(torch.as_tensor(st["warm"].T, dtype=torch.float32))
    S.ctrl.copy_(torch.as_tensor(st["ctrl"].T, dtype=torch.float32))


# ------------------------------------------------------------------------------ c. batch composition
def composition_targets():
    """(past-the-cap, straddling, in-slab) env ids of the deep set: the first of each class."""
    cls = classes(fixture_census("deep"))
    over = int(np.flatnonzero(cls["over"])[0])
    strad = int(np.flatnonzero(cls["straddle"] & ~cls["over"])[0])
    slab = int(np.flatnonzero(cls["slab"] & ~cls["over"])[0])
    return over, strad, slab


def check_batch_composition(make_sim, load_state, solver):
    """A past-the-cap env, a straddling env and an in-slab env give the same bits whatever batch
    they sit in: alone, first and last of 5, last of 68 (the slab's [row][env] stride is the batch
    size), in a wave of resting-cube and lifted-cube envs, and among many-contact envs only.  Their
    waves never take the row-space solve (more than LDS_CON contacts), so the RS kernel's wave-wide
    vote comes out the same in every layout for them; the fill envs' own bits are not compared."""
    cm, fx = model(solver), fixture()
    deep, fill = fx["deep"], fx["fill"]
    nd, nf = len(deep["qpos"]), len(fill["qpos"])
    for t in composition_targets():
        x = take(deep, [t])
        _, alone = substep(make_sim, load_state, cm, x)
        one = rows(alone, [0])
        others = [i for i in range(nd) if i != t]
        # first and last of 5, among many-contact envs
        _, s5 = substep(make_sim, load_state, cm, concat(x, take(deep, others[:3]), x))
        assert_same_bits(rows(s5, [0]), one, what=(t, "env 0 of 5"))
        assert_same_bits(rows(s5, [4]), one, what=(t, "env 4 of 5"))
        # last of 68, many-contact envs only
        _, s68 = substep(make_sim, load_state, cm, concat(take(deep, others[:67]), x))
        assert_same_bits(rows(s68, [67]), one, what=(t, "env 67 of 68, many-contact envs"))
        # among resting-cube (fill 0..15) and lifted-cube (fill 16..23) envs: at every position of an
        # RS wave (4 envs) and in the middle of a quad wave (16 envs)
        pad = take(fill, [(7 * i) % nf for i in range(19)])
        mix = concat(take(pad, np.arange(0, 5)), x, take(pad, np.arange(5, 10)), x, take(pad, np.arange(10, 14)), x,
                     take(pad, np.arange(14, 19)), x)
        at = [5, 11, 16, 22]  # lanes 1, 3, 0, 2 of their RS waves
        S, sm = substep(make_sim, load_state, cm, mix)
        for k in at:
            assert_same_bits(rows(sm, [k]), one, what=(t, "env %d among fill envs" % k))
        nc = to_np(S.ncon)
        keep = np.ones(len(nc), bool)
        keep[at] = False
        assert set(nc[keep]) == {0.0, 4.0}, nc  # (the fill envs are what they claim)


# --------------------------------------------------------------------------------------- d. stale slab
def check_stale_slab(make_sim, load_state, solver):
    """The slab is not cleared between substeps: a batch that stepped 12+-contact states and then has
    8-contact states loaded into the same env slots must give what a fresh batch gives from them."""
    cm, deep = model(solver), fixture()["deep"]
    cen = fixture_census("deep")
    big = np.flatnonzero(cen["ncon"] >= 12)[:6]
    small = np.flatnonzero(cen["ncon"] == 8)[:6]
    assert len(big) == 6 and len(small) == 6
    S = start(make_sim, load_state, cm, take(deep, big))
    S.substeps(1)
    assert (to_np(S.ncon) >= 12).all()
    load_state(S, take(deep, small))
    S.status.zero_()
    S.ncon.zero_()
    S.obs.zero_()
    S.substeps(1)
    S.observe()
    assert (to_np(S.ncon) == 8).all()
    _, fresh = substep(make_sim, load_state, cm, take(deep, small))
    assert_same_bits(snapshot(S), fresh, what="8-contact states after 12+-contact states in the same slots")


def check_env_step_repeats(make_sim, load_state, solver):
    """One full env-step (10 substeps, zero action) from the deep set, twice: bit-identical, finite,
    and no status bit beyond the overflow bit."""
    import torch
    from lerobot_mujoco_sim2real_amd import abi
    cm, deep = model(solver), fixture()["deep"]
    snaps = []
    for _ in range(2):
        S = start(make_sim, load_state, cm, deep)
        S.step(torch.zeros((S.n, S.nact), dtype=torch.float32, device=S.device))
        snaps.append(snapshot(S))
        for k in ("qpos", "qvel", "qacc_warmstart", "obs"):
            assert bool(torch.isfinite(getattr(S, k)).all()), k
        assert (to_np(S.status).astype(int) & ~abi.ST_CONOVERFLOW == 0).all(), to_np(S.status)
    assert_same_bits(snaps[0], snaps[1], what="two env-steps from the same states")
