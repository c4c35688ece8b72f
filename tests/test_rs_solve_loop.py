"""The RS kernel's sweep loop (soarm_rs.h rs_solve): envs of one wave that stop at different sweeps,
and the sweep cap.

An env's lanes leave the loop at the sweep whose improvement passes the stop test while the wave goes
on for its other envs, and the count of sweeps is kept once per wave.  What must hold: an env's result
does not depend on the envs it shares a wave with (bit for bit), no sweep past the cap is run, and
the step stays within the one-substep bars of the float64 oracle.  The loop exists on the device only
(DPP inline assembly), so there is no CPU-backend test of it.
"""
import functools

import numpy as np
import pytest

from conftest import cube_qpos
from oracle import Oracle

pytestmark = pytest.mark.gpu

FIELDS = ("qpos", "qvel", "qacc_warmstart", "ncon", "status", "obs")
QVEL_BARS = (2e-6, 3.5e-4, 2.5e-3)  # = test_gpu_parity.QVEL_BARS (one substep, fp32 device vs fp64 oracle)


def make_sim(cm, n):
    from lerobot_mujoco_sim2real_amd.sim import BatchSim
    return BatchSim(cm, n)


def to_np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def load_state(S, st):
    import torch
    dev = S.device
    S.qpos.copy_(torch.as_tensor(st["qpos"].T, dtype=torch.float32, device=dev))
    S.qvel.copy_(torch.as_tensor(st["qvel"].T, dtype=torch.float32, device=dev))
    S.qacc_warmstart.copy_(torch.as_tensor(st["warm"].T, dtype=torch.float32, device=dev))
    S.ctrl.copy_(torch.as_tensor(st["ctrl"].T, dtype=torch.float32, device=dev))
    S.status.zero_()
    S.ncon.zero_()


def f32(st):
    """Round an oracle state to float32 so every run starts from the same bits."""
    return {k: (v.astype(np.float32).astype(np.float64) if v.dtype == np.float64 else v) for k, v in st.items()}


def take(st, ids):
    return {k: v[ids].copy() for k, v in st.items()}


def snapshot(S):
    """The compared fields as int32 bit patterns (a float compare would pass -0 for +0)."""
    import torch
    torch.cuda.synchronize()
    return {k: getattr(S, k).detach().clone().contiguous().view(torch.int32).cpu() for k in FIELDS}


def assert_same_bits(a, b, what=""):
    import torch
    for k in FIELDS:
        assert torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def run(cm, st, substeps=0, actions=()):
    """A fresh batch at `st`: `substeps` substeps, or one env-step per action."""
    import torch
    S = make_sim(cm, len(st["qpos"]))
    load_state(S, st)
    if substeps:
        S.substeps(substeps)
    for a in actions:
        S.step(torch.as_tensor(a, dtype=torch.float32, device=S.device))
    return S, snapshot(S)


def assert_pct(err, p50, p99, mx, what=""):
    e = np.asarray(err, np.float64).ravel()
    got = (float(np.median(e)), float(np.percentile(e, 99)), float(e.max()))
    assert got[0] <= p50 and got[1] <= p99 and got[2] <= mx, (what, "p50/p99/max", got, "bars", (p50, p99, mx))


@functools.lru_cache(maxsize=None)
def _cube_model(iterations=100):
    from lerobot_mujoco_sim2real_amd import mjcf
    return mjcf.compile_mjcf(mjcf.CUBE_SCENE_XML, iterations=iterations)


@functools.lru_cache(maxsize=None)
def _mixed_states(n=68):
    """Pick-scene states whose envs stop at different sweeps inside one wave (4 envs): even envs
    have the cube resting on the table (4 contacts, 16 pyramid edges: the solve runs to ~95+ sweeps),
    odd envs have it lifted 5 cm clear (frictionloss rows only: a few sweeps).  Not to be modified."""
    cm = _cube_model()
    orc = Oracle(cm)
    rng = np.random.default_rng(11)
    st = orc.new_state(n)
    orc.reset(st, init_qpos=rng.uniform(-0.3, 0.3, (n, 5)), extra_qpos=cube_qpos(cm, n, rng))
    for _ in range(5):  # settle the cubes onto the table
        orc.step(st, rng.uniform(-0.5, 0.5, (n, 5)))
    st["qpos"][1::2, 8] += 0.05
    st["ncon"][:] = 0
    acts = rng.uniform(-0.5, 0.5, (3, n, 5)).astype(np.float32)
    return f32(st), acts


def rows(snap, idx):
    """The envs `idx` of a snapshot (the state is [field, env], ncon / status [env], obs [env, field])."""
    return {k: (v[idx] if k in ("ncon", "status", "obs") else v[:, idx]) for k, v in snap.items()}


@functools.lru_cache(maxsize=None)
def _grouped_reference():
    """The 68 mixed states stepped with the resting-cube envs first and the lifted ones after them, so
    that (nearly) every wave holds envs that stop together: one substep, and 3 env-steps."""
    import torch
    full, acts = _mixed_states()
    order = np.concatenate([np.arange(0, 68, 2), np.arange(1, 68, 2)])
    inv = torch.as_tensor(np.argsort(order))
    _, sub = run(_cube_model(), take(full, order), substeps=1)
    _, stp = run(_cube_model(), take(full, order), actions=[a[order] for a in acts])
    return rows(sub, inv), rows(stp, inv)


@pytest.mark.parametrize("n", [4, 6, 68])
def test_envs_of_a_wave_stop_at_different_sweeps(gpu_lib, monkeypatch, n):
    """One wave (n = 4), a half-empty second wave (6) and 17 waves (68) of interleaved resting-cube
    and lifted-cube envs: every env must get, bit for bit, what it gets in a batch where it shares
    its wave with envs of its own kind; one substep also against the oracle."""
    import torch
    monkeypatch.setenv("SOARM_RS", "1")  # (the row-space kernel: the default, whatever the caller's environment)
    full, acts = _mixed_states()
    st = take(full, np.arange(n))
    ref_sub, ref_stp = _grouped_reference()
    S, sub = run(_cube_model(), st, substeps=1)
    assert_same_bits(sub, rows(ref_sub, torch.arange(n)), what=(n, "one substep"))
    nc = to_np(S.ncon)  # the states are what _mixed_states says: contacts on the resting cubes only
    assert (nc[0::2] > 0).all() and (nc[1::2] == 0).all(), nc
    assert int(to_np(S.status).sum()) == 0
    ref = take(st, np.arange(n))
    Oracle(_cube_model()).step(ref, None, nsub=1)
    np.testing.assert_allclose(to_np(S.qpos).T, ref["qpos"], atol=5e-6)
    dv = np.abs(to_np(S.qvel).T - ref["qvel"]).max(1)
    print(f"n {n}: qvel gap to the oracle p50 {np.median(dv):.2e} max {dv.max():.2e}")
    assert_pct(dv, *QVEL_BARS, what="qvel")
    _, stp = run(_cube_model(), st, actions=[a[:n] for a in acts])
    assert_same_bits(stp, rows(ref_stp, torch.arange(n)), what=(n, "3 env-steps"))


@pytest.mark.parametrize("iterations", [1, 2, 3, 8])
def test_sweep_cap(gpu_lib, monkeypatch, iterations):
    """Models whose sweep cap is hit (odd and even caps, and the loop's first pass): no sweep past the
    cap, none short of it -- within the one-substep bars of the oracle, which runs the same cap."""
    monkeypatch.setenv("SOARM_RS", "1")
    n = 8
    cm = _cube_model(iterations)
    st = take(_mixed_states()[0], np.arange(n))
    S, _ = run(cm, st, substeps=1)
    ref = take(st, np.arange(n))
    Oracle(cm).step(ref, None, nsub=1)
    np.testing.assert_allclose(to_np(S.qpos).T, ref["qpos"], atol=5e-6)
    dv = np.abs(to_np(S.qvel).T - ref["qvel"]).max(1)
    print(f"iterations {iterations}: qvel gap to the oracle p50 {np.median(dv):.2e} max {dv.max():.2e}")
    assert_pct(dv, *QVEL_BARS, what="qvel")
    assert to_np(S.ncon).sum() == ref["ncon"].sum()


# Envs of the contact bench workload (env ids of workloads.initial_qpos / chirp_tables, seed 0) that
# carry, after 100 env-steps, the cube's resting contacts plus one arm-only contact (RS layout
# (1, 0)), one arm-cube contact ((0, 1)) or both ((1, 1)).  Found by the oracle census of
# test_gpu_parity.test_one_substep_extra_contact_sweeps over the first 2048 env ids, the smallest
# power of two that yields every category (1024 has two arm-only envs and no arm-cube contact); the
# test below simulates these ids alone and repeats the census on them.
ARM_IDS, COUPLED_IDS, BOTH_IDS = (415, 562, 1174), (2023,), (1560,)


def _bench_states_of(ids, steps, seed=0):
    """test_gpu_parity._bench_states("contact", ...) for the given env ids only."""
    from lerobot_mujoco_sim2real_amd import workloads as W
    cm = W.model("contact")
    orc = Oracle(cm)
    ids = np.asarray(ids)
    st = orc.new_state(len(ids))
    q = W.initial_qpos(cm, ids, seed)
    orc.reset(st, init_qpos=q[:, :5], extra_qpos=q)
    tab = W.chirp_tables(ids, seed)
    for t in range(steps):
        orc.step(st, W.chirp_action(tab, t), nthreads=8)
    return cm, orc, f32(st)


def test_layouts_with_arm_contacts(gpu_lib, monkeypatch):
    """Waves in the layouts (1, 0), (0, 1) and (1, 1): 16 envs (4 waves) per category -- its envs
    repeated among block-only envs, so that a wave holds envs that stop at different sweeps -- and
    16 mixed; one substep against the oracle, and every copy of an env bit-identical to its others
    whatever wave it sits in."""
    monkeypatch.setenv("SOARM_RS", "1")
    fill = tuple(range(16))  # (block-only at t = 100, checked below)
    ids = ARM_IDS + COUPLED_IDS + BOTH_IDS + fill
    cm, orc, st = _bench_states_of(ids, 100)
    names = cm.geom_names
    table, cube = names.index("table"), names.index("cube")

    def category(i):
        fw = orc.forward(st["qpos"][i], st["qvel"][i], st["ctrl"][i], st["warm"][i])
        g = [(int(c[7]), int(c[8])) for c in fw["contacts"]]
        blk = [x for x in g if set(x) == {table, cube}]
        ext = [x for x in g if set(x) != {table, cube}]
        onc = [cube in x for x in ext]
        if not 1 <= len(blk) <= 4:
            return "other"
        if not ext:
            return "block"
        if len(ext) == 1:
            return "coupled" if onc[0] else "arm"
        return "both" if len(ext) == 2 and not onc[0] else "other"

    cats = [category(i) for i in range(len(ids))]
    na, nc = len(ARM_IDS), len(COUPLED_IDS)
    assert cats[:na] == ["arm"] * na and cats[na:na + nc] == ["coupled"] * nc, cats
    assert cats[na + nc:na + nc + len(BOTH_IDS)] == ["both"] * len(BOTH_IDS), cats
    assert cats[-len(fill):] == ["block"] * len(fill), cats
    arm, coupled, both = list(range(na)), list(range(na, na + nc)), list(range(na + nc, na + nc + len(BOTH_IDS)))
    blk = list(range(len(ids) - len(fill), len(ids)))
    pick = []
    for grp in (arm, coupled, both):
        w = [(grp * 16)[k // 2] if k % 2 == 0 else blk[k] for k in range(16)]
        pick += w
    pick += (arm + coupled + both + blk)[:16]
    sub = take(st, np.array(pick))
    sub["ncon"][:] = 0
    S1, p1 = run(cm, sub, substeps=1)
    ref = take(sub, np.arange(len(pick)))
    orc.step(ref, None, nsub=1)
    dv = np.abs(to_np(S1.qvel).T - ref["qvel"]).max(1)
    assert_pct(dv, 4e-5, 2e-4, 5e-4, what="qvel")  # (test_one_substep_extra_contact_sweeps's bars)
    assert to_np(S1.ncon).sum() == ref["ncon"].sum()
    # an env that appears more than once (in waves of the same layout: the layout is the wave's, and
    # another layout sums in another order)
    import torch
    for grp in (arm, coupled, both):
        base = 16 * (arm, coupled, both).index(grp)
        for j in grp:
            at = [base + k for k in range(0, 16, 2) if pick[base + k] == j]
            for k in at[1:]:
                assert_same_bits(rows(p1, torch.tensor([at[0]])), rows(p1, torch.tensor([k])), what=(j, at[0], k))
