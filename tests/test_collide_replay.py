"""k_collide's per-pair records (dmodel.h PairRec) on the narrowphase paths, on a fixture where
nearly every env runs the jaw-cube narrowphase substep after substep.

The replay of last substep's support records (the third part of the collide-chain work) was not
built, so there is no switch to compare against: what stays of its tests is the comparison of two
default batches with each other, bit for bit after every call, and of their contacts for the
fixture with the CPU backend's, which reads the same records by pair."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 320        # two collide blocks, the second a quarter full; 80 RS waves
NSUB = 12
ARM_GEOMS = 13  # geoms 0..12 are the arm's meshes (floor, table and cube follow)


def _fixture_qpos(cm, n):
    """The issue's fixture: arms at W.initial_qpos, the cube within 2 cm of the end effector."""
    from lerobot_mujoco_sim2real_amd import workloads as W
    from lerobot_mujoco_sim2real_amd.sim import BatchSim
    q = W.initial_qpos(cm, np.arange(n), 0)
    S = BatchSim(cm, n)
    ee = S.reset(init_qpos=q[:, :5], extra_qpos=q)[:, :3].cpu().numpy()
    S.close()
    q[:, 6:9] = ee + np.random.default_rng(1).uniform(-0.02, 0.02, (n, 3))
    return q


_QPOS = {}


def fixture_qpos(cm, n, key):
    if key not in _QPOS:
        _QPOS[key] = _fixture_qpos(cm, n)
    return _QPOS[key]


def arm_cube_envs(cm, con, ncon):
    """Envs whose contact list holds a pair of the cube with an arm geom."""
    d = cm.desc
    cube = cm.geom_names.index("cube")
    armcube = np.array([(d.pair_geom1[p] == cube and d.pair_geom2[p] < ARM_GEOMS) or
                        (d.pair_geom2[p] == cube and d.pair_geom1[p] < ARM_GEOMS) for p in range(d.npair)])
    pid = con.cpu().numpy().view(np.int32)[..., 7]
    nc = ncon.cpu().numpy()
    live = np.arange(pid.shape[1])[None, :] < nc[:, None]
    return int((armcube[np.clip(pid, 0, d.npair - 1)] & live).any(1).sum())


def run_pair(cm, n, q):
    """Two default batches from the fixture through 12 single substeps and 2 env-steps (the captured
    graph): bit-equal state and contacts after every call.  Returns the fixture's contacts."""
    import torch
    from lerobot_mujoco_sim2real_amd.sim import BatchSim
    A, B = BatchSim(cm, n), BatchSim(cm, n)
    for S in (A, B):
        S.reset(init_qpos=q[:, :5], extra_qpos=q)
    act = torch.zeros((n, A.nact), dtype=torch.float32, device=A.device)
    first = None

    def same(tag):
        for k in ("obs", "qpos", "qvel", "ncon"):
            assert torch.equal(getattr(A, k), getattr(B, k)), (tag, k)
        (ca, na), (cb, nb) = A.contacts(), B.contacts()
        assert torch.equal(na, nb) and torch.equal(ca, cb), tag
        return ca, na

    for sub in range(NSUB):
        ca, na = same(("before substep", sub))
        if first is None:
            first = (ca.clone(), na.clone())
        if n == N:  # (a condition of the test, not a measurement)
            held = arm_cube_envs(cm, ca, na)
            assert held >= 300, (sub, held)
        A.step(act, frame_skip=1), B.step(act, frame_skip=1)
    for t in range(2):
        same(("before env-step", t))
        A.step(act), B.step(act)
    same("end")
    assert torch.isfinite(A.qpos).all() and int(A.status.abs().sum()) == 0
    return first


def check_against_cpu_backend(cm, n, q, con, ncon, ccd):
    """The device's contacts for the fixture against the CPU backend's (the same fp32 collide code
    compiled for the host, reading the same records by pair).  The host differs in rounding (no
    fused multiply-add, 1 / sqrt for rsqrt: ~6e-8 m on coordinates ~1 m), which can end a solver's
    refinement one step earlier or later.

    native: EPA's depth is the closest face's distance, within MPR_TOLF = 1e-6 m of the boundary on
    either side, so where both hold the same contact its depth agrees within 2 x 1e-6 + rounding
    -> 4e-6.  The normal is the direction of the final portal's /
    face's closest point: a direction an angle t off the optimum loses about depth x t^2 / 2 of
    support distance, so every direction with t <= sqrt(2 x 1e-6 / depth) is within the solver's
    tolerance and the two sides, which may stop on different portals, can differ by twice that
    (+ 1e-5 of rounding).

    mpr: the depth is the distance of the last portal, whatever triangle that is, so a refinement
    that ends one portal apart moves it by more than the tolerance (first device run of this test:
    5e-5 m in one env of 320 where the bound above allows 4e-6).  Two fp32 runs of MPR differ the way
    the device's fp32 run differs from the fp64 oracle's, so the suite's bars for that comparison
    apply (test_gpu_parity.test_contacts_match_oracle, test_cpu_backend's contact test): depth within
    5e-5 + 2% (contacts shallower than 5 mm) or 3% (deeper), normal components within 2e-2, and at most
    max(2, 6%) / max(2, 5%) of the contacts outside them.

    A contact shallower than 2e-5 may exist on one side only: such envs are not compared (at most a
    tenth of them, as in test_cpu_backend's contact test).  The point may slide within a flat contact
    patch, so it is not compared."""
    from lerobot_mujoco_sim2real_amd.sim import BatchSim
    C = BatchSim(cm, n, -1)
    C.reset(init_qpos=q[:, :5], extra_qpos=q)
    cc, nc = C.contacts()
    cc, nc = cc.numpy(), nc.numpy()
    cg, ng = con.cpu().numpy(), ncon.cpu().numpy()
    pg, pc = cg.view(np.int32)[..., 7], cc.view(np.int32)[..., 7]
    checked, gap = 0, np.zeros(2)
    shallow = deep = geo_bad = nrm_bad = deep_bad = 0
    for e in range(n):
        k = int(ng[e])
        if k != nc[e] or (k and min(np.abs(cg[e, :k, 0]).min(), np.abs(cc[e, :k, 0]).min()) < 2e-5):
            continue
        assert (pg[e, :k] == pc[e, :k]).all(), (e, pg[e, :k], pc[e, :k])
        dd = np.abs(cg[e, :k, 0] - cc[e, :k, 0])
        dn = np.abs(cg[e, :k, 4:7] - cc[e, :k, 4:7]).max(-1) if k else np.zeros(0)
        gap = np.maximum(gap, [dd.max(initial=0.0), dn.max(initial=0.0)])
        ad = np.abs(cc[e, :k, 0])
        if ccd == "native":
            assert (dd <= 4e-6).all(), (e, dd)
            assert (dn <= 2 * np.sqrt(2e-6 / ad) + 1e-5).all(), (e, dn, cc[e, :k, 0])
        else:
            sh = ad < 5e-3
            shallow += int(sh.sum())
            deep += int((~sh).sum())
            geo_bad += int((sh & (dd > 5e-5 + 2e-2 * ad)).sum())
            nrm_bad += int((sh & (dn > 2e-2)).sum())
            deep_bad += int((~sh & (dd > 3e-2 * ad)).sum())
        checked += 1
    print(f"compared {checked} of {n} envs: largest depth gap {gap[0]:.2e} m, largest normal gap {gap[1]:.2e}")
    assert checked >= 0.9 * n, (checked, n)
    if ccd != "native":
        print(f"mpr: {shallow} shallow contacts ({geo_bad} depth, {nrm_bad} normal outside), {deep} deep ({deep_bad} outside)")
        assert geo_bad <= max(2, 0.06 * shallow) and nrm_bad <= max(2, 0.06 * shallow), (geo_bad, nrm_bad, shallow)
        assert deep_bad <= max(2, 0.05 * deep), (deep_bad, deep)


@pytest.mark.parametrize("ccd", ["mpr", "native"])
def test_records_on_narrowphase_paths(gpu_lib, ccd):
    from lerobot_mujoco_sim2real_amd import workloads as W
    cm = W.model("contact", ccd=ccd)
    q = fixture_qpos(cm, N, ("pgs", ccd))
    con, ncon = run_pair(cm, N, q)
    check_against_cpu_backend(cm, N, q, con, ncon, ccd)


def test_records_one_env(gpu_lib):
    from lerobot_mujoco_sim2real_amd import workloads as W
    cm = W.model("contact")
    run_pair(cm, 1, fixture_qpos(cm, N, ("pgs", "mpr"))[:1])


def test_records_quad_kernel(gpu_lib, monkeypatch):
    """The collide kernel is shared by every substep kernel: the quad PGS kernel (SOARM_RS=0)."""
    from lerobot_mujoco_sim2real_amd import workloads as W
    monkeypatch.setenv("SOARM_RS", "0")
    cm = W.model("contact")
    run_pair(cm, N, fixture_qpos(cm, N, ("pgs", "mpr")))


def test_records_newton(gpu_lib):
    from lerobot_mujoco_sim2real_amd import workloads as W
    cm = W.model("contact", solver="newton")
    run_pair(cm, N, fixture_qpos(cm, N, ("newton", "mpr")))
