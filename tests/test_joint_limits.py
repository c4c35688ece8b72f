"""The joint-limit rows of the constraint solve on every kernel path: the checks of
tests/joint_limits_ref.py on the library's CPU backend (no GPU needed) and, marked `gpu`, on the
device for the RS kernel (SOARM_RS=1), the quad kernel (SOARM_RS=0), the Newton model and the fused
contact-free kernel with both solvers; and the census that pins tests/golden/joint_limit_states.npz
to what these tests claim to cover.
"""
import numpy as np
import pytest

import joint_limits_ref as J

SOLVERS = ("PGS", "Newton")
# device cases: (kernel name, SOARM_RS, model's solver)
KERNELS = [pytest.param("1", "PGS", id="rs"), pytest.param("0", "PGS", id="quad"),
           pytest.param("1", "Newton", id="newton")]

# (set, jnt_margin) of the one-substep parity on the pick scene
PICK = [("past", 0.0), ("past", J.MARGIN), ("near", J.MARGIN), ("coupled", 0.0)]
FREE = [("past", 0.0), ("past", J.MARGIN), ("near", J.MARGIN)]
FORCES = ("coupled", "past_rest")


@pytest.fixture(scope="module")
def cpu_lib():
    from lerobot_mujoco_sim2real_amd import abi, build
    build.build()
    return abi.load_lib()


def cpu_sim(cm, n):
    from lerobot_mujoco_sim2real_amd.sim import BatchSim
    return BatchSim(cm, n, -1)


def gpu_sim(cm, n):
    from lerobot_mujoco_sim2real_amd.sim import BatchSim
    return BatchSim(cm, n)


def load_state(S, st):
    import torch
    dev = S.device
    S.qpos.copy_(torch.as_tensor(st["qpos"].T, dtype=torch.float32, device=dev))
    S.qvel.copy_(torch.as_tensor(st["qvel"].T, dtype=torch.float32, device=dev))
    S.qacc_warmstart.copy_(torch.as_tensor(st["warm"].T, dtype=torch.float32, device=dev))
    S.ctrl.copy_(torch.as_tensor(st["ctrl"].T, dtype=torch.float32, device=dev))


# ------------------------------------------------------------------------------------- the fixture
def test_fixture_census():
    """The committed states are what the tests claim to cover, recomputed with the oracle alone
    (orc.forward for the rows, their forces and the contact lists, one orc.step for the status)."""
    import contact_overflow_ref as R
    fx = J.fixture()
    for name in J.SETS:
        for k in J.KEYS:  # fp32 values: every backend starts from the same bits
            assert (fx[name][k] == fx[name][k].astype(np.float32)).all() and np.isfinite(fx[name][k]).all()
        assert np.abs(fx[name]["warm"]).max() > 0 and np.abs(fx[name]["ctrl"]).max() > 0  # mid-trajectory
    elbow_upper = (2, 1)
    # ---- past: stock model
    c = J.fixture_census("past")
    n = len(c["nlim"])
    active = c["present"] & (c["force"] > 0)
    idle = (c["present"] & (c["force"] == 0)).any((1, 2))
    viol = -c["dist"][c["present"]]
    print("past:", n, "envs, nlim", np.bincount(c["nlim"]), "active per (joint, side)", active.sum(0).ravel(), "zero-force",
          int(idle.sum()), "ncon", np.bincount(c["ncon"]), "violation %.1e..%.1e" % (viol.min(), viol.max()),
          "largest limit force %.2f" % c["force"].max())
    assert 150 <= n <= 170 and (c["nlim"] >= 1).all() and (c["status"] == 0).all()
    for j in range(J.NA):
        for s in range(2):
            # elbow_flex cannot pass its upper side in this scene without the base 8..12 mm inside
            # the lower arm (make_golden.joint_limit_states): that pair has no env, here or in `near`
            assert active[:, j, s].sum() >= (0 if (j, s) == elbow_upper else 6), (J.JOINTS[j], J.SIDES[s])
    assert not c["present"][:, 2, 1].any()
    assert min((c["nlim"] == k).sum() for k in (1, 2, 3)) >= 24 and (c["nlim"] >= 4).sum() >= 8
    assert (c["nlim"] == J.NA).sum() >= 4  # (all six joints: the kernels' limit list is full)
    assert idle.sum() >= 12
    assert viol.min() >= J.VIOL[0] and viol.max() <= J.VIOL[1] and viol.min() < 3e-4 and viol.max() > 1e-2
    assert np.isin(c["ncon"], (0, 4)).all() and (c["ncon"] == c["nblk"]).all() and (c["ncon_step"] == c["ncon"]).all()
    assert min((c["ncon"] == 0).sum(), (c["ncon"] == 4).sum()) >= 40
    assert (c["graze"] > R.GRAZING).all() and (c["deepest"] > -R.DEEPEST).all()
    # ---- near: no row on the stock model, rows with 0 < dist < margin on the margin model
    c = J.fixture_census("near")
    close = c["dist"] < J.NEAR
    n = len(c["nlim"])
    print("near:", n, "envs, close per (joint, side)", close.sum(0).ravel(), "3+ joints", int((close.sum((1, 2)) >= 3).sum()),
          "ncon", np.bincount(c["ncon"]))
    assert 44 <= n <= 52 and (c["nlim"] == 0).all() and (c["dist"] > 0).all() and (c["status"] == 0).all()
    assert close.any((1, 2)).all() and (close.sum((1, 2)) >= 3).sum() >= 12
    assert all(close[:, j, s].sum() >= 3 for j in range(J.NA) for s in range(2) if (j, s) != elbow_upper)
    assert np.isin(c["ncon"], (0, 4)).all() and (c["ncon"] == c["nblk"]).all()
    assert (c["graze"] > R.GRAZING).all() and (c["deepest"] > -R.DEEPEST).all()
    m = J.fixture_census("near", J.MARGIN)
    assert (m["nlim"] >= 1).all() and (m["nlim"] == close.sum((1, 2))).all() and (m["status"] == 0).all()
    assert ((m["dist"][m["present"]] > 0) & (m["dist"][m["present"]] < J.MARGIN)).all()
    assert (m["present"] & (m["force"] > 0)).any()
    # ---- coupled: limit rows and arm contacts, all in LDS
    c = J.fixture_census("coupled")
    arm = c["ncon"] - c["nblk"]
    active = c["present"] & (c["force"] > 0)
    print("coupled:", len(arm), "envs, nlim", np.bincount(c["nlim"]), "ncon", np.bincount(c["ncon"]), "arm contacts",
          np.bincount(arm), "active per (joint, side)", active.sum(0).ravel(), "largest force %.1f" % c["fmax"].max())
    assert 28 <= len(arm) <= 36 and (c["nlim"] >= 1).all() and (arm >= 1).all() and (c["ncon"] <= R.LDS_CON).all()
    assert (c["status"] == 0).all() and (c["ncon_step"] == c["ncon"]).all()
    assert (c["graze"] > R.GRAZING).all() and (c["deepest"] > -R.DEEPEST).all()
    assert active.any((1, 2)).sum() >= 16 and (active.sum(0) > 0).sum() >= 6
    # ---- fill, and the pool of the wave-composition check
    c = J.fixture_census("fill")
    assert len(c["nlim"]) == 24 and (c["nlim"] == 0).all() and (c["ncon"][:16] == 4).all() and (c["ncon"][16:] == 0).all()
    assert len(J.sparse_targets()) >= 12
    # ---- the contact-free model sees the same rows (the cube's coordinates dropped)
    for name in ("past", "near"):
        for margin in (0.0, J.MARGIN):
            a, b = J.fixture_census(name, margin), J.fixture_census(name, margin, False)
            assert (a["present"] == b["present"]).all() and (b["ncon"] == 0).all() and (b["status"] == 0).all()


@pytest.mark.parametrize("solver", SOLVERS)
def test_crossing_census(solver):
    """The env-step states of check_env_step_crossing, from the oracle stepped substep by substep:
    the number of joints past their range changes inside the step in at least 16 of the 64 envs,
    upwards (entering) and downwards (leaving) in at least 8 each; the oracle-only fp32-noise
    envelope is finite and under 1e-3 in every kept env, and at most 5 % of the draws were left out."""
    X = J.crossing(solver)
    d = np.diff(X["nlim"], axis=0)
    enter, leave = (d > 0).any(0), (d < 0).any(0)
    share = 1 - X["kept"] / X["drawn"]
    print(f"crossing {solver}: entering {int(enter.sum())}, leaving {int(leave.sum())}, both {int((enter & leave).sum())}, "
          f"kept {X['kept']} of {X['drawn']} drawn (left out {100 * share:.1f} %), envelope max {X['envelope'].max():.2e}, "
          f"nlim at the start {np.bincount(X['nlim'][0])}, at the end {np.bincount(X['nlim'][-1])}")
    assert len(X["st"]["qpos"]) == 64 and share <= 0.05
    assert np.isfinite(X["envelope"]).all() and X["envelope"].max() < 1e-3
    assert (enter | leave).sum() >= 16 and enter.sum() >= 8 and leave.sum() >= 8
    assert (X["ref"]["status"] == 0).all()
    for k in ("qpos", "qvel", "warm", "ctrl"):
        assert (X["st"][k] == X["st"][k].astype(np.float32)).all()


# --------------------------------------------------------------------------------- the CPU backend
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name, margin", PICK)
def test_cpu_substep_parity(cpu_lib, solver, name, margin):
    J.check_substep_parity(cpu_sim, load_state, solver, name, margin)


@pytest.mark.parametrize("solver", SOLVERS)
def test_cpu_wave_composition(cpu_lib, solver):
    J.check_wave_composition(cpu_sim, load_state, solver)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name, margin", FREE)
def test_cpu_contact_free(cpu_lib, solver, name, margin):
    J.check_contact_free(cpu_sim, load_state, solver, name, margin)


@pytest.mark.parametrize("solver", SOLVERS)
def test_cpu_domain_randomised(cpu_lib, solver):
    J.check_substep_parity(cpu_sim, load_state, solver, "past", 0.0, dr=True)


@pytest.mark.parametrize("solver", SOLVERS)
def test_cpu_env_step_crossing(cpu_lib, solver):
    J.check_env_step_crossing(cpu_sim, load_state, solver)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", FORCES)
def test_cpu_contact_forces(cpu_lib, solver, name):
    J.check_contact_forces(cpu_sim, load_state, solver, name)


def test_cpu_soft_reset_both_sides(cpu_lib):
    J.check_soft_reset_both_sides(cpu_sim, load_state)


# -------------------------------------------------------------------------------------- the device
@pytest.mark.gpu
@pytest.mark.parametrize("rs, solver", KERNELS)
@pytest.mark.parametrize("name, margin", PICK)
def test_substep_parity(gpu_lib, monkeypatch, rs, solver, name, margin):
    """Measured on an MI355X, qvel gap to the oracle, p50 / p99 / max, device | CPU backend on the
    same states (bars: p99 and max 10 x the CPU backend's; `coupled`: QVEL_BARS):
      past, stock     rs     2.05e-7 / 1.18e-6 / 1.26e-6 | 2.04e-7 / 1.18e-6 / 1.26e-6
                      quad   1.98e-7 / 1.18e-6 / 1.24e-6 | the same
                      newton 2.21e-7 / 1.18e-6 / 1.27e-6 | 2.42e-7 / 1.18e-6 / 1.27e-6
      past, margin    rs     2.51e-7 / 4.09e-7 / 4.24e-7 | 2.48e-7 / 4.23e-7 / 4.25e-7
                      quad   2.50e-7 / 4.24e-7 / 4.61e-7 | the same
                      newton 2.66e-7 / 5.91e-7 / 1.10e-6 | 2.59e-7 / 1.01e-6 / 1.05e-6
      near, margin    rs     2.62e-7 / 3.58e-7 / 3.62e-7 | 2.72e-7 / 3.87e-7 / 3.88e-7
                      quad   2.77e-7 / 3.83e-7 / 3.88e-7 | the same
                      newton 2.36e-7 / 5.46e-7 / 5.54e-7 | 2.57e-7 / 5.93e-7 / 6.26e-7
      coupled         rs     3.55e-7 / 1.86e-5 / 2.57e-5 | 3.01e-7 / 1.26e-5 / 1.56e-5
                      quad   3.70e-7 / 1.85e-5 / 2.57e-5 | the same
                      newton 3.85e-7 / 1.98e-5 / 2.57e-5 | 3.24e-7 / 1.31e-5 / 1.56e-5
    (the test prints all of it, and the worst env of every (joint, side)).  Library builds with the
    upper side's velocity sign not flipped, or with the last record of the limit list skipped in
    the PGS sweep, miss `past` on the stock model by 1.4e-3 and 8e-4..1.3e-3 rad in qpos."""
    monkeypatch.setenv("SOARM_RS", rs)
    J.check_substep_parity(gpu_sim, load_state, solver, name, margin)


@pytest.mark.gpu
@pytest.mark.parametrize("rs, solver", KERNELS)
def test_wave_composition(gpu_lib, monkeypatch, rs, solver):
    monkeypatch.setenv("SOARM_RS", rs)
    J.check_wave_composition(gpu_sim, load_state, solver)


@pytest.mark.gpu
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name, margin", FREE)
def test_contact_free(gpu_lib, solver, name, margin):
    """The fused k_step.  Measured on an MI355X (p50 / p99 / max, device | CPU backend):
      past, stock   PGS 1.97e-7 / 1.17e-6 / 1.26e-6 | 2.06e-7 / 1.18e-6 / 1.26e-6   Newton 2.27e-7 / 1.18e-6 / 1.27e-6 | 2.36e-7 / 1.18e-6 / 1.27e-6
      past, margin  PGS 2.38e-7 / 4.11e-7 / 4.30e-7 | 2.48e-7 / 4.23e-7 / 4.25e-7   Newton 2.57e-7 / 5.82e-7 / 5.99e-7 | 2.59e-7 / 1.04e-6 / 1.28e-6
      near, margin  PGS 2.67e-7 / 3.83e-7 / 3.88e-7 | 2.72e-7 / 3.87e-7 / 3.88e-7   Newton 2.52e-7 / 5.46e-7 / 5.54e-7 | 2.55e-7 / 5.93e-7 / 6.26e-7"""
    J.check_contact_free(gpu_sim, load_state, solver, name, margin)


@pytest.mark.gpu
@pytest.mark.parametrize("rs, solver", KERNELS)
def test_domain_randomised(gpu_lib, monkeypatch, rs, solver):
    monkeypatch.setenv("SOARM_RS", rs)
    J.check_substep_parity(gpu_sim, load_state, solver, "past", 0.0, dr=True)


@pytest.mark.gpu
@pytest.mark.parametrize("rs, solver", KERNELS)
def test_env_step_crossing(gpu_lib, monkeypatch, rs, solver):
    monkeypatch.setenv("SOARM_RS", rs)
    J.check_env_step_crossing(gpu_sim, load_state, solver)


@pytest.mark.gpu
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", FORCES)
def test_contact_forces(gpu_lib, solver, name):
    J.check_contact_forces(gpu_sim, load_state, solver, name)


@pytest.mark.gpu
@pytest.mark.parametrize("rs", ["1", "0"])
def test_soft_reset_both_sides(gpu_lib, monkeypatch, rs):
    monkeypatch.setenv("SOARM_RS", rs)
    J.check_soft_reset_both_sides(gpu_sim, load_state)
