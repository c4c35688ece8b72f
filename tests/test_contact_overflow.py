"""The constraint solve past LDS_CON = 6 contacts per env, up to and over the cap of 16: the
checks of tests/contact_overflow_ref.py on the library's CPU backend (no GPU needed) and, marked
`gpu`, on the device for the RS kernel (SOARM_RS=1), the quad kernel (SOARM_RS=0) and the Newton
model; and the census that pins tests/golden/contact_overflow_states.npz to what these tests claim
to cover.
"""
import numpy as np
import pytest

import contact_overflow_ref as R

SOLVERS = ("PGS", "Newton")
# device cases: (kernel name, SOARM_RS, model's solver)
KERNELS = [pytest.param("1", "PGS", id="rs"), pytest.param("0", "PGS", id="quad"),
           pytest.param("1", "Newton", id="newton")]


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
    """The committed states are what the tests claim to cover, recomputed with the oracle
    (orc.forward for the contact lists, one orc.step for the overflow bit)."""
    from lerobot_mujoco_sim2real_amd import abi
    fx = R.fixture()
    for name in R.SETS:
        for k in R.KEYS:  # fp32 values: every backend starts from the same bits
            assert (fx[name][k] == fx[name][k].astype(np.float32)).all() and np.isfinite(fx[name][k]).all()
    # shallow: 24..32 envs, 7+ contacts, every contact between 20 um and 5 mm deep
    sh = R.fixture_census("shallow")
    assert 24 <= len(sh["ncon"]) <= 32
    assert (sh["ncon"] > R.LDS_CON).all() and (sh["status"] == 0).all()
    assert (sh["deepest"] > -R.DEEPEST).all() and (sh["graze"] > R.GRAZING).all()
    assert (sh["ncon_step"] == sh["ncon"]).all()
    # deep: 7+ contacts, none grazing, at least 8 envs of each class and 3 at each count 9..15
    dp = R.fixture_census("deep")
    n = len(dp["ncon"])
    assert 88 <= n <= 104
    assert (dp["ncon"] > R.LDS_CON).all() and (dp["graze"] > R.GRAZING).all()
    assert (dp["status"] & ~abi.ST_CONOVERFLOW == 0).all() and np.isfinite(dp["qvel"]).all()
    assert (dp["ncon_step"] == dp["ncon"]).all()
    cls = R.classes(dp)
    count = {k: int(v.sum()) for k, v in cls.items()}
    print("deep:", n, "envs,", count, "by ncon", np.bincount(dp["ncon"], minlength=17))
    print("shallow:", len(sh["ncon"]), "envs,", {k: int(v.sum()) for k, v in R.classes(sh).items()},
          "by ncon", np.bincount(sh["ncon"], minlength=17))
    assert min(count.values()) >= 8, count
    assert (np.bincount(dp["ncon"], minlength=17)[9:16] >= 3).all()
    assert (dp["ncon"][cls["over"]] == R.MAXCON).all()
    # fill: 16 resting cubes (the block's 4 contacts alone), 8 lifted cubes (none)
    fl = R.fixture_census("fill")
    assert (fl["ncon"][:16] == 4).all() and (fl["nblk"][:16] == 4).all() and (fl["ncon"][16:] == 0).all()
    assert len(fl["ncon"]) == 24 and (fl["status"] == 0).all()
    # the envs the composition and stale-slab checks pick exist
    over, strad, slab = R.composition_targets()
    assert cls["over"][over] and cls["straddle"][strad] and cls["slab"][slab]
    assert (dp["ncon"] >= 12).sum() >= 6 and (dp["ncon"] == 8).sum() >= 6


# --------------------------------------------------------------------------------- the CPU backend
@pytest.mark.parametrize("solver", SOLVERS)
def test_cpu_shallow_parity(cpu_lib, solver):
    R.check_shallow_parity(cpu_sim, load_state, solver)


@pytest.mark.parametrize("solver", SOLVERS)
def test_cpu_deep_parity(cpu_lib, solver):
    """(The device under test is the CPU backend itself here, so the relative bars hold trivially:
    what this run checks is ncon and the status bits against the oracle, and that at most 1 % of
    the committed deep set is over QVEL_BARS[2] on the CPU backend.)"""
    dv, _ = R.check_deep_parity(cpu_sim, load_state, solver)
    assert (dv > R.QVEL_BARS[2]).sum() <= 0.01 * len(dv), np.flatnonzero(dv > R.QVEL_BARS[2])


@pytest.mark.parametrize("solver", SOLVERS)
def test_cpu_batch_composition(cpu_lib, solver):
    R.check_batch_composition(cpu_sim, load_state, solver)


@pytest.mark.parametrize("solver", SOLVERS)
def test_cpu_stale_slab(cpu_lib, solver):
    R.check_stale_slab(cpu_sim, load_state, solver)


@pytest.mark.parametrize("solver", SOLVERS)
def test_cpu_env_step_repeats(cpu_lib, solver):
    R.check_env_step_repeats(cpu_sim, load_state, solver)


# -------------------------------------------------------------------------------------- the device
@pytest.mark.gpu
@pytest.mark.parametrize("rs, solver", KERNELS)
def test_shallow_parity(gpu_lib, monkeypatch, rs, solver):
    monkeypatch.setenv("SOARM_RS", rs)
    R.check_shallow_parity(gpu_sim, load_state, solver)


@pytest.mark.gpu
@pytest.mark.parametrize("rs, solver", KERNELS)
def test_deep_parity(gpu_lib, monkeypatch, rs, solver):
    """Measured on an MI355X, qvel gap to the oracle over the 96 envs (p50 / p99 / max; none over
    QVEL_BARS[2] = 2.5e-3 on either side), device | CPU backend on the same states:
      rs      1.07e-6 / 8.82e-4 / 9.75e-4 | 1.08e-6 / 3.40e-4 / 7.57e-4   (bars 3.2e-6, 1.02e-3)
      quad    1.12e-6 / 8.82e-4 / 9.75e-4 | the same
      newton  1.09e-6 / 8.88e-4 / 9.79e-4 | 1.09e-6 / 2.35e-4 / 7.57e-4   (bars 3.3e-6, 1.02e-3: the CPU
              backend's PGS line sets them; before the fix of the CPU backend's Newton stopping test its
              Newton line was 1.12e-6 / 1.05e-3 / 1.90e-3 and the bars 3.4e-6, 3.15e-3)
    per class, device max (rs | quad | newton) and CPU backend max (PGS | Newton):
      lds      8.77e-4 | 8.77e-4 | 8.83e-4      3.19e-4 | 2.08e-4
      straddle 1.95e-6 | 1.95e-6 | 1.95e-6      2.70e-6 | 3.90e-6
      slab     6.44e-4 | 6.45e-4 | 6.45e-4      7.57e-4 | 7.57e-4
      full     1.96e-5 | 1.96e-5 | 3.25e-5      3.19e-4 | 2.08e-4
      over     5.15e-6 | 5.15e-6 | 5.41e-6      4.25e-6 | 4.42e-6
    (the test prints all of it, p50 and p99 per class included)."""
    monkeypatch.setenv("SOARM_RS", rs)
    R.check_deep_parity(gpu_sim, load_state, solver)


@pytest.mark.gpu
@pytest.mark.parametrize("rs, solver", KERNELS)
def test_batch_composition(gpu_lib, monkeypatch, rs, solver):
    monkeypatch.setenv("SOARM_RS", rs)
    R.check_batch_composition(gpu_sim, load_state, solver)


@pytest.mark.gpu
@pytest.mark.parametrize("rs, solver", KERNELS)
def test_stale_slab(gpu_lib, monkeypatch, rs, solver):
    monkeypatch.setenv("SOARM_RS", rs)
    R.check_stale_slab(gpu_sim, load_state, solver)


@pytest.mark.gpu
@pytest.mark.parametrize("rs, solver", KERNELS)
def test_env_step_repeats(gpu_lib, monkeypatch, rs, solver):
    monkeypatch.setenv("SOARM_RS", rs)
    R.check_env_step_repeats(gpu_sim, load_state, solver)
