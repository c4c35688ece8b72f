"""box_box (table - cube) and plane_box (floor - cube) beyond the flat resting cube, and the 2-bit
contact-count word they hand to the constraint solve: the checks of tests/box_contacts_ref.py on
the library's CPU backend (no GPU needed) and, marked `gpu`, on the device -- the contact lists
under both convex-convex narrowphases, one substep on the RS kernel (SOARM_RS=1), the quad kernel
(SOARM_RS=0) and the Newton model; and the census of what the poses reach.
"""
import numpy as np
import pytest

import box_contacts_ref as R
from test_contact_overflow import KERNELS, SOLVERS, cpu_sim, gpu_sim

CONTACT_CASES = [pytest.param(r, ccd, id=f"{r}-{ccd}") for r, ccd in R.CONTACT_CASES]


@pytest.fixture(scope="module")
def cpu_lib():
    from lerobot_mujoco_sim2real_amd import abi, build
    build.build()
    return abi.load_lib()


# -------------------------------------------------------------------------------------- the references
def test_census():
    """What the poses reach, from the float64 oracle (contact counts per pair, the leave-out set)
    and the numpy SAT (branch, reference box and face, size of the clipped polygon) alone: at least
    8 envs of each class over all regimes, and at most 3 % of a regime left out."""
    total = R.census()
    for k, v in total.items():
        if k != "left out":
            assert v >= R.CENSUS_MIN, (k, v, total)
    for r in R.REGIMES:
        q = R.poses(r)
        assert len(q) == R.N and 64 <= R.N <= 96 and (q == q.astype(np.float32)).all()
        assert R.oracle_contacts(r)[1].sum() <= R.LEAVE_OUT * R.N, r
    for r, ccd in R.CONTACT_CASES:
        assert R.oracle_contacts(r, ccd)[1].sum() <= R.LEAVE_OUT * R.N, (r, ccd)
    # the envs the composition check picks exist, and the folded arm touches nothing
    assert len(R.composition_targets()) == 5
    fl, tb, cu = R.geoms(R.model())
    for r in R.REGIMES:
        for c in R.oracle_contacts(r)[0]:
            assert (c[:, 8] == cu).all() and np.isin(c[:, 7], (fl, tb)).all(), (r, c)


def test_references_agree():
    """The two references against each other on every env the oracle does not leave out: the numpy
    plane-box contacts and the numpy box-box invariants hold for the oracle's own lists."""
    fl, tb, cu = R.geoms(R.model())
    for r in R.REGIMES:
        cons, out = R.oracle_contacts(r)
        q = R.poses(r)
        for e in np.flatnonzero(~out):
            k = cons[e]
            R.check_plane_box(k[k[:, 7] == fl, :7], q[e])
            R.check_box_box(k[k[:, 7] == tb, :7], q[e])


# ------------------------------------------------------------------------------------ the CPU backend
@pytest.mark.parametrize("regime, ccd", CONTACT_CASES)
def test_cpu_contact_parity(cpu_lib, regime, ccd):
    R.check_contact_parity(cpu_sim, regime, ccd)


@pytest.mark.parametrize("regime, ccd", CONTACT_CASES)
def test_cpu_invariants(cpu_lib, regime, ccd):
    R.check_invariants(cpu_sim, regime, ccd)


@pytest.mark.parametrize("solver", SOLVERS)
def test_cpu_stale_counts(cpu_lib, solver):
    R.check_stale_counts(cpu_sim, solver)


@pytest.mark.parametrize("solver", SOLVERS)
def test_cpu_batch_composition(cpu_lib, solver):
    R.check_batch_composition(cpu_sim, solver)


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("solver", SOLVERS)
def test_cpu_substep(cpu_lib, solver, regime):
    R.check_substep(cpu_sim, solver, regime)


@pytest.mark.parametrize("solver", SOLVERS)
def test_cpu_newton_corner(cpu_lib, solver):
    """Before the fix of the CPU backend's Newton stopping test the 8 envs were 1.0e-3 to 2.1e-3
    from the oracle under Newton (bar 3.5e-4); after it at most 1.1e-6, under PGS 5e-7."""
    R.check_newton_corner(cpu_sim, solver)


# ----------------------------------------------------------------------------------------- the device
@pytest.mark.gpu
@pytest.mark.parametrize("regime, ccd", CONTACT_CASES)
def test_contact_parity(gpu_lib, regime, ccd):
    """Measured on an MI355X, largest gap to the oracle over a regime's 96 envs (no env left out in
    any regime; bars 5e-6, 5e-6, 1e-5), distance / position / normal, the same under MPR and native:
      tilt 7.8e-9 3.0e-8 0        small_tilt 1.3e-9 4.2e-8 0    edge 6.7e-10 2.2e-7 0
      corner 1.6e-8 1.9e-7 1.4e-8 rim 8.9e-8 2.2e-7 1.3e-7      vertex 8.3e-8 1.2e-7 1.2e-7
      side 7.5e-8 6.9e-8 0        floor 3.1e-8 4.5e-8 0         floor_small_tilt 3.0e-8 4.9e-8 0
    The CPU backend's (test_cpu_contact_parity) are within 2e-8 of these but for the normal on rim
    and vertex (2.6e-7, 3.2e-7).  No count mismatch on either."""
    R.check_contact_parity(gpu_sim, regime, ccd)


@pytest.mark.gpu
@pytest.mark.parametrize("regime, ccd", CONTACT_CASES)
def test_invariants(gpu_lib, regime, ccd):
    R.check_invariants(gpu_sim, regime, ccd)


@pytest.mark.gpu
@pytest.mark.parametrize("rs, solver", KERNELS)
def test_stale_counts(gpu_lib, monkeypatch, rs, solver):
    monkeypatch.setenv("SOARM_RS", rs)
    R.check_stale_counts(gpu_sim, solver)


@pytest.mark.gpu
@pytest.mark.parametrize("rs, solver", KERNELS)
def test_batch_composition(gpu_lib, monkeypatch, rs, solver):
    monkeypatch.setenv("SOARM_RS", rs)
    R.check_batch_composition(gpu_sim, solver)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("rs, solver", KERNELS)
def test_substep(gpu_lib, monkeypatch, rs, solver, regime):
    """Measured on an MI355X, 96 envs per regime, qvel gap to the oracle p50 / p99 / max (no env over
    QVEL_BARS[2] anywhere; qpos gap at most 1.4e-7 on the device, 1.9e-7 on the CPU backend), and
    the oracle's envelope p50 / p99 that the bars come from:
                        rs                      quad                    newton                  envelope
      tilt              3.0e-7 1.1e-6 1.3e-6    3.5e-7 9.3e-7 1.1e-6    5.9e-7 3.3e-6 4.7e-6    9.6e-7 3.5e-6
      small_tilt        2.5e-7 6.7e-7 7.1e-7    2.7e-7 6.7e-7 6.9e-7    1.3e-6 6.3e-6 6.8e-6    1.0e-7 1.2e-6
      edge              3.2e-7 1.2e-6 1.3e-6    3.3e-7 1.3e-6 1.3e-6    1.1e-6 6.6e-6 7.3e-6    2.7e-6 2.8e-5
      corner            4.1e-7 2.8e-6 3.2e-6    4.9e-7 2.6e-6 2.8e-6    8.4e-7 3.4e-6 3.5e-6    1.2e-5 3.9e-5
      rim               2.1e-6 1.2e-5 1.3e-5    2.1e-6 1.2e-5 1.4e-5    2.8e-6 1.5e-5 1.6e-5    3.1e-5 1.5e-4
      vertex            2.2e-6 9.6e-6 9.9e-6    2.1e-6 9.4e-6 9.6e-6    2.8e-6 9.6e-6 1.5e-5    4.2e-5 9.6e-5
      side              1.7e-6 7.8e-6 9.8e-6    1.6e-6 8.0e-6 9.9e-6    2.9e-6 1.1e-5 1.2e-5    2.6e-5 6.0e-5
      floor             9.3e-7 4.0e-6 5.1e-6    9.2e-7 4.5e-6 5.2e-6    1.1e-6 4.7e-6 5.1e-6    2.7e-5 5.4e-5
      floor_small_tilt  3.5e-6 7.9e-6 8.4e-6    3.5e-6 7.9e-6 8.7e-6    3.7e-6 1.1e-5 1.2e-5    3.9e-6 7.0e-5
    and on the CPU backend (test_cpu_substep), PGS | Newton:
      tilt              2.6e-7 7.6e-7 8.3e-7 | 6.6e-7 3.1e-6 4.2e-6
      small_tilt        1.3e-7 6.4e-7 9.3e-7 | 6.5e-7 2.6e-6 2.6e-6
      edge              2.0e-7 1.1e-6 1.1e-6 | 8.7e-7 3.9e-6 9.3e-6
      corner            4.1e-7 3.1e-6 4.1e-6 | 8.9e-7 4.2e-6 4.5e-6
      rim               2.1e-6 1.2e-5 1.3e-5 | 2.5e-6 1.3e-5 1.3e-5
      vertex            2.1e-6 9.9e-6 1.6e-5 | 2.3e-6 9.6e-6 1.9e-5
      side              1.8e-6 7.7e-6 1.0e-5 | 2.1e-6 8.7e-6 1.2e-5
      floor             8.8e-7 4.5e-6 5.2e-6 | 1.1e-6 3.9e-6 5.7e-6
      floor_small_tilt  3.4e-6 8.4e-6 8.7e-6 | 3.4e-6 8.6e-6 9.5e-6
    (the test prints all of it).  The p50 bar is QVEL_BARS[0] = 2e-6 on tilt and small_tilt (10 x the
    envelope's median is below it) and 10 x the envelope's median elsewhere; the p99 bar is
    QVEL_BARS[1] = 3.5e-4 except on rim, vertex, side, floor and floor_small_tilt (5.4e-4 to 1.5e-3)."""
    monkeypatch.setenv("SOARM_RS", rs)
    R.check_substep(gpu_sim, solver, regime)


@pytest.mark.gpu
@pytest.mark.parametrize("rs, solver", KERNELS)
def test_newton_corner(gpu_lib, monkeypatch, rs, solver):
    """Measured on an MI355X, largest qvel gap of the 8 envs: rs 4.6e-7, quad 6.1e-7, newton 1.8e-6
    (the device's Newton solve never had the CPU backend's early stop)."""
    monkeypatch.setenv("SOARM_RS", rs)
    R.check_newton_corner(gpu_sim, solver)
