"""``Kinematics``: the reference's joint-limit-aware IK class over ``sim_ik_box``.

Reference: ``control/casadi_ik.py:11-167``.  There the problem

    minimise  10 |p(q) - p*|^2 + 0.1 |log3(R(q) R*')|^2 + 0.1 |q - q_last|^2
    subject   lowerPositionLimit <= q <= upperPositionLimit

is built symbolically (pinocchio.casadi) and handed to IPOPT (``tol`` 1e-4).  Here the same cost
over the same box is minimised by the projected Gauss-Newton method of ``csrc/soarm_ikbox.h`` on a
one-env batch, and the feed-forward torque ``rnea(q, 0, 0)`` is ``sim_bias`` at the solution
with zero velocity.  The interior-point path is not reproduced: what agrees is the minimiser.

Same surface: ``Kinematics(ee_frame)``, ``buildFromMJCF(path)``, ``ik(T, current_arm_motor_q,
current_arm_motor_dq) -> (dof, info)`` with ``info = {"sol_tauff", "success"}``; ``init_data``
carries the last solution to the next call (start and smoothing anchor).  A solve that does not
converge raises, as the reference re-raises IPOPT's error.
"""
import numpy as np

from ..mjcf import compile_mjcf, mat2quat
from ..sim import BatchSim


class Kinematics:
    def __init__(self, ee_frame, device=0) -> None:
        """ee_frame: the end-effector site's name ("gripperframe"); device: HIP ordinal, or -1 for
        the CPU backend."""
        self.frame_name = ee_frame
        self.device = device

    def buildFromMJCF(self, mcjf_file):
        self.cm = compile_mjcf(mcjf_file, obs_site=self.frame_name)
        self.createSolver()

    def buildFromURDF(self, urdf_file):
        raise NotImplementedError("Kinematics.buildFromURDF: this package compiles MJCF only; "
                                  "buildFromMJCF(path) is the supported route")

    def createSolver(self):
        self.sim = BatchSim(self.cm, 1, self.device)
        self.nq, self.nv = self.sim.nq, self.sim.nv
        self.narm = _count_arm_hinges(self.cm)
        # the reference starts from zeros(nq); joints that are not arm hinges keep qpos0
        self.init_data = np.array(self.cm.qpos0(), dtype=np.float64)
        self.init_data[: self.narm] = 0.0
        self.opts = {}  # w_pos / w_rot / w_smooth / tol / max_steps overrides (BatchSim.ik_bounded)

    def ik(self, T, current_arm_motor_q=None, current_arm_motor_dq=None):
        """T: 4x4 target pose of the end-effector site in the world frame."""
        torch = self.sim.torch
        if current_arm_motor_q is not None:
            cur = np.asarray(current_arm_motor_q, dtype=np.float64).ravel()
            self.init_data = self.init_data.copy()
            self.init_data[: len(cur)] = cur
        T = np.asarray(T, dtype=np.float64)
        q = torch.as_tensor(self.init_data.astype(np.float32).reshape(-1, 1), device=self.sim.device).contiguous()
        q, ok, _ = self.sim.ik_bounded(T[:3, 3].reshape(1, 3), q=q, target_quat=mat2quat(T[:3, :3]),
                                       ndof=self.narm, **self.opts)
        sol_q = q[:, 0].cpu().numpy().astype(np.float64)
        self.init_data = sol_q  # (on failure: the start clamped into the joint ranges)
        if not bool(ok[0]):
            raise RuntimeError(f"Kinematics.ik did not converge; motorstate: {current_arm_motor_q}, pose:\n{T}")
        # rnea(q, v = 0, a = 0): the gravity torque
        self.sim.qpos.copy_(q)
        self.sim.qvel.zero_()
        tau = self.sim.bias()[:, 0].cpu().numpy().astype(np.float64)
        sol_tauff = np.concatenate([tau, np.zeros(max(0, self.nq - len(tau)))])
        info = {"sol_tauff": sol_tauff, "success": True}
        dof = np.zeros(self.nq)
        dof[: len(sol_q)] = sol_q
        return dof, info


def _count_arm_hinges(cm):
    """The leading hinges of the model (the arm chain: qpos address == dof address)."""
    from .. import abi
    d, n = cm.desc, 0
    while n < d.njnt and d.jnt_type[n] == abi.JNT_HINGE:
        n += 1
    return n
