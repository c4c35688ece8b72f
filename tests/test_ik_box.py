"""sim_ik_box: the joint-limit-aware site IK (control/casadi_ik.py:27-167; csrc/soarm_ikbox.h).

The reference minimises 10|p - p*|^2 + 0.1|log3(R R*')|^2 + 0.1|q - q_last|^2 inside the joint
limits with IPOPT, which is not available here; what these tests pin is the problem, not IPOPT's
path: every output lies in the box (1), a converged output is a KKT point of that cost over that
box, measured in float64 with this file's own kinematics (2), and it agrees with a float64 numpy
restatement of the same projected Gauss-Newton method, `RefIK` below, built on
mjcf.NumpyKinematics (3).  The same assertions run on the CPU backend (no GPU needed) and on the
device (marked gpu).

Bars (derived, none fitted to the library's output):
  (2) |pg|_inf <= 2 tol.  The library accepted on its float32 projected gradient below tol; that
      gradient differs from the float64 one by about 2 w_pos |J| (fp32 FK error ~1e-6) ~ 1e-5.
  (3) |q - q_ref| <= 1e-3.  Two points with |pg| < tol lie within 2 tol / lambda_min(H) of each
      other and lambda_min(H) >= 2 w_smooth: 2 * 1e-4 / 0.2.  (H is the Gauss-Newton matrix, not
      the true Hessian: a derived bar, not a proof.  A wrong bound, weight or Jacobian row moves q
      by more than 1e-2.)  At most 2 % of the envs may be left out (either side not converged),
      and at least 40 % of the reference solutions must have a joint exactly on a bound.
"""
import ctypes as C

import numpy as np
import pytest

from lerobot_mujoco_sim2real_amd import abi, build, mjcf

BACKENDS = [pytest.param(-1, id="cpu"), pytest.param(0, id="gpu", marks=pytest.mark.gpu)]
NDOF = 5
W_POS, W_ROT, W_SMOOTH, TOL, MAX_STEPS = 10.0, 0.1, 0.1, 1e-4, 100
FLT_MAX, FLT_EPS = float(np.finfo(np.float32).max), float(np.finfo(np.float32).eps)
N_SINGLE, N_CHAIN, F_CHAIN = 130, 70, 7  # 130: two full waves and a 2-lane tail


# ------------------------------------------------------------------ the float64 restatement
class RefIK:
    """The algorithm of csrc/soarm_ikbox.h in float64 numpy (the box is the library's: jnt_range
    rounded to float32)."""

    def __init__(self, cm, ndof=NDOF, w_pos=W_POS, w_rot=W_ROT, w_smooth=W_SMOOTH, tol=TOL, max_steps=MAX_STEPS):
        d = cm.desc
        self.cm, self.kin, self.site = cm, mjcf.NumpyKinematics(cm), d.obs_site
        self.sb = d.site_bodyid[self.site]
        self.na = 6
        self.used = np.array([i < ndof and self.kin.is_ancestor(d.dof_bodyid[i], self.sb) for i in range(self.na)])
        self.lo = np.array([np.float32(d.jnt_range[i][0]) if self.used[i] and d.jnt_limited[i] else -FLT_MAX
                            for i in range(self.na)], dtype=np.float64)
        self.hi = np.array([np.float32(d.jnt_range[i][1]) if self.used[i] and d.jnt_limited[i] else FLT_MAX
                            for i in range(self.na)], dtype=np.float64)
        self.w = (w_pos, w_rot, w_smooth)
        self.tol, self.max_steps = tol, max_steps

    def clamp(self, q):
        return np.minimum(np.maximum(q, self.lo), self.hi)

    def _full(self, q):
        qf = np.array(self.cm.qpos0(), dtype=np.float64)
        qf[:self.na] = q
        return qf

    def fk(self, q):
        k = self.kin.forward_position(self._full(q))
        return k.site_xpos(self.site), k.site_xquat(self.site)

    def errors(self, q, tp, tq):
        """(p, dp, e) at q: site position, position error, rotation error (mju_quat2Vel of
        site * conj(target), the angle wrapped to (-pi, pi]; 0 without a target quaternion)"""
        p, sq = self.fk(q)
        e = np.zeros(3)
        if tq is not None:
            eq = mjcf.quat_mul(sq, np.array([tq[0], -tq[1], -tq[2], -tq[3]]))
            s = np.linalg.norm(eq[1:])
            if s >= 1e-15:
                speed = 2.0 * np.arctan2(s, eq[0])
                if speed > np.pi:
                    speed -= 2.0 * np.pi
                e = eq[1:] / s * speed
        return p, p - tp, e

    def cost(self, q, tp, tq, qlast):
        wp, wr, ws = self.w
        _, dp, e = self.errors(q, tp, tq)
        dq = (q - qlast) * self.used
        return wp * dp @ dp + wr * e @ e + ws * dq @ dq

    def grad_hess(self, q, tp, tq, qlast):
        wp, wr, ws = self.w
        if tq is None:
            wr = 0.0
        p, dp, e = self.errors(q, tp, tq)
        jp, jr = self.kin.jac(p, self.sb)  # world-frame site Jacobians; only the moved joints count
        jp, jr = jp[:, :self.na] * self.used, jr[:, :self.na] * self.used
        g = 2.0 * (wp * jp.T @ dp + wr * jr.T @ e + ws * (q - qlast)) * self.used
        H = 2.0 * (wp * jp.T @ jp + wr * jr.T @ jr + ws * np.eye(self.na))
        for i in range(self.na):
            if not self.used[i]:
                H[i, :] = H[:, i] = 0.0
                H[i, i] = 1.0
        return g, H

    def proj_grad(self, q, tp, tq, qlast):
        g, _ = self.grad_hess(q, tp, tq, qlast)
        return q - self.clamp(q - g)

    def solve(self, q0, tp, tq):
        """one frame from the (already clamped) start q0 = q_last -> (q, ok, iters)"""
        q, qlast = q0.copy(), q0.copy()
        f = self.cost(q, tp, tq, qlast)
        it = 0
        while it < self.max_steps:
            g, H = self.grad_hess(q, tp, tq, qlast)
            pgn = np.max(np.abs(q - self.clamp(q - g)))
            if pgn < self.tol:
                return q, True, it
            eps = min(1e-2, pgn)
            act = ((q <= self.lo + eps) & (g > 0)) | ((q >= self.hi - eps) & (g < 0))
            for i in np.nonzero(act)[0]:
                hii = H[i, i]
                H[i, :] = H[:, i] = 0.0
                H[i, i] = hii
            d = np.linalg.solve(H, -g)
            alpha, acc = 1.0, False
            for _ in range(12):
                qt = self.clamp(q + alpha * d)
                ft = self.cost(qt, tp, tq, qlast)
                if ft <= f + 1e-4 * g @ (qt - q) + 4.0 * FLT_EPS * abs(f):
                    q, f, acc = qt, ft, True
                    break
                alpha *= 0.5
            if not acc:
                return q, False, it
            it += 1
        return q, False, it

    def chain(self, q0, tps, tqs):
        """frames chained: a failed frame outputs the last good solution -> (traj [F, na], ok [F])"""
        good = self.clamp(q0)
        traj, oks = [], []
        for f in range(len(tps)):
            q, ok, _ = self.solve(good, tps[f], None if tqs is None else tqs[f])
            if ok:
                good = q
            traj.append(good.copy())
            oks.append(ok)
        return np.array(traj), np.array(oks)


# ------------------------------------------------------------------ inputs and references (made once)
class Case:
    pass


_cache = {}


def ref_for(cm):
    if "ref" not in _cache:
        _cache["ref"] = RefIK(cm)
    return _cache["ref"]


def single_case(cm):
    """N_SINGLE envs: pose = FK(q_t), q_t up to 0.5 rad outside the ranges; start = the clamped q_t
    perturbed by up to 0.15 rad, clamped.  Reference solutions for the pose and position-only solves."""
    if "single" in _cache:
        return _cache["single"]
    R, rng, c = ref_for(cm), np.random.default_rng(1), Case()
    n = N_SINGLE
    lo, hi = R.lo[:NDOF], R.hi[:NDOF]
    qt = np.zeros((n, 6))
    qt[:, :NDOF] = rng.uniform(lo - 0.5, hi + 0.5, (n, NDOF))
    fk = [R.fk(q) for q in qt]
    c.tp = np.array([p for p, _ in fk]).astype(np.float32)
    c.tq = np.array([s for _, s in fk]).astype(np.float32)
    q0 = qt.copy()
    q0[:, :NDOF] = np.clip(np.clip(qt[:, :NDOF], lo, hi) + rng.uniform(-0.15, 0.15, (n, NDOF)), lo, hi)
    c.q0 = q0.astype(np.float32)
    c.qlast = R.clamp(c.q0.astype(np.float64))
    c.ref = {}
    for name, tq in (("pose", c.tq), ("pos", None)):
        sol = [R.solve(c.qlast[e], c.tp[e].astype(np.float64), None if tq is None else tq[e].astype(np.float64))
               for e in range(n)]
        q, ok = np.array([s[0] for s in sol]), np.array([s[1] for s in sol])
        # what the issue's prototype showed on these inputs, re-checked for this seed and size
        assert ok.all(), f"restatement: {name} ok on {ok.mean():.3f} of the envs"
        on_bound = ((q[:, :NDOF] == lo) | (q[:, :NDOF] == hi)).any(axis=1)
        assert on_bound.mean() >= 0.4, f"restatement: {name} has a joint on a bound in {on_bound.mean():.3f}"
        c.ref[name] = (q, ok, on_bound)
    _cache["single"] = c
    return c


def chain_case(cm):
    """N_CHAIN envs x F_CHAIN frames: FK along a straight joint-space ramp from an in-range q_a to a
    q_b that lies 0.4 rad past the range on two joints."""
    if "chain" in _cache:
        return _cache["chain"]
    R, rng, c = ref_for(cm), np.random.default_rng(2), Case()
    n, F = N_CHAIN, F_CHAIN
    lo, hi = R.lo[:NDOF], R.hi[:NDOF]
    qa, qb = np.zeros((n, 6)), np.zeros((n, 6))
    qa[:, :NDOF] = rng.uniform(lo + 0.1, hi - 0.1, (n, NDOF))
    qb[:, :NDOF] = np.clip(qa[:, :NDOF] + rng.uniform(-0.5, 0.5, (n, NDOF)), lo, hi)
    for e in range(n):
        j = rng.choice(NDOF, 2, replace=False)
        up = rng.random(2) < 0.5
        qb[e, j] = np.where(up, hi[j] + 0.4, lo[j] - 0.4)
    c.tp, c.tq = np.zeros((F, n, 3), np.float32), np.zeros((F, n, 4), np.float32)
    for f in range(F):
        for e in range(n):
            p, s = R.fk(qa[e] + (f + 1) / F * (qb[e] - qa[e]))
            c.tp[f, e], c.tq[f, e] = p, s
    c.q0 = qa.astype(np.float32)
    c.qlast = R.clamp(c.q0.astype(np.float64))
    sol = [R.chain(c.q0[e].astype(np.float64), c.tp[:, e].astype(np.float64), c.tq[:, e].astype(np.float64))
           for e in range(n)]
    c.ref_traj = np.array([s[0] for s in sol]).transpose(1, 0, 2)  # [F, n, na]
    c.ref_ok = np.array([s[1] for s in sol]).T  # [F, n]
    _cache["chain"] = c
    return c


# ------------------------------------------------------------------ running the library
def make_sim(request, cm, n, dev):
    from lerobot_mujoco_sim2real_amd.sim import BatchSim
    if dev >= 0:
        request.getfixturevalue("gpu_lib")
    else:
        build.build()
    return BatchSim(cm, n, dev)


def to_np(t):
    return t.detach().cpu().numpy()


def run_single(S, c, tq, tp=None, **opts):
    import torch
    q = torch.as_tensor(c.q0.T.copy(), device=S.device)
    q, ok, it = S.ik_bounded(c.tp if tp is None else tp, q=q, target_quat=tq, ndof=NDOF, **opts)
    return to_np(q).T.copy(), to_np(ok).astype(bool), to_np(it)


def assert_feasible(R, q32):
    """lo <= q <= hi on the moved joints, compared in float32, exactly"""
    lo32, hi32 = R.lo[:NDOF].astype(np.float32), R.hi[:NDOF].astype(np.float32)
    q32 = np.asarray(q32, dtype=np.float32)[..., :NDOF]
    assert np.isfinite(q32).all()
    assert (q32 >= lo32).all() and (q32 <= hi32).all(), (
        f"outside the box by {max((lo32 - q32).max(), (q32 - hi32).max()):.3e}")


def assert_optimal(R, q, ok, tps, tqs, qlast):
    worst = 0.0
    for e in np.nonzero(ok)[0]:
        pg = R.proj_grad(q[e].astype(np.float64), tps[e].astype(np.float64),
                         None if tqs is None else tqs[e].astype(np.float64), qlast[e])
        worst = max(worst, np.max(np.abs(pg)))
    print(f"largest float64 projected gradient of a converged env: {worst:.3e} (bar {2 * TOL:.1e})")
    assert worst <= 2 * TOL


def assert_agrees(q, ok, q_ref, ok_ref, what=""):
    both = ok & ok_ref
    left_out = 1.0 - both.mean()
    err = np.abs(q[both][:, :NDOF] - q_ref[both][:, :NDOF]).max() if both.any() else 0.0
    print(f"{what}: left out {left_out:.4f} (bar 0.02), max |q - q_ref| {err:.3e} (bar 1e-3)")
    assert left_out <= 0.02
    assert err <= 1e-3


def check_single(request, cm, dev, name):
    R, c = ref_for(cm), single_case(cm)
    S = make_sim(request, cm, N_SINGLE, dev)
    tq = c.tq if name == "pose" else None
    q, ok, it = run_single(S, c, tq)
    q_ref, ok_ref, on_bound = c.ref[name]
    print(f"{name}: ok {ok.mean():.4f}, iterations max {it.max()}, on a bound (reference) {on_bound.mean():.3f}")
    assert_feasible(R, q)
    assert (q[:, NDOF:] == c.q0[:, NDOF:]).all()  # joints past ndof keep their value
    assert_optimal(R, q, ok, c.tp, tq, c.qlast)
    assert_agrees(q, ok, q_ref, ok_ref, name)
    assert on_bound[ok & ok_ref].mean() >= 0.4
    # targets 3x out of reach: still inside the box, converged or not
    q3, ok3, _ = run_single(S, c, tq, tp=3.0 * c.tp)
    assert_feasible(R, q3)
    assert_optimal(R, q3, ok3, 3.0 * c.tp, tq, c.qlast)


# ------------------------------------------------------------------ tests 1-4: one frame
@pytest.mark.parametrize("dev", BACKENDS)
def test_pose_feasible_optimal_and_matches_restatement(request, arm_model, dev):
    check_single(request, arm_model, dev, "pose")


@pytest.mark.parametrize("dev", BACKENDS)
def test_position_only_feasible_optimal_and_matches_restatement(request, arm_model, dev):
    check_single(request, arm_model, dev, "pos")


# ------------------------------------------------------------------ tests 5-6: chained frames
def run_chain(S, c, **opts):
    import torch
    q = torch.as_tensor(c.q0.T.copy(), device=S.device)
    q, ok, it, traj = S.ik_bounded(c.tp, q=q, target_quat=c.tq, ndof=NDOF, **opts)
    return to_np(q), to_np(ok).astype(bool), to_np(it), to_np(traj)


@pytest.mark.parametrize("dev", BACKENDS)
def test_chained_frames(request, arm_model, dev):
    import torch
    cm = arm_model
    R, c = ref_for(cm), chain_case(cm)
    S = make_sim(request, cm, N_CHAIN, dev)
    q, ok, it, traj = run_chain(S, c)
    assert traj.shape == (F_CHAIN, S.nq, N_CHAIN) and ok.shape == (F_CHAIN, N_CHAIN)
    assert_feasible(R, traj.transpose(0, 2, 1))
    assert q.tobytes() == traj[-1].tobytes()  # the in/out buffer is the last frame, bit for bit
    print(f"chain: ok {ok.mean():.4f} (reference {c.ref_ok.mean():.4f}), iterations max {it.max()}")
    for f in range(F_CHAIN):
        assert_agrees(traj[f].T, ok[f], c.ref_traj[f], c.ref_ok[f], f"frame {f}")
    # a converged frame is optimal for its own q_last, the previous frame's output
    prev = c.qlast
    for f in range(F_CHAIN):
        assert_optimal(R, traj[f].T, ok[f], c.tp[f], c.tq[f], prev)
        prev = traj[f].T.astype(np.float64)
    # F = 1 called F times, q fed back: the same trajectory, bit for bit
    q1 = torch.as_tensor(c.q0.T.copy(), device=S.device)
    for f in range(F_CHAIN):
        q1, ok1, it1 = S.ik_bounded(c.tp[f], q=q1, target_quat=c.tq[f], ndof=NDOF)
        assert to_np(q1).tobytes() == traj[f].tobytes(), f"frame {f}"
        assert (to_np(ok1).astype(bool) == ok[f]).all() and (to_np(it1) == it[f]).all()


@pytest.mark.parametrize("dev", BACKENDS)
def test_failed_frame_repeats_last_good_solution(request, arm_model, dev):
    cm = arm_model
    R, c = ref_for(cm), chain_case(cm)
    S = make_sim(request, cm, N_CHAIN, dev)
    start = np.clip(c.q0[:, :NDOF], R.lo[:NDOF].astype(np.float32), R.hi[:NDOF].astype(np.float32))
    for max_steps in (1, 3):  # 1: (nearly) every frame fails; 3: a mix of converged and failed frames
        q, ok, it, traj = run_chain(S, c, max_steps=max_steps)
        assert (it <= max_steps).all() and not ok.all()
        assert_feasible(R, traj.transpose(0, 2, 1))
        prev = start
        for f in range(F_CHAIN):
            cur = traj[f].T[:, :NDOF]
            assert (cur[~ok[f]] == prev[~ok[f]]).all(), f"frame {f}"
            prev = cur
        if not ok.any():
            assert (traj[-1].T[:, :NDOF] == start).all()


# ------------------------------------------------------------------ test 7: arguments
@pytest.mark.parametrize("dev", BACKENDS)
def test_bad_arguments_are_rejected(request, arm_model, dev):
    import torch
    S = make_sim(request, arm_model, 4, dev)
    lib = S.lib
    f32 = dict(dtype=torch.float32, device=S.device)
    t, tq = torch.zeros((1, 4, 3), **f32), torch.zeros((1, 4, 4), **f32)
    q, traj = torch.zeros((S.nq, 4), **f32), torch.zeros((1, S.nq, 4), **f32)
    ok = torch.zeros((1, 4), dtype=torch.int32, device=S.device)
    it = torch.zeros((1, 4), dtype=torch.int32, device=S.device)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def opts(**kw):
        o = dict(w_pos=W_POS, w_rot=W_ROT, w_smooth=W_SMOOTH, tol=TOL, max_steps=MAX_STEPS,
                 site=arm_model.desc.obs_site, ndof=NDOF)
        o.update(kw)
        return abi.IkBoxOpts(o["w_pos"], o["w_rot"], o["w_smooth"], o["tol"], o["max_steps"], o["site"], o["ndof"], 0)

    def call(b=S._batch, nframe=1, target=p(t), q_=p(q), ok_=p(ok), o=None, null_opts=False):
        o = opts() if o is None else o
        return lib.sim_ik_box(b, nframe, target, p(tq), q_, p(traj), ok_, p(it), None if null_opts else C.byref(o),
                              S._stream())

    assert call() == 0  # the well-formed call the cases below each break in one place
    if dev >= 0:
        torch.cuda.synchronize()
    bad = [dict(b=None), dict(target=None), dict(q_=None), dict(ok_=None), dict(null_opts=True),
           dict(nframe=0), dict(nframe=-3),
           dict(o=opts(w_smooth=0.0)), dict(o=opts(w_smooth=-0.1)), dict(o=opts(w_pos=-1.0)),
           dict(o=opts(w_rot=-1.0)), dict(o=opts(tol=0.0)), dict(o=opts(tol=-1e-4)),
           dict(o=opts(w_smooth=float("nan"))),
           dict(o=opts(site=-1)), dict(o=opts(site=arm_model.desc.nsite)),
           dict(o=opts(ndof=0)), dict(o=opts(ndof=7))]
    for kw in bad:
        assert call(**kw) == abi.E_ARG, kw
        assert lib.sim_last_error(), kw
    for field, val in (("struct_size", C.sizeof(abi.IkBoxOpts) - 8), ("abi_version", abi.ABI_VERSION - 1)):
        o = opts()
        setattr(o, field, val)
        assert call(o=o) == abi.E_ARG
        assert b"sim_ik_box_opts" in lib.sim_last_error() and b"struct_size / abi_version" in lib.sim_last_error()
    with pytest.raises(TypeError):
        S.ik_bounded(np.zeros((4, 3), np.float32), rot_weight=0.5)


# ------------------------------------------------------------------ test 8: the Kinematics class
@pytest.mark.parametrize("dev", BACKENDS)
def test_kinematics_class(request, arm_model, dev):
    from lerobot_mujoco_sim2real_amd.control.casadi_ik import Kinematics
    if dev >= 0:
        request.getfixturevalue("gpu_lib")
    else:
        build.build()
    R = ref_for(arm_model)
    arm = Kinematics("gripperframe", device=dev)
    with pytest.raises(NotImplementedError, match="MJCF"):
        arm.buildFromURDF("so101.urdf")
    arm.buildFromMJCF(mjcf.SCENE_XML)
    assert arm.init_data.shape == (arm.nq,) and not arm.init_data[:6].any()

    def pose(q):
        p, s = R.fk(q)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = mjcf.quat2mat(s), p
        return T, p, s

    rng = np.random.default_rng(3)
    mid, half = 0.5 * (R.lo[:NDOF] + R.hi[:NDOF]), 0.5 * (R.hi[:NDOF] - R.lo[:NDOF])
    qs = np.zeros((2, 6))
    qs[0, :NDOF] = mid + 0.5 * half * rng.uniform(-1, 1, NDOF)
    qs[1, :NDOF] = qs[0, :NDOF] + 0.05 * rng.uniform(-1, 1, NDOF)
    start = qs[0].copy()
    start[:NDOF] += 0.1 * np.sign(mid - qs[0, :NDOF])  # 0.1 rad away on every joint, inside the ranges
    T, p, s = pose(qs[0])
    dof, info = arm.ik(T, current_arm_motor_q=start)
    assert info["success"] is True and dof.shape == (arm.nq,)
    assert_feasible(R, dof[None])
    qlast = R.clamp(start.astype(np.float32).astype(np.float64))
    p = p.astype(np.float32).astype(np.float64)
    pg = R.proj_grad(dof[:6], p, mjcf.mat2quat(T[:3, :3]).astype(np.float32).astype(np.float64), qlast)
    assert np.max(np.abs(pg)) <= 2 * TOL
    # sol_tauff = rnea(q, 0, 0): BatchSim.bias at that q with zero velocity
    import torch
    from lerobot_mujoco_sim2real_amd.sim import BatchSim
    B = BatchSim(arm_model, 1, dev)
    B.qpos.copy_(torch.as_tensor(dof.astype(np.float32).reshape(-1, 1)))
    tau = to_np(B.bias())[:, 0]
    assert info["sol_tauff"].shape == (arm.nq,)
    np.testing.assert_allclose(info["sol_tauff"][:arm.nv], tau, rtol=0, atol=1e-6)
    assert np.abs(tau).max() > 1e-3  # (gravity does load the arm here)
    # the second call warm-starts from the first (init_data), which is also its smoothing anchor
    np.testing.assert_array_equal(arm.init_data[:6], dof[:6])
    T2, p2, s2 = pose(qs[1])
    dof2, info2 = arm.ik(T2)
    assert info2["success"]
    p2 = p2.astype(np.float32).astype(np.float64)
    pg2 = R.proj_grad(dof2[:6], p2, mjcf.mat2quat(T2[:3, :3]).astype(np.float32).astype(np.float64),
                      dof[:6].astype(np.float32).astype(np.float64))
    assert np.max(np.abs(pg2)) <= 2 * TOL
    # a solve that does not converge raises, as the reference re-raises
    arm.opts = dict(max_steps=0)
    with pytest.raises(RuntimeError, match="did not converge"):
        arm.ik(pose(qs[0])[0])


# ------------------------------------------------------------------ the trajectory generator
@pytest.mark.parametrize("dev", BACKENDS)
def test_generator_bounded_path(request, arm_model, dev):
    """generate_bounded solves the path as one chained call; solve_batch(bounded=True) reaches the
    same kernel with independent targets."""
    from lerobot_mujoco_sim2real_amd.control import CartesianTrajectoryGenerator
    if dev >= 0:
        request.getfixturevalue("gpu_lib")
    else:
        build.build()
    R = ref_for(arm_model)
    gen = CartesianTrajectoryGenerator(model=arm_model, device=dev, time_horizon=4)
    xyz, q, t = gen.generate_bounded("Fig8", target_orientation=None)
    assert q.shape == (len(xyz), NDOF) and len(t) == len(xyz)
    assert_feasible(R, q)
    q0 = np.tile(arm_model.qpos0(), (len(xyz), 1))
    qb, okb, _ = gen.solve_batch(xyz, q0=q0, bounded=True)
    assert qb.shape == (len(xyz), arm_model.nq) and okb.dtype == bool
    assert_feasible(R, qb)
    assert_optimal(R, qb, okb, xyz.astype(np.float32), None, R.clamp(q0[:, :6].astype(np.float64)))
    # the chain's first point starts where the independent solve of that point starts
    np.testing.assert_array_equal(q[0], qb[0, :NDOF])
