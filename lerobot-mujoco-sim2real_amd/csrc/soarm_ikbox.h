// soarm_ikbox.h — joint-limit-aware site IK (control/casadi_ik.py:27-167): per env and frame the
// minimiser of
//   f(q) = w_pos |p(q) - p*|^2 + w_rot |log3(R(q) R*')|^2 + w_smooth |q - q_last|^2
// over the box lo <= q <= hi of the joint ranges.  The reference hands this to IPOPT; here it is
// a projected Gauss-Newton method (Bertsekas' eps-active set), one lane per env, the frames of a
// trajectory chained inside the call.  Shared by k_ik_box (soarm_sim.hip) and the CPU backend.
//
//   bounds   lo, hi = jnt_range where jnt_limited, else -+FLT_MAX; the start is clamped into the
//            box and is the first frame's q_last
//   e        = quat2vel(site_xquat * conj(target_quat)), angle in (-pi, pi]; 0 without a target quat
//   g        = 2 (w_pos Jp'(p - p*) + w_rot Jr' e + w_smooth (q - q_last))     (exact: e is an
//              eigenvector, eigenvalue 1, of the log map's Jacobian)
//   H        = 2 (w_pos Jp'Jp + w_rot Jr'Jr + w_smooth I)                      (SPD: w_smooth > 0)
//   stop     pg = q - clamp(q - g);  |pg|_inf < tol -> ok
//   step     eps = min(1e-2, |pg|_inf); joint i active if (q_i <= lo_i + eps and g_i > 0) or
//            (q_i >= hi_i - eps and g_i < 0); H's off-diagonal entries in active rows / columns
//            are zeroed, then H d = -g (active joints: -g_i / H_ii, free joints: reduced Newton)
//   search   alpha = 1, 1/2, ... (12 trials): q' = clamp(q + alpha d), accepted when
//            f(q') <= f(q) + 1e-4 g'(q' - q) + 4 FLT_EPSILON |f(q)|  (the last term: the fp32
//            resolution of f, above the true decrease near the optimum); none accepted -> fail
//   frames   frame k starts from frame k-1's output, which is also its q_last; a failed frame's
//            output is the last good solution (control/TrajectoryGenerator.py:180-205), for
//            frame 0 the clamped start
// Joints past ndof, or whose body is no ancestor of the site body, keep their value: identity row
// in H, zero gradient, no bounds.
#pragma once
#include <float.h>

#include "soarm_env.h"

namespace soarm {

// the frame's cost at S (kinematics done): site position sp, position error dp, rotation error er
template <int NA>
HDI float ik_box_cost(const Sim<NA, 0>& S, int site, int sb, int nuse, const float tp[3], const float tqt[4],
                      bool rot, const float qlast[NA], float wp, float wr, float ws, float sp[3], float dp[3],
                      float er[3]) {
  const DModel& m = *S.mp;
  const float lp[3] = {m.site_pos[site][0], m.site_pos[site][1], m.site_pos[site][2]};
  float bq[4] = {1.f, 0.f, 0.f, 0.f};
  sp[0] = sp[1] = sp[2] = 0.f;
#pragma unroll
  for (int b = 1; b < Sim<NA, 0>::NB; b++)
    if (b == sb) {
      float t[3];
      mv(t, S.xmat[b], lp);
      sp[0] = S.xpos[b][0] + t[0], sp[1] = S.xpos[b][1] + t[1], sp[2] = S.xpos[b][2] + t[2];
      bq[0] = S.xquat[b][0], bq[1] = S.xquat[b][1], bq[2] = S.xquat[b][2], bq[3] = S.xquat[b][3];
    }
  dp[0] = sp[0] - tp[0], dp[1] = sp[1] - tp[1], dp[2] = sp[2] - tp[2];
  er[0] = er[1] = er[2] = 0.f;
  float f = wp * dot3(dp, dp);
  if (rot) {
    const float sq_[4] = {m.site_quat[site][0], m.site_quat[site][1], m.site_quat[site][2], m.site_quat[site][3]};
    float sq[4], eq[4];
    qmul(sq, bq, sq_);
    qnormalize(sq);
    const float ct[4] = {tqt[0], -tqt[1], -tqt[2], -tqt[3]};
    qmul(eq, sq, ct);
    const float s = sqrtf(eq[1] * eq[1] + eq[2] * eq[2] + eq[3] * eq[3]);  // mju_quat2Vel, dt = 1
    if (s >= 1e-15f) {
      float speed = 2.f * atan2f(s, eq[0]);
      if (speed > 3.14159265358979f) speed -= 6.28318530717959f;
      er[0] = eq[1] / s * speed, er[1] = eq[2] / s * speed, er[2] = eq[3] / s * speed;
    }
    f += wr * dot3(er, er);
  }
  float sm = 0.f;
#pragma unroll
  for (int i = 0; i < NA; i++) {
    const float dq = S.qpos[i] - qlast[i];
    sm += i < nuse ? dq * dq : 0.f;
  }
  return f + ws * sm;
}

// target [F][N][3]; tq [F][N][4] or null; q [nq][N] in: start, out: the last frame; q_traj
// [F][nq][N] or null; ok [F][N]; iters [F][N] or null
template <int NA>
HDI void env_ik_box(const DModel* __restrict__ dm, int n, int e, int nframe, const float* __restrict__ target,
                    const float* __restrict__ tq, float* __restrict__ q, float* __restrict__ q_traj,
                    int32_t* __restrict__ ok, int32_t* __restrict__ iters, const sim_ik_box_opts& o) {
  const DModel& m = *dm;
  Sim<NA, 0> S(dm, 1.f, -1.f, 1.f);
  const int site = o.site, sb = m.site_bodyid[site];
  // hinge i moves the site iff its body (i + 2: the chain is serial) is an ancestor of the site body
  const int nuse = o.ndof < sb - 1 ? o.ndof : sb - 1;
  const bool rot = tq != nullptr;
  const float wp = (float)o.w_pos, wr = rot ? (float)o.w_rot : 0.f, ws = (float)o.w_smooth, tol = (float)o.tol;
  float lo[NA], hi[NA], qc[NA];  // qc: the last good solution (every value of it is inside the box)
#pragma unroll
  for (int i = 0; i < NA; i++) {
    const bool lim = i < nuse && m.jnt_limited[i] != 0;
    lo[i] = lim ? m.jnt_range[i][0] : -FLT_MAX;
    hi[i] = lim ? m.jnt_range[i][1] : FLT_MAX;
    qc[i] = fminf(fmaxf(q[(size_t)i * n + e], lo[i]), hi[i]);
  }
  for (int fr = 0; fr < nframe; fr++) {
    const size_t fe = (size_t)fr * n + e;
    const float tp[3] = {target[3 * fe], target[3 * fe + 1], target[3 * fe + 2]};
    float tqt[4] = {1.f, 0.f, 0.f, 0.f};
    if (rot)
#pragma unroll
      for (int k = 0; k < 4; k++) tqt[k] = tq[4 * fe + k];
    float qlast[NA], qn[NA], sp[3], dp[3], er[3];
#pragma unroll
    for (int i = 0; i < NA; i++) qlast[i] = qn[i] = S.qpos[i] = qc[i];
    S.kinematics();
    float f = ik_box_cost<NA>(S, site, sb, nuse, tp, tqt, rot, qlast, wp, wr, ws, sp, dp, er);
    int success = 0, it = 0;
    for (; it < o.max_steps; it++) {
      // site jacobian at qn (S holds its kinematics), gradient, Gauss-Newton Hessian
      float Jp[3][NA], Jr[3][NA], g[NA], H[NA * (NA + 1) / 2];
#pragma unroll
      for (int i = 0; i < NA; i++) {
        const float r[3] = {sp[0] - S.anchor[i][0], sp[1] - S.anchor[i][1], sp[2] - S.anchor[i][2]};
        float c[3];
        cross(c, S.axis[i], r);
        const bool use = i < nuse;
#pragma unroll
        for (int k = 0; k < 3; k++) Jp[k][i] = use ? c[k] : 0.f, Jr[k][i] = use ? S.axis[i][k] : 0.f;
      }
      float pgn = 0.f;
#pragma unroll
      for (int a = 0; a < NA; a++) {
        const bool use = a < nuse;
        float gp = 0.f, gr = 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) gp += Jp[k][a] * dp[k], gr += Jr[k][a] * er[k];
        g[a] = use ? 2.f * (wp * gp + wr * gr + ws * (qn[a] - qlast[a])) : 0.f;
        pgn = fmaxf(pgn, fabsf(qn[a] - fminf(fmaxf(qn[a] - g[a], lo[a]), hi[a])));
#pragma unroll
        for (int b = 0; b <= a; b++) {
          float hp = 0.f, hr = 0.f;
#pragma unroll
          for (int k = 0; k < 3; k++) hp += Jp[k][a] * Jp[k][b], hr += Jr[k][a] * Jr[k][b];
          const float h = 2.f * (wp * hp + wr * hr);
          H[a * (a + 1) / 2 + b] = a == b ? (use ? h + 2.f * ws : 1.f) : h;
        }
      }
      if (pgn < tol) {
        success = 1;
        break;
      }
      const float eps = fminf(1e-2f, pgn);
      bool act[NA];
#pragma unroll
      for (int a = 0; a < NA; a++)
        act[a] = (qn[a] <= lo[a] + eps && g[a] > 0.f) || (qn[a] >= hi[a] - eps && g[a] < 0.f);
      float ng[NA], d[NA], Hd[NA];
#pragma unroll
      for (int a = 0; a < NA; a++) {
        ng[a] = -g[a];
#pragma unroll
        for (int b = 0; b < a; b++)
          if (act[a] || act[b]) H[a * (a + 1) / 2 + b] = 0.f;
      }
      ldl_factor<NA>(H, Hd);
      ldl_solve<NA>(H, Hd, d, ng);
      // backtracking over the projection arc; a rejected trial redoes the kinematics at the
      // smaller step, the accepted one's stay in S for the next iteration
      bool acc = false;
      float alpha = 1.f;
      for (int t = 0; t < 12 && !acc; t++, alpha *= 0.5f) {
        float qt[NA], gd = 0.f;
#pragma unroll
        for (int i = 0; i < NA; i++) {
          qt[i] = fminf(fmaxf(qn[i] + alpha * d[i], lo[i]), hi[i]);
          gd += g[i] * (qt[i] - qn[i]);
          S.qpos[i] = qt[i];
        }
        S.kinematics();
        float sp_[3], dp_[3], er_[3];
        const float ft = ik_box_cost<NA>(S, site, sb, nuse, tp, tqt, rot, qlast, wp, wr, ws, sp_, dp_, er_);
        if (ft <= f + 1e-4f * gd + 4.f * FLT_EPSILON * fabsf(f)) {
          acc = true, f = ft;
#pragma unroll
          for (int i = 0; i < NA; i++) qn[i] = qt[i];
#pragma unroll
          for (int k = 0; k < 3; k++) sp[k] = sp_[k], dp[k] = dp_[k], er[k] = er_[k];
        }
      }
      if (!acc) break;
    }
    if (success)
#pragma unroll
      for (int i = 0; i < NA; i++) qc[i] = qn[i];
    ok[fe] = success;
    if (iters) iters[fe] = it;
    if (q_traj) {
      float* qf = q_traj + (size_t)fr * m.nq * n;
#pragma unroll
      for (int i = 0; i < NA; i++) qf[(size_t)i * n + e] = qc[i];
      for (int i = NA; i < m.nq; i++) qf[(size_t)i * n + e] = q[(size_t)i * n + e];
    }
  }
#pragma unroll
  for (int i = 0; i < NA; i++) q[(size_t)i * n + e] = qc[i];
}

}  // namespace soarm
