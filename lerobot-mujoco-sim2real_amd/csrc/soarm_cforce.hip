// soarm_cforce.hip — the contact-force readout's kernel (sim_contact_forces, include/soarm_sim.h):
// mj_forward at the current state + mj_contactForce of every contact.  Its own translation unit:
// the step's kernels (soarm_sim.hip) sit on their register limit and stay byte for byte what they
// are; this one shares only the per-env physics headers with them.
//
// k_contact_force<NA, NF, SOL> is the dense solve the CPU backend also runs (soarm_cpu.hip), on the
// one statement of the rows both share (soarm_dense.h: MuJoCo's order -- dof frictionloss, joint
// limits lower/upper, 4 pyramid edges per contact in contact order -- with the rows' constants, force
// and cost, the contact frame and Jacobian, the packed Cholesky solve and the pyramid decode), solved
// by mj_solPGS's Gauss-Seidel in that order or mj_solNewton's primal Newton with the exact line
// search, laid out for the GPU: 16 lanes per env (one DPP row), 4 envs per
// wave.  Lane l of an env owns rows r = l (mod 16), one per slot s = r / 16; the slots are unrolled,
// so a lane's per-row scalars (aref, R, frictionloss, AR diagonal, force) are registers.  The lanes
// build their rows' Jacobians and W = M^-1 J' in parallel (the bulk of the work) into LDS rows
// [r][J | W]; the smooth dynamics before that run on every lane of the env (identical values).
//   PGS    : the serial sweep visits rows in order; the owner forms the projected step, the group
//            reads it by a lane broadcast and every lane moves its copy of v by W_r df (W_r: an LDS
//            broadcast read).
//   Newton : cost, gradient, Hessian and the line search's derivative are sums over rows -- per-lane
//            partial sums over the slots, then rowsum16 (soarm_rs.h), which leaves the same bits in
//            all 16 lanes, so every branch on them is uniform over the env's lanes.
// An env's result depends on nothing but its own state: the other envs of its wave only decide
// how long the wave loops (a converged env's steps are exact zeros / skipped).
#include <hip/hip_runtime.h>

#include "soarm_collide.h"
#include "soarm_env.h"
#include "sim_internal.h"
#include "soarm_dense.h"
#include "soarm_pgs.h"

using namespace soarm;

namespace {

constexpr int CF_LPE = 16;            // lanes per env
constexpr int CF_EPW = 64 / CF_LPE;   // envs per wave (workgroup)

template <int NA, int NF>
struct CfDims {
  static constexpr int NV = NA + 6 * NF;
  static constexpr int MAXR = NV + 2 * NA + 4 * SIM_MAXCON;
  static constexpr int NSL = (MAXR + CF_LPE - 1) / CF_LPE;  // row slots per lane
  static constexpr int NROW = NSL * CF_LPE;                 // LDS rows (rows past the env's are zero)
  static constexpr int ROWF = 2 * NV + 1;                   // J | W, odd stride: the lanes' rows on distinct banks
  static constexpr int NH = NV * (NV + 1) / 2;
};

template <int NA, int NF, int SOL>
__global__ __launch_bounds__(64) void k_contact_force(const DModel* __restrict__ dm, int n, sim_state st,
                                                      sim_params pp, const float* __restrict__ cbuf,
                                                      uint32_t* __restrict__ pmask, float* __restrict__ contacts,
                                                      float* __restrict__ force, int32_t* __restrict__ ncon_out) {
  using D = CfDims<NA, NF>;
  constexpr int NV = D::NV, NSL = D::NSL, ROWF = D::ROWF;
  const int lane = (int)threadIdx.x % CF_LPE, col = (int)threadIdx.x / CF_LPE;
  // (no early return: the groups past the batch's end run a copy of the last env and write nothing,
  // so every barrier below is reached by the whole wave)
  const int e_raw = (int)blockIdx.x * CF_EPW + col;
  const bool live = e_raw < n;
  const int e = live ? e_raw : n - 1;
  const DModel& m = *dm;
  Sim<NA, NF> S(dm, pp.mass_scale ? pp.mass_scale[e] : 1.f, pp.friction ? pp.friction[e] : -1.f,
                pp.damping_scale ? pp.damping_scale[e] : 1.f);
  load_state(S, st, n, e);

  __shared__ float s_rows[CF_EPW][D::NROW * ROWF];  // [r][J(NV) | W(NV)]
  __shared__ float s_con[CF_EPW][SIM_MAXCON * 8];   // the env's contacts as sim_contacts writes them
  __shared__ float s_fe[CF_EPW][D::NROW];           // the solution's force per row
  __shared__ float s_bp[CF_EPW][D::NROW + CF_LPE];  // Newton: the line search's breakpoints
  float* const rows = s_rows[col];
  float* const con = s_con[col];

  // ---- the env's contact list: the pairs in order, each pair's contacts in slot order, at most
  // SIM_MAXCON kept (every lane of the env walks it and stores the same values)
  int ncon = 0;
  if (m.npair > 0) {
    PairMask pm;
    pm.load(pmask, m, n, e);
    for (int p = 0; p < m.npair; p++) {
      const int c = (pm.w[p >> 5] >> (p & 31)) & 1u ? pm.count(m, p) : 0;
      const int s0 = m.pair_slot[p];
      for (int k = 0; k < c && ncon < SIM_MAXCON; k++, ncon++) {
#pragma unroll
        for (int f = 0; f < 7; f++) con[ncon * 8 + f] = cbuf[((size_t)(s0 + k) * 7 + f) * n + e];
        con[ncon * 8 + 7] = __int_as_float(p);
      }
    }
  }
  for (int k = ncon * 8 + lane; k < SIM_MAXCON * 8; k += CF_LPE) con[k] = 0.f;
  __syncthreads();

  // ---- smooth dynamics (mj_forward's position, velocity and the unconstrained acceleration)
  S.kinematics();
  S.com_crb();
  S.factor();
  S.smooth_forces();
  if (st.qfrc_applied) S.add_applied(st.qfrc_applied, n, e);
  S.solve_m(S.qacc_s, S.fsmooth);

  // ---- the lane's rows (mj_makeConstraint: soarm_dense.h states each kind; a lane finds "row r of
  // the env" by counting the rows before it in MuJoCo's order)
  int type[NSL];
  float aref[NSL], R[NSL], fl[NSL], ARd[NSL], f[NSL];
  float pv[NV];  // PGS: this lane's part of sum_r W_r f_r (the warm start's v)
#pragma unroll
  for (int i = 0; i < NV; i++) pv[i] = 0.f;
  int nr = 0;
#pragma unroll
  for (int s = 0; s < NSL; s++) {
    const int r = lane + CF_LPE * s;
    float J[NV], W[NV];
#pragma unroll
    for (int i = 0; i < NV; i++) J[i] = 0.f;
    // (an absent row: J = 0, aref = 0, R = 1 -- its force stays an exact zero in either solver)
    type[s] = ROW_NONE, aref[s] = 0.f, R[s] = 1.f, fl[s] = 0.f;
    auto put = [&](int t, const RowConst& c) { type[s] = t, aref[s] = c.aref, R[s] = c.R, fl[s] = c.fl; };
    int k = 0;
#pragma unroll
    for (int i = 0; i < NV; i++) {  // dof frictionloss
      if (!(m.dof_frictionloss[i] > 0.f)) continue;
      if (k == r) {
        J[i] = 1.f;
        put(ROW_FRICTION, friction_row(m, i, S.qvel[i]));
      }
      k++;
    }
#pragma unroll
    for (int i = 0; i < NA; i++) {  // joint limits, lower then upper
      if (!m.jnt_limited[i]) continue;
#pragma unroll
      for (int side = 0; side < 2; side++) {
        const float dist = side == 0 ? S.qpos[i] - m.jnt_range[i][0] : m.jnt_range[i][1] - S.qpos[i];
        if (!(dist < m.jnt_margin[i])) continue;
        if (k == r) {
          J[i] = side == 0 ? 1.f : -1.f;
          put(ROW_LIMIT, limit_row(m, i, side, dist, S.qvel[i]));
        }
        k++;
      }
    }
    const int r0 = k;  // first contact row
    nr = r0 + 4 * ncon;
    if (r >= r0 && r < nr) {  // pyramid edge ed of contact c (condim 3)
      const int c = (r - r0) >> 2, ed = (r - r0) & 3;
      const float cdist = con[c * 8];
      const float cpos[3] = {con[c * 8 + 1], con[c * 8 + 2], con[c * 8 + 3]};
      const float cn[3] = {con[c * 8 + 4], con[c * 8 + 5], con[c * 8 + 6]};
      const int p = __float_as_int(con[c * 8 + 7]);
      const float mu = S.fric >= 0.f ? S.fric : m.pair_friction[p];
      float fr[9], jd[3][NV], imp, R0, Rpy;
      contact_frame(cn, fr);
      contact_jac(S, m.pair_body1[p], m.pair_body2[p], cpos, fr, jd);
      contact_consts(m, p, mu, cdist, imp, R0, Rpy);
      put(ROW_CONTACT, {edge_row(m, jd, ed, mu, S.qvel, p, imp, cdist, J), Rpy, 0.f});
    }
    S.solve_m(W, J);
    float jw = 0.f, jar = -aref[s];
#pragma unroll
    for (int i = 0; i < NV; i++) {
      jw += J[i] * W[i];
      jar += J[i] * S.warm[i];
      rows[r * ROWF + i] = J[i];
      rows[r * ROWF + NV + i] = W[i];
    }
    ARd[s] = jw + R[s];
    f[s] = warm_force(type[s], R[s], fl[s], jar);  // PGS's warm start: the forces implied by qacc_warmstart
#pragma unroll
    for (int i = 0; i < NV; i++) pv[i] += W[i] * f[s];
  }
  __syncthreads();

  const float scale = m.pgs_scale, tol = m.tolerance;
  const int iters = m.iterations;
  // J_r x for this lane's row of slot s
  auto jdot = [&](int s, const float (&x)[NV]) {
    const float* Jr = rows + (lane + CF_LPE * s) * ROWF;
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < NV; i++) d += Jr[i] * x[i];
    return d;
  };

  if constexpr (SOL == SIM_SOL_PGS) {
    // ------------------------------------------------------------------ mj_solPGS
    float v[NV];
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = S.qacc_s[i] + rowsum16(pv[i]);
    {  // the warm start is kept if its dual cost beats f = 0
      float pc = 0.f;
#pragma unroll
      for (int s = 0; s < NSL; s++) {
        const float jv = jdot(s, v), jq = jdot(s, S.qacc_s);
        pc += 0.5f * f[s] * (jv - aref[s] + R[s] * f[s]) + 0.5f * f[s] * (jq - aref[s]);
      }
      if (rowsum16(pc) > 0.f) {
#pragma unroll
        for (int s = 0; s < NSL; s++) f[s] = 0.f;
#pragma unroll
        for (int i = 0; i < NV; i++) v[i] = S.qacc_s[i];
      }
    }
    // the wave sweeps as far as its longest env; rows past an env's own are zero rows
    int nrmax = nr;
    nrmax = max(nrmax, __shfl_xor(nrmax, 16));
    nrmax = max(nrmax, __shfl_xor(nrmax, 32));
    bool done = false;
    for (int it = 0; it < iters; it++) {
      if (__all(done)) break;
      float improvement = 0.f;
#pragma unroll
      for (int s = 0; s < NSL; s++) {
        if (CF_LPE * s >= nrmax) continue;
        float Jr[NV];
#pragma unroll
        for (int i = 0; i < NV; i++) Jr[i] = rows[(lane + CF_LPE * s) * ROWF + i];
        const int qn = min(CF_LPE, nrmax - CF_LPE * s);
#pragma unroll 1
        for (int q = 0; q < qn; q++) {
          // every lane forms its own row's step from the current v; row q's (its turn) is taken
          float res = -aref[s] + R[s] * f[s];
#pragma unroll
          for (int i = 0; i < NV; i++) res += Jr[i] * v[i];
          float fn = f[s] - res / ARd[s];
          fn = pgs_project(type[s], fl[s], fn);
          const bool mine = lane == q && !done && type[s] != ROW_NONE;
          const float dfo = mine ? fn - f[s] : 0.f;
          const float df = __shfl(dfo, q, CF_LPE);
          if (mine && dfo != 0.f) {
            f[s] = fn;
            improvement -= dfo * (res + 0.5f * ARd[s] * dfo);
          }
          if (df != 0.f) {
            const float* Wr = rows + (CF_LPE * s + q) * ROWF + NV;
#pragma unroll
            for (int i = 0; i < NV; i++) v[i] += Wr[i] * df;
          }
        }
      }
      improvement = rowsum16(improvement);
      if (improvement * scale < tol) done = true;
    }
  } else {
    // ------------------------------------------------------------------ mj_solNewton
    // c(a) = 1/2 (a - a0)' M (a - a0) + sum_r s_r(J_r a - aref_r); jar = J a - aref
    auto cost_at = [&](const float (&a)[NV], float (&jar)[NSL]) {
      float da[NV], Mda[NV], c = 0.f, pc = 0.f;
#pragma unroll
      for (int i = 0; i < NV; i++) da[i] = a[i] - S.qacc_s[i];
      mul_m(S, da, Mda);
#pragma unroll
      for (int i = 0; i < NV; i++) c += 0.5f * da[i] * Mda[i];
#pragma unroll
      for (int s = 0; s < NSL; s++) {
        jar[s] = jdot(s, a) - aref[s];
        pc += row_cost(type[s], R[s], fl[s], jar[s]);
      }
      return c + rowsum16(pc);
    };
    float a[NV], jar[NSL], jv[NSL];
    {  // warm start (mj_fwdConstraint): qacc_warmstart unless qacc_smooth costs less
      const float cw = cost_at(S.warm, jar), cs = cost_at(S.qacc_s, jar);
#pragma unroll
      for (int i = 0; i < NV; i++) a[i] = cw < cs ? S.warm[i] : S.qacc_s[i];
    }
    float cost = cost_at(a, jar);
    // one iteration; false: the solve has stopped (every test is uniform over the env's lanes)
    auto iterate = [&]() -> bool {
      float da[NV], g[NV], pg[NV], H[D::NH];
#pragma unroll
      for (int i = 0; i < NV; i++) da[i] = a[i] - S.qacc_s[i], pg[i] = 0.f;
      mul_m(S, da, g);
#pragma unroll
      for (int k = 0; k < D::NH; k++) H[k] = 0.f;
#pragma unroll
      for (int s = 0; s < NSL; s++) {
        const float* Jr = rows + (lane + CF_LPE * s) * ROWF;
        bool q;
        const float fr = row_force(type[s], R[s], fl[s], jar[s], q);
        const float Dq = q ? 1.f / R[s] : 0.f;
#pragma unroll
        for (int i = 0; i < NV; i++) {
          pg[i] += Jr[i] * fr;
#pragma unroll
          for (int k = 0; k <= i; k++) H[tri(i, k)] += Dq * Jr[i] * Jr[k];
        }
      }
      float gn = 0.f;
#pragma unroll
      for (int i = 0; i < NV; i++) {
        g[i] -= rowsum16(pg[i]);
        gn += g[i] * g[i];
#pragma unroll
        for (int k = 0; k <= i; k++) H[tri(i, k)] = m_at(S, i, k) + rowsum16(H[tri(i, k)]);
      }
      if (scale * sqrtf(gn) < tol || gn == 0.f) return false;
      float p[NV], mg[NV];
#pragma unroll
      for (int i = 0; i < NV; i++) mg[i] = -g[i];
      if (!chol_solve<NV>(H, p, mg)) return false;
      float Mp[NV], pMp = 0.f, g0 = 0.f, dz = 0.f;
      mul_m(S, p, Mp);
#pragma unroll
      for (int i = 0; i < NV; i++) pMp += p[i] * Mp[i], g0 += da[i] * Mp[i], dz += g[i] * p[i];
      if (!(dz < 0.f)) return false;  // not a descent direction at fp32 resolution: converged
#pragma unroll
      for (int s = 0; s < NSL; s++) jv[s] = jdot(s, p);
      // d/dalpha c(a + alpha p) = g0 + alpha pMp - sum_r f_r(jar_r + alpha jv_r) jv_r, and its slope
      auto deriv = [&](float alpha, float* curv) {
        float pgs = 0.f, ph = 0.f;
#pragma unroll
        for (int s = 0; s < NSL; s++) {
          bool q;
          pgs -= row_force(type[s], R[s], fl[s], jar[s] + alpha * jv[s], q) * jv[s];
          if (q) ph += jv[s] * jv[s] / R[s];
        }
        if (curv) *curv = pMp + rowsum16(ph);
        return g0 + alpha * pMp + rowsum16(pgs);
      };
      // the exact minimiser over alpha >= 0 of the convex piecewise-quadratic c(a + alpha p): the
      // root of its increasing piecewise-linear derivative, between the two neighbouring zone
      // breakpoints that bracket it.  No sort: the lanes post their rows' breakpoints in LDS and
      // every one inside the current bracket is tried in turn (an LDS broadcast read) and
      // tightens one end.
      float alpha;
      {
        float lo = 0.f, glo = deriv(0.f, nullptr);
        if (glo >= 0.f) return false;
        float hi = INFINITY, ghi = 0.f;
        float* const bps = s_bp[col];  // [r] the row's first breakpoint | [NROW + r] a frictionloss row's second
#pragma unroll
        for (int s = 0; s < NSL; s++) {
          const bool fric = type[s] == ROW_FRICTION;
          float b0 = INFINITY, b1 = INFINITY;
          if (type[s] != ROW_NONE && jv[s] != 0.f) {
            const float al0 = ((fric ? -R[s] * fl[s] : 0.f) - jar[s]) / jv[s], al1 = (R[s] * fl[s] - jar[s]) / jv[s];
            if (al0 > 0.f) b0 = al0;
            if (fric && al1 > 0.f) b1 = al1;
          }
          bps[lane + CF_LPE * s] = b0;
          if (s == 0) bps[D::NROW + lane] = b1;  // (frictionloss rows are rows r < NV <= 16: slot 0)
        }
        wave_sync();
#pragma unroll 1
        for (int j = 0; j < nr + CF_LPE; j++) {
          const float b = bps[j < nr ? j : D::NROW + (j - nr)];
          if (!(b > lo && b < hi)) continue;
          const float gb = deriv(b, nullptr);
          if (gb >= 0.f)
            hi = b, ghi = gb;
          else
            lo = b, glo = gb;
        }
        wave_sync();  // (the next iteration's posts follow these reads)
        if (hi < INFINITY) {
          alpha = lo + (hi - lo) * (-glo) / (ghi - glo);
        } else {
          float h;
          deriv(lo + 1.f, &h);  // the last (unbounded) piece's curvature
          alpha = lo - glo / h;
        }
      }
      if (!(alpha > 0.f)) return false;
      float an[NV], jn[NSL];
#pragma unroll
      for (int i = 0; i < NV; i++) an[i] = a[i] + alpha * p[i];
      const float cn = cost_at(an, jn);
      if (!(cn <= cost + 1e-5f * fabsf(cost))) return false;  // a real increase (numerical trouble): keep a
      // the stopping tests of solve_newton (soarm_cpu.hip): the quadratic model's improvement along
      // p, and a full step that leaves every row in its zone
      float changed = 0.f;
#pragma unroll
      for (int s = 0; s < NSL; s++) {
        bool q0, q1;
        const float f0 = row_force(type[s], R[s], fl[s], jar[s], q0), f1 = row_force(type[s], R[s], fl[s], jn[s], q1);
        if (!(q0 == q1 && (q0 || f0 == f1))) changed += 1.f;
        jar[s] = jn[s];
      }
      const bool same = rowsum16(changed) == 0.f;
#pragma unroll
      for (int i = 0; i < NV; i++) a[i] = an[i];
      cost = cn;
      return !(scale * (-0.5f * alpha * dz) < tol || (same && fabsf(alpha - 1.f) < 1e-3f));
    };
    bool done = false;
    for (int it = 0; it < iters; it++) {
      if (__all(done)) break;
      if (!done) done = !iterate();
    }
    // efc_force as MuJoCo derives it from qacc
#pragma unroll
    for (int s = 0; s < NSL; s++) {
      bool q;
      f[s] = row_force(type[s], R[s], fl[s], jar[s], q);
    }
  }

  // ---- mju_decodePyramid per contact (lane c takes contact c)
#pragma unroll
  for (int s = 0; s < NSL; s++) s_fe[col][lane + CF_LPE * s] = type[s] != ROW_NONE ? f[s] : 0.f;
  __syncthreads();
  static_assert(SIM_MAXCON <= CF_LPE, "one lane per contact");
  if (live && lane < SIM_MAXCON) {
    const int c = lane;
    float fo[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c < ncon) {
      const int p = __float_as_int(con[c * 8 + 7]);
      const float mu = S.fric >= 0.f ? S.fric : m.pair_friction[p];
      const float cn[3] = {con[c * 8 + 4], con[c * 8 + 5], con[c * 8 + 6]};
      float fr[9];
      contact_frame(cn, fr);
      decode_pyramid(&s_fe[col][nr - 4 * ncon + 4 * c], mu, fr, fo);
    }
#pragma unroll
    for (int q = 0; q < 6; q++) force[((size_t)e * SIM_MAXCON + c) * 6 + q] = fo[q];
    if (contacts)
#pragma unroll
      for (int q = 0; q < 8; q++) contacts[((size_t)e * SIM_MAXCON + c) * 8 + q] = con[c * 8 + q];
  }
  if (live && lane == 0) {
    ncon_out[e] = ncon;
    for (int w = 0; w < pmask_words(m); w++) soa(pmask, w, n, e) = 0u;  // consumed: clear for the next collide
  }
}

}  // namespace

int launch_contact_force(int nf, int sol, const DModel* d_model, int n, const sim_state& st, const sim_params& pp,
                         const float* cbuf, uint32_t* pmask, float* contacts, float* force, int32_t* ncon,
                         void* stream) {
  dispatch_nf(nf, [&](auto nfc) {
    dispatch_sol(sol, [&](auto solc) {
      constexpr int NA = 6, NF = decltype(nfc)::value, SOL = decltype(solc)::value;
      hipLaunchKernelGGL((k_contact_force<NA, NF, SOL>), dim3((n + CF_EPW - 1) / CF_EPW), dim3(64), 0,
                         (hipStream_t)stream, d_model, n, st, pp, cbuf, pmask, contacts, force, ncon);
    });
  });
  return (int)hipGetLastError();
}
