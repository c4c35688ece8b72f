// soarm_prof.h — the phase profiler of the diagnostic build (-DSOARM_PHASE_PROF, tools/phase_prof.py):
// its device globals, the macros the kernels stamp with, and the reductions that close a kernel's
// profile.  In the default build every macro here expands to nothing, so the kernel headers carry
// the stamps without an #ifdef; included by soarm_pgs.h.
#pragma once

namespace soarm {

#ifdef SOARM_PHASE_PROF
constexpr bool PHASE_PROF = true;
// a declaration / a statement of the diagnostic build only (PROF_DECL(int n = 0); PROF_DO(n++);)
#define PROF_DECL(...) __VA_ARGS__
#define PROF_DO(...) __VA_ARGS__
#define PHASE_T(v) const long long v = clock64()

// per-env PGS start/end clock, sweep count, fast-path flag (env < 65536):
//   [0] sweeps start, [1] solve end, [2] sweeps, [3] variant and census bits (solve_constraints),
//   [4] active limits, [5] contacts, [6] rows built, [7] warm start + cost done
__device__ long long g_pgs_prof[65536 * 8];
// fine-grained per-env clock stamps of one k_substep: see k_substep
__device__ long long g_stamp[65536 * 16];
#define PSTAMP(k) \
  if (e < 65536) g_stamp[16 * e + (k)] = clock64()
// per-wave accumulators of k_substep's phase profile: summed wave cycles per phase
//   [0] state load + checks, [1] kinematics..smooth forces, [2] constraint rows,
//   [3] PGS sweeps, [4] qacc/fcon + Euler + obs + geom poses, [5] waves,
//   [6] sum over envs of PGS sweeps, [7] env count, [8] max wave cycles,
//   [9] waves on the register fast path, [10] max wave PGS cycles,
//   [11] sum over waves of the wave's max sweep count, [12] waves with an active
//   joint limit, [13] waves with a contact outside the register block, [14] waves
//   with more than LDS_CON contacts, [15] max contacts of an env, [16] rows: up to
//   the built contact rows, [17] rows: warm start + cost, [18] rows: block setup
//   [19..22] waves per sweep variant (y-pure, y+arm slot, block-first general, other),
//   [23..26] max wave cycles per variant, [27] waves with a non-block contact on the free body
//   [28..42] wave cycles between consecutive fine stamps (g_stamp, see PSTAMP sites)
//   [43..52] per-lane census of lanes in waves on a non-y sweep (prof_substep_end)
//   [53..56] contact-row build split (g_rowprof),
//   [57] waves that retired the arm rows, [58] sum of their retire sweeps,
//   [59] / [60] max wave cycles of the waves that did not / did retire
//   y+arm slot waves by (F slot, E coupled to the cube) = 2 F + coupled:
//   [61..64] waves, [65..68] max wave cycles, [69..72] sum of PGS
//   cycles, [73..76] sum of the arm-retire sweep (0: not retired)
//   [77..81] the RS solve's split (prof_rs_split)
// Lane 0 of each wave owns its row and launches are stream-ordered, so plain
// read-modify-writes: shared-address atomics from every wave queued behind the profiled kernel's own
// loads and inflated the phases after the solve ~15x (r05).  sim_phase_profile reduces the rows.
// [82..84]: RS-kernel waves that took the v-form fallback -- count, max and summed wave cycles;
// [85..91] lanes of such waves by cause (rs_why bits).
constexpr int WPH = 92, WPH_MAXW = 16384;
__device__ unsigned long long g_wphase[WPH_MAXW * WPH];
#define WPH_ID() (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6)
__device__ int g_rs_force11;  // (set from SOARM_RS_FORCE11 by the launch code)
#define WPH_ADD(k, v) g_wphase[WPH_ID() * WPH + (k)] += (unsigned long long)(v)
#define WPH_MAX(k, v) \
  g_wphase[WPH_ID() * WPH + (k)] = max(g_wphase[WPH_ID() * WPH + (k)], (unsigned long long)(v))
// contact-row build split: [0] loads + frame, [1] Jacobian, [2] Gram / M^-1 / velocities, [3] edges + LDS writes
__device__ long long g_rowprof[65536 * 4];
#define RP_INIT long long rp_acc[4] = {0, 0, 0, 0}, rp_t = clock64()
#define RP_MARK(k)                  \
  {                                 \
    const long long t_ = clock64(); \
    rp_acc[k] += t_ - rp_t;         \
    rp_t = t_;                      \
  }
#define RP_STORE \
  if (e < 65536) g_rowprof[4 * e] = rp_acc[0], g_rowprof[4 * e + 1] = rp_acc[1], g_rowprof[4 * e + 2] = rp_acc[2], g_rowprof[4 * e + 3] = rp_acc[3]

// Newton (soarm_newton.h): [0] solves (one lane per env), [1] sum of iterations, [2] sum of line-search
// evaluations, [3] solves on the coupled (whole-problem) path, [4] sum of solve cycles, [5] max
// solve cycles, [6] max iterations, [7] max line-search evaluations of one solve; split solves
// (per env): [8] arm iterations, [9] arm evaluations, [10] free-body iterations, [11] free-body
// evaluations; per wave: [12] waves, [13] sum over waves of the wave's max evaluations, [14] of
// its max iterations, [15] sum of the wave's max solve cycles; per env (sum over both ranges):
// [16] warm-start cycles, [17] Hessian + factor + solve cycles, [18] line-search cycles,
// [19] cycles of the pass at the new point, [20] wave-max sum of [16], [21] of [17], [22] of [18],
// [23] of [19]
__device__ unsigned long long g_newton[24];
#define NT_STAMP(k)                          \
  {                                          \
    const long long t_ = clock64();          \
    ncyc[k] += t_ - nt_;                     \
    nt_ = t_;                                \
  }
DEVI int wave_max_i(int v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// the close of newton_solve's profile; one: this lane counts for its env
DEVI void prof_newton_end(long long t0, bool one, int it, int nls, bool coupled, int it_arm, int nls_arm,
                          const long long (&ncyc)[4]) {
  // reduced over the wave first (one lane per env counts), then one atomic per counter and
  // wave: per-env atomics on shared counters serialise in L2 and stall the waves being measured
  const long long dt = clock64() - t0;
  auto wsum = [](double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
  };
  const double sv[16] = {1.0, (double)it, (double)nls, (double)coupled, (double)dt, (double)it_arm,
                         (double)nls_arm, (double)(it - it_arm), (double)(nls - nls_arm),
                         (double)ncyc[0], (double)ncyc[1], (double)ncyc[2], (double)ncyc[3], 0.0, 0.0, 0.0};
  const int sk[13] = {0, 1, 2, 3, 4, 8, 9, 10, 11, 16, 17, 18, 19};
  for (int k = 0; k < 13; k++) {
    const double w = wsum(one ? sv[k] : 0.0);
    if ((threadIdx.x & 63) == 0) atomicAdd(&g_newton[sk[k]], (unsigned long long)w);
  }
  const int mx[4] = {wave_max_i((int)dt), wave_max_i(it), wave_max_i(nls), 0};
  const int wc[4] = {wave_max_i((int)ncyc[0]), wave_max_i((int)ncyc[1]), wave_max_i((int)ncyc[2]),
                     wave_max_i((int)ncyc[3])};
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&g_newton[5], (unsigned long long)mx[0]);
    atomicMax(&g_newton[6], (unsigned long long)mx[1]);
    atomicMax(&g_newton[7], (unsigned long long)mx[2]);
    atomicAdd(&g_newton[12], 1ull);
    atomicAdd(&g_newton[13], (unsigned long long)mx[2]);
    atomicAdd(&g_newton[14], (unsigned long long)mx[1]);
    atomicAdd(&g_newton[15], (unsigned long long)mx[0]);
    for (int k = 0; k < 4; k++) atomicAdd(&g_newton[20 + k], (unsigned long long)wc[k]);
  }
}

// the RS solve's split: [77] setup (from the sweeps' start stamp to rp0), [78] sweeps, [79] final
// qacc, summed over waves; [80] waves; [81] sum of wave sweeps
DEVI void prof_rs_split(int e, long long rp0, long long rp1, int wsw) {
  if ((threadIdx.x & 63) == 0 && WPH_ID() < WPH_MAXW) {
    const long long rp2 = clock64();
    WPH_ADD(77, rp0 - g_pgs_prof[8 * e]);
    WPH_ADD(78, rp1 - rp0);
    WPH_ADD(79, rp2 - rp1);
    WPH_ADD(80, 1);
    WPH_ADD(81, wsw);
  }
}

// the close of k_substep's profile: the wave's row of g_wphase from the env's stamps; t0..t5 are
// the kernel's PHASE_T marks, lds_con = LDS_CON
DEVI void prof_substep_end(int e, long long t0, long long t1, long long t2, long long t5, int lds_con) {
  const long long p0 = g_pgs_prof[8 * e], p1 = g_pgs_prof[8 * e + 1];
  const int nsw = (int)g_pgs_prof[8 * e + 2];
  const bool anylim = __any(g_pgs_prof[8 * e + 4] > 0), anyslow = __any(g_pgs_prof[8 * e + 3] == 0),
             anyovf = __any(g_pgs_prof[8 * e + 5] > lds_con), anyfree = __any(g_pgs_prof[8 * e + 3] & 16);
  // (wave reductions first: one row per wave in g_wphase, no shared-address atomics)
  auto wsum = [](int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
  };
  int wmax = nsw, cmax = (int)g_pgs_prof[8 * e + 5];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wmax = max(wmax, __shfl_xor(wmax, o)), cmax = max(cmax, __shfl_xor(cmax, o));
  // per-lane census of lanes in waves on a non-y sweep: [43..46] npost 0..3+, [47..49] extras on
  // the free body 0/1/2+, [50] > 5 contacts, [51] active limit, [52] overflow rows
  const long long cv = g_pgs_prof[8 * e + 3];
  const bool ny = (cv & 15) >= 2;
  int census[10];
#pragma unroll
  for (int k = 0; k < 4; k++) census[k] = wsum(ny && ((cv >> 8) & 3) == k);
#pragma unroll
  for (int k = 0; k < 3; k++) census[4 + k] = wsum(ny && min((int)((cv >> 12) & 3), 2) == k);
  census[7] = wsum(ny && ((cv >> 16) & 1)), census[8] = wsum(ny && ((cv >> 17) & 1)),
  census[9] = wsum(ny && ((cv >> 18) & 1));
  const int nsw_sum = wsum(nsw), lanes = wsum(1);
  int why[7];
#pragma unroll
  for (int k = 0; k < 7; k++) why[k] = wsum((int)((cv >> (41 + k)) & 1));
  if ((threadIdx.x & 63) == 0 && WPH_ID() < WPH_MAXW) {
    WPH_MAX(15, cmax);
    WPH_ADD(6, nsw_sum);
    WPH_ADD(7, lanes);
#pragma unroll
    for (int k = 0; k < 10; k++) WPH_ADD(43 + k, census[k]);
    WPH_ADD(0, t1 - t0);
    WPH_ADD(1, t2 - t1);
    WPH_ADD(2, p0 - t2);
    WPH_ADD(3, p1 - p0);
    WPH_ADD(4, t5 - p1);
    WPH_MAX(8, t5 - t0);
    {
      int var = (int)g_pgs_prof[8 * e + 3] & 15;
      WPH_ADD(9, var == 0);
      WPH_ADD(19 + var, 1);
      WPH_MAX(23 + var, t5 - t0);
    }
    WPH_ADD(27, anyfree);
    for (int k = 0; k < 15; k++) WPH_ADD(28 + k, g_stamp[16 * e + k + 1] - g_stamp[16 * e + k]);
    for (int k = 0; k < 4; k++) WPH_ADD(53 + k, g_rowprof[4 * e + k]);
    WPH_ADD(16, g_pgs_prof[8 * e + 6] - t2);
    WPH_ADD(17, g_pgs_prof[8 * e + 7] - g_pgs_prof[8 * e + 6]);
    WPH_ADD(18, p0 - g_pgs_prof[8 * e + 7]);
    WPH_ADD(12, anylim);
    WPH_ADD(13, anyslow);
    WPH_ADD(14, anyovf);
    WPH_MAX(10, p1 - p0);
    WPH_ADD(11, wmax);
    WPH_ADD(5, 1);
    if ((cv >> 40) & 1) {
      WPH_ADD(82, 1), WPH_MAX(83, t5 - t0), WPH_ADD(84, t5 - t0);
#pragma unroll
      for (int k = 0; k < 7; k++) WPH_ADD(85 + k, why[k]);
    }
    const int ast = (int)((g_pgs_prof[8 * e + 3] >> 20) & 255);
    if (ast) WPH_ADD(57, 1), WPH_ADD(58, ast);
    WPH_MAX(ast ? 60 : 59, t5 - t0);
    const int xv = (int)((g_pgs_prof[8 * e + 3] >> 28) & 7);
    if (xv >= 4) {
      WPH_ADD(61 + xv - 4, 1);
      WPH_MAX(65 + xv - 4, t5 - t0);
      WPH_ADD(69 + xv - 4, p1 - p0);
      WPH_ADD(73 + xv - 4, ast);
    }
  }
}
#else
constexpr bool PHASE_PROF = false;
#define PROF_DECL(...)
#define PROF_DO(...)
#define PHASE_T(v)
#define PSTAMP(k)
#define RP_INIT
#define RP_MARK(k)
#define RP_STORE
#define NT_STAMP(k)
#endif

}  // namespace soarm
