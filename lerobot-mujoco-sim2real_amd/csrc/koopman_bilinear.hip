// koopman_bilinear.hip — the control step of the bilinear DBKN model (include/koopman_mpc.h:
// sim_koopman_set_bilinear, sim_koopman_bilinear_step, sim_koopman_set_bilinear_box,
// sim_koopman_bilinear_box_step): one condensed QP per env and frame, one wave per env, float64.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "koopman_internal.h"

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------- DBKN (bilinear) first move
// The bilinear model's input matrix depends on the lifted state: B_total = B + sum_j z0_j Hhat_j
// (linearize_B, MPC_Controler.py:46-63), so the condensed QP (MPC_Controler.py:100-141, state_full:
// Q = q I, R = r I) differs per env and frame.  One wave per env, float64, everything in LDS:
//   M_0 = B_total, M_k = A M_{k-1}; X_k = M_k ('mpc') or C_k = sum_{i<=k} M_i ('delta_mpc')
//     (A staged in LDS once per workgroup);
//   rhs[s] = q sum_{t >= s} X_{t-s}' e_t, e_t = ref_t - A^{t+1} z0 - [delta] C_t u_prev;
//   G = Xs' Xs, the Gram of the stacked X_k (N = H nu columns, nz rows) on the f64 MFMA, in
//     registers until every X_k is read, then stored packed lower over X's storage;
//   Hess[s1][s2] = q sum_{t >= max(s1,s2)} X_{t-s1}' X_{t-s2} + r I -- along each block diagonal
//     a prefix sum of G's blocks: with the block order reversed, flip(s nu + c) = (H-1-s) nu + c,
//     Hess[flip a][flip b] = q sum_{b' <= b} G[b' + a - b][b'] (blocks a >= b), so the prefix sums
//     overwrite G in place (one lane per block diagonal and (c1, c2)) and leave
//     P = Pi Hess Pi' packed lower, Pi the block reversal;
//   P v' = Pi rhs by a Cholesky with the rows in registers, a forward solve and the first nu steps
//   of the back substitution (pivots by readlane): v_0 = v'_{(H-1) nu + c} comes first there;
//   u0 = v_0 + u_prev, action = clip(u0).
// Shapes: nz <= 64, nu <= 8, N = H nu <= 64.  Per env LDS: the X region (X [H][xs], later G
// and P) and the M region (M [nz*nu] and Zs [H+1][nz], later Y [N][H], then the Cholesky's column
// buffer; >= 256 doubles): 17.3 KB at nz 32, nu 5, H 10; up to 8 envs (waves) per workgroup, or as
// many as the LDS holds with A [nz][nz].  The plan is BDev (koopman_internal.h), from set_bilinear.

// a double of lane l (l wave-uniform) in every lane: two v_readlane
DEVI double rdlane(double x, int l) {
  const long long b = __double_as_longlong(x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffff), l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// sum_j x[j * sx] y[j], j < len: four independent FMA chains (the loads of a step do not wait for
// the previous step's FMA)
DEVI double dotn(const double* x, int sx, const double* y, int len) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int j = 0;
#pragma unroll 2
  for (; j + 4 <= len; j += 4) {
    s0 = fma(x[j * sx], y[j], s0);
    s1 = fma(x[(j + 1) * sx], y[j + 1], s1);
    s2 = fma(x[(j + 2) * sx], y[j + 2], s2);
    s3 = fma(x[(j + 3) * sx], y[j + 3], s3);
  }
  for (; j < len; j++) s0 = fma(x[j * sx], y[j], s0);
  return (s0 + s1) + (s2 + s3);
}
#ifdef SOARM_BL_PROF
// diagnostic build: per phase of k_bilinear, summed wave cycles ([0..7]) and waves ([8])
__device__ unsigned long long g_bl[9];
#define BL_STAMP(k)                                                                  \
  {                                                                                  \
    const long long t_ = clock64();                                                  \
    if ((k) > 0 && lane == 0) atomicAdd(&g_bl[(k) - 1], (unsigned long long)(t_ - bl_t)); \
    if ((k) == 8 && lane == 0) atomicAdd(&g_bl[8], 1ull);                            \
    bl_t = t_;                                                                       \
  }
#else
#define BL_STAMP(k)
#endif
// HS / NUS / NZS: a static horizon, input count and lifted dimension (0: read from K) -- the
// reference's configuration (horizon 10, u_dim 5, nz = 8 + 24 = 32: N = 50) gets an instantiation in
// which every loop bound and guard on N, nu, H and nz is a constant (the Cholesky's and the solves'
// unrolled loops lose their per-column branches)
//
// BOX (k_bilinear_box, sim_koopman_bilinear_box_step): the same QP with the input limit in it, in the
// model inputs w [N] (include/koopman_mpc.h):  min 1/2 w'P w - g'w,  lo <= w <= hi.  In w the state
// term of both kinds is the 'mpc' form (X_k = M_k); 'delta_mpc' differs in the input term, r D'D (D the
// block first difference: 2r on the diagonal blocks, r on the last one, -r beside them), and in the
// right-hand side: no C_t u_prev in e_t, and r u_prev added on block 0.  The phases up to the packed
// P = Pi Hess Pi' are shared; the Cholesky and the solves are replaced by projected Gauss-Seidel in
// registers, one lane per row:
//   lane i holds row i of P (both triangles, read once from the packed LDS copy), w_i, lo_i, hi_i,
//   1 / P_ii and the running gradient r_i = (P w - g)_i;
//   step i of a sweep: every lane forms clip(w - r / P_ii) - w, lane i's value is broadcast by
//   readlane, lane i takes its clipped value, every lane does r += P[.][i] delta -- no dot product and
//   no LDS traffic in the sweep, monotone descent, no tuning parameter.  The sweep runs over the lanes
//   in order, i.e. over the time blocks from the last to the first (the reversed order Pi).
//   Start: w = clip(0).  There is no factorisation in this kernel, so an env whose unconstrained
//   minimiser lies inside the box is iterated like every other one: it gets iters > 0 and is solved to
//   tol (the DKUC step returns such an env with iters = 0).
//   Stop test, after EVERY sweep: res = w - clip(w - r / Lhat, lo, hi) from the maintained gradient,
//   Lhat = ||P||_inf of this env (a lane's absolute row sum, then the wave maximum); done when
//   ||res||_inf <= tol.  iters counts sweeps; at max_iter: ok = 0, iters = max_iter, the last iterate
//   (every entry is a projection: inside the box).
struct BXDev {
  double umax, tol;
  int max_iter;
  double* plan;  // [H][nu][n] or null
  int* ok;       // [n] or null
  int* iters;    // [n] or null
};
constexpr int BBOX_MAX_ITER = 128;  // default (twice the measured maximum, rounded up)

template <int EPW, int HS, int NUS, int NZS, bool BOX>
DEVI void bilinear_body(double* lds, const BDev& K, const BXDev& bx, const double* __restrict__ A,
                        const double* __restrict__ Bm, const double* __restrict__ Hh, int n,
                        const double* __restrict__ z0g, const double* __restrict__ win,
                        double* __restrict__ uprev, float* __restrict__ action) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // XCD-aware chunking: workgroups are dealt round-robin over the 8 XCDs, so chunk the envs per
  // XCD (workgroup b runs chunk (b % 8) G/8 + b / 8): neighbouring envs -- which share the cache
  // lines of z0 and of the [H][nz][n] window -- land in the same L2
  const int nwg = gridDim.x;
  const int b = (nwg & 7) ? (int)blockIdx.x : ((int)blockIdx.x & 7) * (nwg >> 3) + ((int)blockIdx.x >> 3);
  const int e = b * EPW + w;
#ifdef SOARM_BL_PROF
  long long bl_t = 0;
#endif
  const int nz = NZS ? NZS : K.nz, nu = NUS ? NUS : K.nu, H = HS ? HS : K.H, N = (HS && NUS) ? HS * NUS : K.N;
  const int zu = nz * nu, xs = K.xs;
  // A, shared by the workgroup's envs, rows padded to an odd stride (nz + 1 doubles): lanes reading
  // one element of different rows hit different banks (a 256-B stride puts them all on one)
  const int as = nz + 1;
  double* As = lds + (size_t)EPW * K.per_env;
  for (int i = threadIdx.x; i < nz * nz; i += blockDim.x) As[(i / nz) * as + (i % nz)] = A[i];
  __syncthreads();
  if (e >= n) return;  // (whole waves: no workgroup barrier below)
  BL_STAMP(0);
  double* X = lds + (size_t)w * K.per_env;  // [H][xs]; later G and P, packed lower (N (N + 1) / 2)
  double* M = X + K.xreg;                   // [zu]; later Y, then the Cholesky's column buffer
  double* Zs = M + zu;                      // [H + 1][nz]: A^t z0 (t = 0..H), later e_t over row t + 1
  for (int i = lane; i < nz; i += 64) Zs[i] = z0g[(size_t)i * n + e];
  double up[8];
#pragma unroll
  for (int c = 0; c < 8; c++) up[c] = c < nu ? uprev[(size_t)c * n + e] : 0.0;
  wsync();
  // B_total = B + sum_j z0_j Hhat_j  (Hhat [j][(i nu + c)]: a load instruction reads 64
  // consecutive doubles); for nz <= 32 all of an output's loads are issued before its FMAs (the
  // same four chains, in the same order, as dotn)
  for (int o = lane; o < zu; o += 64) {
    const double* hr = Hh + o;
    double d;
    if (nz <= 32) {
      double h[32];
#pragma unroll
      for (int j = 0; j < 32; j++) h[j] = hr[(size_t)min(j, nz - 1) * zu];
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
      for (int j = 0; j < 32; j += 4)
        if (j + 4 <= nz) {
          s0 = fma(h[j], Zs[j], s0);
          s1 = fma(h[j + 1], Zs[j + 1], s1);
          s2 = fma(h[j + 2], Zs[j + 2], s2);
          s3 = fma(h[j + 3], Zs[j + 3], s3);
        }
#pragma unroll
      for (int j = 0; j < 32; j++)
        if (j >= (nz & ~3) && j < nz) s0 = fma(h[j], Zs[j], s0);
      d = (s0 + s1) + (s2 + s3);
    } else {
      d = dotn(hr, zu, Zs, nz);
    }
    const double s = Bm[o] + d;
    M[o] = s, X[o] = s;
  }
  wsync();
  // the reference window of the first 16 frames (lane < nz; clamped addresses, no guarded loads),
  // issued after B_total's loads so that its latency overlaps the M_k phase (no global loads there:
  // the load counter is waited on in order)
  double wv[16];
  {
    const int li = min(lane, nz - 1);
#pragma unroll
    for (int t = 0; t < 16; t++) wv[t] = win[((size_t)min(t, H - 1) * nz + li) * n + e];
  }
  BL_STAMP(1);
  // M_k = A M_{k-1}; X_k = M_k or X_{k-1} + M_k, on the f64 MFMA: A's 16-row tiles (A fragment:
  // lane l holds A[16 t + (l & 15)][4 ks + (l >> 4)]) times M_{k-1} padded to 16 columns (B: lane l
  // holds M[4 ks + (l >> 4)][l & 15]); C: lane l, register r = row 16 t + (l >> 4) + 4 r, column l & 15.
  // Column nu of the B operand carries A^{k-1} z0, so the same products give the free response
  // A^k z0 (k = 1..H; the last round computes only that column).
  {
    const int NTz = (nz + 15) >> 4, KSz = (nz + 3) >> 2, fr = lane >> 4, fc = lane & 15;
    // A's fragments for nz <= 32 (2 row tiles x 8 k-steps) stay in registers across the H steps
    double af[2][8];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int ks = 0; ks < 8; ks++) {
        const int ar = 16 * t + fc, jr = 4 * ks + fr;
        af[t][ks] = (ar < nz && jr < nz) ? As[ar * as + jr] : 0.0;
      }
    const double* zc = Zs;  // A^{k-1} z0
    auto bop = [&](int jr) {  // B operand of row jr (lane column fc)
      return jr < nz ? (fc < nu ? M[jr * nu + fc] : (fc == nu ? zc[jr] : 0.0)) : 0.0;
    };
    for (int k = 1; k <= H; k++) {
      d4 acc[4];
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
      if (nz <= 32) {
        double bm[8];
#pragma unroll
        for (int ks = 0; ks < 8; ks++) bm[ks] = bop(4 * ks + fr);
#pragma unroll
        for (int ks = 0; ks < 8; ks++) {
          acc[0] = mfma(af[0][ks], bm[ks], acc[0]);
          if (NTz > 1) acc[1] = mfma(af[1][ks], bm[ks], acc[1]);
        }
      } else {
        for (int ks = 0; ks < KSz; ks++) {
          const int jr = 4 * ks + fr;
          const double bm = bop(jr);
#pragma unroll
          for (int t = 0; t < 4; t++) {
            const int ar = 16 * t + fc;
            if (t < NTz) acc[t] = mfma((ar < nz && jr < nz) ? As[ar * as + jr] : 0.0, bm, acc[t]);
          }
        }
      }
      wsync();  // (every lane has read M_{k-1})
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = 16 * t + fr + 4 * r, o = row * nu + fc;
          if (t < NTz && row < nz) {
            if (fc < nu && k < H) {
              M[o] = acc[t][r];
              X[k * xs + o] = (K.delta && !BOX) ? X[(k - 1) * xs + o] + acc[t][r] : acc[t][r];
            } else if (fc == nu) {
              Zs[k * nz + row] = acc[t][r];
            }
          }
        }
      zc = Zs + k * nz;
      wsync();
    }
  }
  BL_STAMP(2);
  // e_t = ref_t - A^{t+1} z0 - [delta] C_t u_prev (lane i < nz), in place over row t + 1 of Zs
  if (lane < nz) {
#pragma unroll 2
    for (int t = 0; t < H; t++) {
      double wt = 0.0;
#pragma unroll
      for (int s2 = 0; s2 < 16; s2++) wt = s2 == t ? wv[s2] : wt;
      if (t >= 16) wt = win[((size_t)t * nz + lane) * n + e];
      double ev = wt - Zs[(t + 1) * nz + lane];
      if (K.delta && !BOX) {
#pragma unroll
        for (int c = 0; c < 8; c++)
          if (c < nu) ev = fma(-X[t * xs + lane * nu + c], up[c], ev);
      }
      Zs[(t + 1) * nz + lane] = ev;
    }
  }
  wsync();
  // rhs in the reversed order (lane a holds entry flip(a) = s nu + c, s = H-1 - a / nu):
  // rhs[s] = q sum_{t >= s} X_{t-s}' e_t.  For H <= 16 from Y = Xs' E (the Gram's MFMA loop below,
  // N x H); otherwise here, one dot product per (lane, t).
  double rhs = 0.0;
  const int ls = H - 1 - lane / nu, lc = lane % nu;
  if (H > 16 && lane < N) {
    for (int t = ls; t < H; t++) rhs = fma(K.q, dotn(X + (t - ls) * xs + lc, nu, Zs + (t + 1) * nz, nz), rhs);
  }
  BL_STAMP(3);
  // Gram G[a][b] = sum_i X[i][a] X[i][b] over the N = H nu columns a = k nu + c of the stacked X_k
  // (rows i < nz), on the f64 MFMA: the A fragment of (tile t, k-step ks) -- lane l holds
  // X[4 ks + (l >> 4)][16 t + (l & 15)] -- is also the B fragment of (t, ks), so 4 fragment loads
  // per k-step feed the <= 10 lower tiles (ta >= tb); C: lane l, register r = row (l >> 4) + 4 r,
  // column l & 15 of the tile.  Stored packed lower (row >= col) over X, once every lane has read X.
  double* G = X;
  {
    const int NT = (N + 15) >> 4, KS = (nz + 3) >> 2;
    const bool yk = H <= 16;  // Y = Xs' E here (B operand: lane l holds e_{l & 15}[4 ks + (l >> 4)])
    d4 acc[10], yacc[4];
#pragma unroll
    for (int q = 0; q < 10; q++) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; q++) yacc[q] = d4{0.0, 0.0, 0.0, 0.0};
    const int fr = lane >> 4, fc = lane & 15;
    for (int ks = 0; ks < KS; ks++) {
      double fg[4];
      const int i = 4 * ks + fr;
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int a = 16 * t + fc, k = a / nu;
        fg[t] = (t < NT && a < N && i < nz) ? X[k * xs + i * nu + (a - k * nu)] : 0.0;
      }
#pragma unroll
      for (int ta = 0, q = 0; ta < 4; ta++)
#pragma unroll
        for (int tb = 0; tb <= ta; tb++, q++)
          if (ta < NT) acc[q] = mfma(fg[ta], fg[tb], acc[q]);
      if (yk) {
        const double eo = (fc < H && i < nz) ? Zs[(fc + 1) * nz + i] : 0.0;
#pragma unroll
        for (int ta = 0; ta < 4; ta++)
          if (ta < NT) yacc[ta] = mfma(fg[ta], eo, yacc[ta]);
      }
    }
    wsync();
    if (yk) {  // Y [a][t] over M's storage (M and E are dead), then each lane's diagonal sum
      double* Y = M;
#pragma unroll
      for (int ta = 0; ta < 4; ta++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int a = 16 * ta + fr + 4 * r;
          if (ta < NT && a < N && fc < H) Y[a * H + fc] = yacc[ta][r];
        }
      wsync();
      if (lane < N)
        for (int t = ls; t < H; t++) rhs = fma(K.q, Y[((t - ls) * nu + lc) * H + t], rhs);
    }
#pragma unroll
    for (int ta = 0, q = 0; ta < 4; ta++)
#pragma unroll
      for (int tb = 0; tb <= ta; tb++, q++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = 16 * ta + fr + 4 * r, col = 16 * tb + fc;
          if (ta < NT && row < N && col <= row) G[row * (row + 1) / 2 + col] = acc[q][r];
        }
  }
  wsync();
  BL_STAMP(4);
  // P = Pi Hess Pi' in place over G: lane (d, c1, c2) walks its block diagonal's entries
  // (a1, a2) = ((b + d) nu + c1, b nu + c2), b = 0, 1, ... (a1 >= a2: d > 0, or c1 >= c2), keeps the
  // running sum S of G there and writes q S + r [d = 0, c1 = c2] back.  Every entry has one owner.
  double* P = G;
  for (int tr = lane; tr < H * nu * nu; tr += 64) {
    const int d = tr / (nu * nu), c1 = (tr / nu) % nu, c2 = tr % nu;
    if (d == 0 && c1 < c2) continue;  // (upper triangle of a diagonal block: not stored)
    const double rd = (d == 0 && c1 == c2) ? K.r : 0.0;
    double S = 0.0;
    for (int b = 0; b + d < H; b++) {
      const int a1 = (b + d) * nu + c1, a2 = b * nu + c2, o = a1 * (a1 + 1) / 2 + a2;
      S += G[o];
      if constexpr (BOX) {  // 'delta_mpc': r D'D in the reversed order (block b = 0 is the last time block)
        const double rb = !K.delta ? rd : c1 != c2 ? 0.0 : d == 0 ? (b == 0 ? K.r : 2.0 * K.r) : d == 1 ? -K.r : 0.0;
        P[o] = fma(K.q, S, rb);
      } else {
        P[o] = fma(K.q, S, rd);
      }
    }
  }
  wsync();
  BL_STAMP(5);
  if constexpr (BOX) {
    // the plan's own entry of lane a: time block ls, input lc (above); u_prev of that input
    double upl = 0.0;
#pragma unroll
    for (int c = 0; c < 8; c++) upl = lc == c ? up[c] : upl;
    const bool live = lane < N;
    if (K.delta && live && ls == 0) rhs = fma(K.r, upl, rhs);
    double lo = live ? -bx.umax : 0.0, hi = live ? bx.umax : 0.0;
    if (!K.delta && live && ls == 0) lo -= upl, hi -= upl;  // |v_0 + u_prev| <= u_max: what is applied
    // row `lane` of P, both triangles (lanes >= N and columns >= N: zero)
    double prow[64];
#pragma unroll
    for (int k = 0; k < 64; k++) {
      const int hi_i = max(lane, k), lo_i = min(lane, k);
      prow[k] = (live && k < N) ? P[hi_i * (hi_i + 1) / 2 + lo_i] : 0.0;
    }
    const double idg = live ? 1.0 / P[lane * (lane + 1) / 2 + lane] : 0.0;
    double lh = 0.0;
#pragma unroll
    for (int k = 0; k < 64; k++) lh += fabs(prow[k]);
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) lh = fmax(lh, __shfl_xor(lh, s));
    const double ilh = 1.0 / lh;
    // start: w = clip(0), gradient r = P w - g
    double wl = clipd(0.0, lo, hi);
    double gr = -rhs;
#pragma unroll
    for (int k = 0; k < 64; k++)
      if (k < N) gr = fma(prow[k], rdlane(wl, k), gr);
    int it = 0, done = 0;
    while (it < bx.max_iter) {
      it++;
#pragma unroll
      for (int i = 0; i < 64; i++)
        if (i < N) {
          const double wn = clipd(fma(-gr, idg, wl), lo, hi);
          const double di = rdlane(wn - wl, i);
          if (lane == i) wl = wn;
          gr = fma(prow[i], di, gr);
        }
      double res = fabs(wl - clipd(fma(-gr, ilh, wl), lo, hi));
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) res = fmax(res, __shfl_xor(res, s));
      if (rdlane(res, 0) <= bx.tol) {
        done = 1;
        break;
      }
    }
    if (live) {
      if (bx.plan) bx.plan[((size_t)ls * nu + lc) * n + e] = wl;
      if (ls == 0) {  // u0 = w_0 ('delta_mpc') or v_0 + u_prev (the sum may round one ulp past the limit)
        const double u0 = K.delta ? wl : clipd(wl + upl, -bx.umax, bx.umax);
        uprev[(size_t)lc * n + e] = u0;
        action[(size_t)e * nu + lc] = (float)u0;
      }
    }
    if (lane == 0) {
      if (bx.ok) bx.ok[e] = done;
      if (bx.iters) bx.iters[e] = it;
    }
    return;
  }
  // Cholesky P = L L' with the rows in registers: lane i holds row i (compile-time column index,
  // N <= 64), in blocks of 4 columns.  Inside a block, column j is updated by the block's earlier
  // columns with L[j][q] taken by readlane (uniform), then scaled by its pivot; the trailing
  // columns k >= jb + 4 are updated once per block from the 4 columns put in LDS (M's storage),
  // read as same-address broadcasts.  Every row entry sees the same FMAs in the same column order
  // as the column-by-column right-looking form.  Pivots: 1/sqrt(d) from v_rsq_f64 and two Newton
  // steps, L[j][j] = d / sqrt(d) by that.  Lane l keeps 1 / L[l][l].  (The entries right of a
  // lane's diagonal take junk updates and are never read.)
  double row[64];
#pragma unroll
  for (int k = 0; k < 64; k++) row[k] = (lane < N && k <= lane) ? P[lane * (lane + 1) / 2 + k] : 0.0;
  double idg = 0.0;
  double* colb = M;  // [64][4] (>= 256 doubles: M is dead once X is complete)
#pragma unroll
  for (int jb = 0; jb < 64; jb += 4) {
    if (jb < N) {
      double l[4];
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const int j = jb + m;
        l[m] = 0.0;
        if (j < N) {
          double v = row[j];
#pragma unroll
          for (int q = 0; q < m; q++) v = fma(-l[q], rdlane(l[q], j), v);
          const double dj = rdlane(v, j);
          double y = __builtin_amdgcn_rsq(dj);
          y = fma(0.5 * y, fma(-(dj * y), y, 1.0), y);
          y = fma(0.5 * y, fma(-(dj * y), y, 1.0), y);
          l[m] = lane > j ? v * y : (lane == j ? dj * y : 0.0);
          row[j] = l[m];
          if (lane == j) idg = y;
        }
      }
      if (jb + 4 < N) {
        *(d2*)(colb + 4 * lane) = d2{l[0], l[1]};
        *(d2*)(colb + 4 * lane + 2) = d2{l[2], l[3]};
        wsync();
#pragma unroll
        for (int k = jb + 4; k < 64; k++)
          if (k < N) {
            const d2 c01 = *(const d2*)(colb + 4 * k), c23 = *(const d2*)(colb + 4 * k + 2);
            double v = fma(-l[0], c01[0], row[k]);
            v = fma(-l[1], c01[1], v);
            v = fma(-l[2], c23[0], v);
            row[k] = fma(-l[3], c23[1], v);
          }
        wsync();
      }
    }
  }
  BL_STAMP(6);
  // L y = rhs from the register rows; then L' v' = y, of which only v'_a, a >= N - nu, is wanted
  // (u0's entries, in the reversed order): those are the back substitution's first nu steps, so
  // only rows a >= N - nu of L go back to LDS (lane i reads row j's entry i, contiguous over the
  // lanes).  Pivot values by readlane.
  double y = rhs;
#pragma unroll
  for (int j = 0; j < 64; j++) {
    if (j < N) {
      const double yj = rdlane(y, j) * rdlane(idg, j);
      if (lane == j) y = yj;
      if (lane > j && lane < N) y = fma(-row[j], yj, y);
    }
  }
  const int a0 = N - nu;
#pragma unroll
  for (int k = 0; k < 64; k++)
    if (lane < N && k <= lane && k >= a0) P[lane * (lane + 1) / 2 + k] = row[k];
  wsync();
  for (int j = N - 1; j >= a0; j--) {
    const double vj = rdlane(y, j) * rdlane(idg, j);
    if (lane == j) y = vj;
    if (lane >= a0 && lane < j) y = fma(-P[j * (j + 1) / 2 + lane], vj, y);
  }
  BL_STAMP(7);
  const int c0 = lane - a0;  // v_0's entry c sits in lane flip(c) = (H-1) nu + c
  if (c0 >= 0 && c0 < nu) {  // u0 = v_0 + u_prev (get_control, MPC_Controler.py:147-149)
    double upl = 0.0;
#pragma unroll
    for (int c = 0; c < 8; c++) upl = c0 == c ? up[c] : upl;
    const double u0 = y + upl;
    uprev[(size_t)c0 * n + e] = u0;
    action[(size_t)e * nu + c0] = (float)fmin(fmax(u0, -K.uclip), K.uclip);
  }
  BL_STAMP(8);
}

template <int EPW, int HS = 0, int NUS = 0, int NZS = 0>
__global__ __launch_bounds__(64 * EPW) void k_bilinear(BDev K, const double* __restrict__ A,
                                                          const double* __restrict__ Bm,
                                                          const double* __restrict__ Hh, int n,
                                                          const double* __restrict__ z0g,
                                                          const double* __restrict__ win,
                                                          double* __restrict__ uprev, float* __restrict__ action) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  bilinear_body<EPW, HS, NUS, NZS, false>(lds, K, BXDev{}, A, Bm, Hh, n, z0g, win, uprev, action);
}

template <int EPW, int HS = 0, int NUS = 0, int NZS = 0>
__global__ __launch_bounds__(64 * EPW) void k_bilinear_box(BDev K, BXDev bx, const double* __restrict__ A,
                                                              const double* __restrict__ Bm,
                                                              const double* __restrict__ Hh, int n,
                                                              const double* __restrict__ z0g,
                                                              const double* __restrict__ win,
                                                              double* __restrict__ uprev,
                                                              float* __restrict__ action) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  bilinear_body<EPW, HS, NUS, NZS, true>(lds, K, bx, A, Bm, Hh, n, z0g, win, uprev, action);
}

// The kernels by (BOX, slot): slots 0..4 are the envs per workgroup EPWS, slot 5 the static shapes
// of the reference (horizon 10, u_dim 5, nz 32 at 8 envs per workgroup)
constexpr int EPWS[5] = {8, 6, 4, 2, 1};
constexpr int NSLOT = 6;
const void* const BILINEAR[2][NSLOT] = {
    {(const void*)k_bilinear<8>, (const void*)k_bilinear<6>, (const void*)k_bilinear<4>, (const void*)k_bilinear<2>,
     (const void*)k_bilinear<1>, (const void*)k_bilinear<8, 10, 5, 32>},
    {(const void*)k_bilinear_box<8>, (const void*)k_bilinear_box<6>, (const void*)k_bilinear_box<4>,
     (const void*)k_bilinear_box<2>, (const void*)k_bilinear_box<1>, (const void*)k_bilinear_box<8, 10, 5, 32>}};

int slot_of(const BDev& b) {
  if (b.H == 10 && b.nu == 5 && b.nz == 32 && b.epw == 8) return 5;
  return (int)(std::find(EPWS, EPWS + 5, b.epw) - EPWS);
}

// dynamic LDS of a workgroup: its envs' regions, then A with its rows padded to nz + 1
size_t lds_bytes(const BDev& b) { return ((size_t)b.per_env * b.epw + (size_t)b.nz * (b.nz + 1)) * sizeof(double); }

int raise_lds(bool box) {
  for (const void* f : BILINEAR[box]) KCHECK(koopman_raise_lds(f));
  return SIM_OK;
}

// one step of n envs; bx: the box step's arguments (k_bilinear_box), null for k_bilinear
int launch(sim_koopman* k, BXDev* bx, int n, const double* z0, const double* window, double* u_prev, float* action,
           void* stream) {
  void* args[11];
  int na = 0;
  args[na++] = &k->bd;
  if (bx) args[na++] = bx;
  for (void* a : {(void*)&k->d_A, (void*)&k->d_B, (void*)&k->d_Hh, (void*)&n, (void*)&z0, (void*)&window,
                  (void*)&u_prev, (void*)&action})
    args[na++] = a;
  const int ep = k->bd.epw;
  (void)hipLaunchKernel(BILINEAR[bx != nullptr][slot_of(k->bd)], dim3((n + ep - 1) / ep), dim3(64 * ep), args,
                        lds_bytes(k->bd), (hipStream_t)stream);
  KCHECK(hipGetLastError());
  return SIM_OK;
}

}  // namespace

extern "C" {

#ifdef SOARM_BL_PROF
// diagnostic build only: the k_bilinear phase cycles (9 values), reset after reading
int sim_koopman_bl_profile(double* out) {
  unsigned long long h[9];
  KCHECK(hipDeviceSynchronize());
  KCHECK(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_bl), sizeof(h)));
  for (int k = 0; k < 9; k++) out[k] = (double)h[k];
  const unsigned long long z[9] = {};
  KCHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_bl), z, sizeof(z)));
  return 0;
}
#endif

int sim_koopman_set_bilinear(sim_koopman* k, const double* A, const double* B, const double* Hhat, int delta,
                             double q, double r) {
  if (!k || !A || !B || !Hhat) return soarm_set_error(SIM_E_ARG, "null argument");
  k->bbox = false;  // (the constrained step's options belong to the model they were set for)
  const int nz = k->kd.nz, nu = k->kd.ud, H = k->kd.H, N = H * nu;
  if (nz > 64 || nu > 8 || N > 64) return soarm_set_error(SIM_E_MODEL, "bilinear MPC: nz <= 64, u_dim <= 8, H * u_dim <= 64");
  if (!(q > 0.0) || !(r > 0.0)) return soarm_set_error(SIM_E_ARG, "bilinear MPC: q and r must be positive");
  BDev b{};
  b.nz = nz, b.nu = nu, b.H = H, b.N = N, b.delta = delta ? 1 : 0, b.q = q, b.r = r, b.uclip = k->kd.uclip;
  b.xs = nz * nu + ((nu - nz * nu) % 32 + 32) % 32;
  b.xreg = (std::max(H * b.xs, N * (N + 1) / 2) + 1) & ~1;  // (even: M's column buffer is read as 16-B pairs)
  b.mreg = (std::max(std::max(nz * nu + (H + 1) * nz, N * H), 256) + 1) & ~1;
  b.per_env = b.xreg + b.mreg;
  // as many envs per workgroup as fit the CU's LDS with A (8 at nz 32, nu 5, H 10: 125 KB; the
  // kernel's 215 VGPRs allow 2 waves per SIMD, so 8 is also the register limit)
  for (int ep : EPWS) {
    b.epw = ep;
    if (lds_bytes(b) <= KOOPMAN_LDS_BYTES) break;
    b.epw = 0;
  }
  if (!b.epw) return soarm_set_error(SIM_E_MODEL, "bilinear MPC does not fit in LDS");
  // Hhat [j][i][c] is already the kernel's layout [j][(i nu + c)]
  std::vector<double> hht(Hhat, Hhat + (size_t)nz * nz * nu);
  KCHECK(hipSetDevice(k->device));
  (void)hipFree(k->d_A), (void)hipFree(k->d_B), (void)hipFree(k->d_Hh);
  k->d_A = k->d_B = k->d_Hh = nullptr;
  KCHECK(hipMalloc(&k->d_A, (size_t)nz * nz * 8));
  KCHECK(hipMalloc(&k->d_B, (size_t)nz * nu * 8));
  KCHECK(hipMalloc(&k->d_Hh, hht.size() * 8));
  KCHECK(hipMemcpy(k->d_A, A, (size_t)nz * nz * 8, hipMemcpyHostToDevice));
  KCHECK(hipMemcpy(k->d_B, B, (size_t)nz * nu * 8, hipMemcpyHostToDevice));
  KCHECK(hipMemcpy(k->d_Hh, hht.data(), hht.size() * 8, hipMemcpyHostToDevice));
  if (int rc = raise_lds(false)) return rc;
  k->bd = b;
  return SIM_OK;
}

int sim_koopman_bilinear_step(sim_koopman* k, int n, const double* z0, const double* window, double* u_prev,
                              float* action, void* stream) {
  if (!k || !z0 || !window || !u_prev || !action || n < 0) return soarm_set_error(SIM_E_ARG, "bad argument");
  if (!k->d_A) return soarm_set_error(SIM_E_ARG, "sim_koopman_set_bilinear was not called");
  if (n == 0) return SIM_OK;
  return launch(k, nullptr, n, z0, window, u_prev, action, stream);
}

// The DBKN step with input limits.  k_bilinear_box runs on k_bilinear's LDS plan (the sweep lives in
// registers and needs no LDS of its own) and on fewer registers (no Cholesky rows beside P's), so
// every shape set_bilinear accepts is accepted here: there is no SIM_E_MODEL of its own.
int sim_koopman_set_bilinear_box(sim_koopman* k, const sim_koopman_box_opts* opts) {
  if (!k) return soarm_set_error(SIM_E_ARG, "null argument");
  k->bbox = false;  // a refusal below leaves bilinear_box_step refused and everything else as it was
  if (!k->d_A) return soarm_set_error(SIM_E_ARG, "sim_koopman_set_bilinear was not called");
  if (int rc = koopman_box_check_opts(opts)) return rc;
  const double umax = opts ? opts->u_max : k->bd.uclip;
  if (!(umax > 0.0)) return soarm_set_error(SIM_E_ARG, "box MPC: u_max must be positive");
  KCHECK(hipSetDevice(k->device));
  if (int rc = raise_lds(true)) return rc;
  k->bb_umax = umax, k->bb_tol = opts ? opts->tol : 1e-9, k->bb_max_iter = opts ? opts->max_iter : BBOX_MAX_ITER;
  k->bbox = true;
  return SIM_OK;
}

int sim_koopman_bilinear_box_step(sim_koopman* k, int n, const double* z0, const double* window, double* u_prev,
                                  double* plan, float* action, int32_t* ok, int32_t* iters, void* stream) {
  if (!k || !z0 || !window || !u_prev || !action || n < 0) return soarm_set_error(SIM_E_ARG, "bad argument");
  if (!k->d_A || !k->bbox) return soarm_set_error(SIM_E_ARG, "sim_koopman_set_bilinear_box was not called (or refused)");
  if (n == 0) return SIM_OK;
  BXDev bx{};
  bx.umax = k->bb_umax, bx.tol = k->bb_tol, bx.max_iter = k->bb_max_iter;
  bx.plan = plan, bx.ok = ok, bx.iters = iters;
  return launch(k, &bx, n, z0, window, u_prev, action, stream);
}

}  // extern "C"
