// koopman_train.hip — one training step of the DKUC Koopman model and of the bilinear DBKN one
// (include/koopman_mpc.h sim_koopman_trainer_*, sim_koopman_loss_grad, sim_koopman_train_step) on
// float64 MFMA.
//
// Reference: train() (train.py:89-266) over k_linear_loss (models/losses.py:54-129, "mse") and
// torch.optim.Adam: per step six encoder calls, five lA / lB steps, about fifteen MSE reductions,
// their autograd backward and the optimizer -- a few hundred launches.  Here a step is two:
//
//   k_koopman_grad   one wave serves 16 windows (samples on the MFMA's N side, as in koopman_mpc.hip),
//     four waves a workgroup.  The encoder's forward fragments and biases are staged in LDS (the
//     shared encode<NTL> and its activation-keeping twin below read them); W', [A | B] and A' are
//     read from global memory (lane-contiguous 512-B fragment loads of a blob every wave shares:
//     L2-resident) -- both orientations do not fit the LDS together.
//     Forward, i < P: z^_{i+1} = [A | B][z^_i; u_i] as k_predict steps it; Psi(x_{t0+i+1}) with the
//     hidden activations kept (in the wave's scratch); the loss partials; g_{i+1}; and -- its output gradient
//     being known at once, -g_{i+1}'s feature rows -- that encode's backward right away, so only
//     the encode of x_t0 is run twice.  z^_i and g_{i+1} go to a per-wave scratch (each lane reads
//     back what it wrote).  Reverse, i = P-1 .. 0: dA += lambda_{i+1} z^_i', dB += lambda_{i+1} u_i',
//     lambda_i = g_i + A' lambda_{i+1}; then the encode of x_t0 and its backward with
//     (A' lambda_1)'s feature rows.
//     W' delta chains in registers like the forward (C/D layout = B layout).  The weight-gradient
//     products delta a' contract over the 16 samples: both operands are transposes of the C/D layout
//     and go through a per-wave 16 x 16 LDS tile (row stride 18 doubles: the 16-lane write groups
//     and the 32-lane read groups are conflict-free under the ds_write_b64 / ds_read_b64 bank rules).
//     Every wave accumulates its gradient in its own slot of the workspace, as the products' tiles in
//     the C/D layout (512-B rows, no guards; plain loads and stores, a fixed order); its four loss sums
//     follow it there.  No floating-point atomics.
//   k_koopman_apply  sums the slots in slot order (bitwise reproducible), writes grad and losses and,
//     for train_step, runs Adam on the master vector and rewrites every fragment copy through the
//     index map.  The bias correction's step count lives on the device: k_koopman_grad's first
//     thread advances it (stream order makes it visible to k_koopman_apply), so steps queue
//     without a host round trip.
// The loss (BaseLoss: mse, nmse, weighted_mse; sim_koopman_trainer_set_loss) is a template parameter of both:
// weighted_mse is the same two launches with other constants.  nmse divides by sums over the whole
// minibatch that every sample's backward needs, so two launches precede them:
//   k_koopman_stats       the forward alone, per wave and step the sums of squared errors and labels;
//   k_koopman_nmse_table  one workgroup adds them in a fixed order into the per-step coefficients and the losses.
// No grid-wide barrier, no wave waits on another: stream order is the only dependency.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "koopman_frag.h"
#include "koopman_train_plan.h"
#include "sim_internal.h"

namespace {

using ktrain::TILE_LD;

// what the kernels need of ktrain::Plan (kernel argument)
struct TDev {
  int wt[SIM_KMAXLAYER];
  int ab, at;
  int sw[SIM_KMAXLAYER], sb[SIM_KMAXLAYER], sA;  // offsets into a wave's slot (ktrain::Plan)
  int slot_stride, scr_stride;
  int P, npos;
  double gamma;
};

// transpose of a C/D-layout tile M [16 rows][16 samples] through the wave's LDS tile:
// out[s], lane l = M[l & 15][4 s + (l >> 4)] -- the A operand of k-step s for M, the B operand for M'
DEVI void transpose(double* tile, int lane, d4 c, double (&out)[4]) {
  const int kq = lane >> 4, col = lane & 15;
#pragma unroll
  for (int r = 0; r < 4; r++) tile[(kq + 4 * r) * TILE_LD + col] = c[r];
  wsync();
#pragma unroll
  for (int s = 0; s < 4; s++) out[s] = tile[col * TILE_LD + 4 * s + kq];
  wsync();
}

// the scheduler may not move instructions across this: without it it issues every load of an
// unrolled phase (64 fragment loads, 64 slot loads) first and the kernel spills
DEVI void sched_fence() { __builtin_amdgcn_sched_barrier(0); }

// p, with its value hidden from the optimizer.  Every fragment, slot and scratch access is base +
// a constant, mostly beyond the load's immediate range; seen through, the compiler computes those
// few hundred addresses once, ahead of the loops, and parks them in registers (all 512, and spills).
// Taken from an opaque base inside the loop they are two VALU adds at the point of use instead.
template <class T>
DEVI T* opaque(T* p) {
  asm volatile("" : "+v"(p));
  return p;
}

// slot[.] (+)= v: the wave's own partial (first: nothing to add to yet)
DEVI void accum(double* p, double v, bool first) { *p = first ? v : *p + v; }

// one 64-row layer from the 64-row activations `in`: acc = W in + b (NT output tiles)
template <int NT>
DEVI void dense(const double* A, const double* bias, int kq, const d4 (&in)[KT], d4 (&acc)[KT]) {
#pragma unroll
  for (int T = 0; T < NT; T++)
#pragma unroll
    for (int r = 0; r < 4; r++) acc[T][r] = bias[16 * T + kq + 4 * r];
#pragma unroll
  for (int s = 0; s < 4 * KT; s++)
#pragma unroll
    for (int T = 0; T < NT; T++) acc[T] = mfma(A[(T * 16 + s) * 64], in[s >> 2][s & 3], acc[T]);
}

// the hidden activations of one encode in the wave's scratch: hs[(16 l + 4 T + r) * 64] (hs carries the lane)
DEVI void put_h(double* hs, int l, const d4 (&a)[KT]) {
  hs = opaque(hs + l * KT * 4 * 64) - l * KT * 4 * 64;
#pragma unroll
  for (int T = 0; T < KT; T++)
#pragma unroll
    for (int r = 0; r < 4; r++) hs[((l * KT + T) * 4 + r) * 64] = a[T][r];
}
DEVI void get_h(const double* hs, int l, d4 (&a)[KT]) {
  hs = opaque(hs + l * KT * 4 * 64) - l * KT * 4 * 64;
#pragma unroll
  for (int T = 0; T < KT; T++)
#pragma unroll
    for (int r = 0; r < 4; r++) a[T][r] = hs[((l * KT + T) * 4 + r) * 64];
}

// encode<NTL> (koopman_frag.h) that also keeps the hidden layers' activations (after the ReLU:
// h > 0 is the ReLU's derivative) for the backward, in the wave's scratch: each lane reads back what
// it wrote.  (Held in registers across the backward they cost 128 VGPRs and the kernel spilled.)
template <int NTL>
DEVI void encode_keep(const KDev& K, const double* lds, int lane, const double xb[2], double* hs, d4 (&out)[KT]) {
  const int kq = lane >> 4;
  d4 acc[KT], cur[KT];
  {
    const double* A = lds + K.frag[0] + lane;
    const double* bias = lds + K.bias;
#pragma unroll
    for (int T = 0; T < KT; T++)
#pragma unroll
      for (int r = 0; r < 4; r++) acc[T][r] = bias[16 * T + kq + 4 * r];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
      for (int T = 0; T < KT; T++) acc[T] = mfma(A[(T * 2 + s) * 64], xb[s], acc[T]);
#pragma unroll
    for (int T = 0; T < KT; T++)
#pragma unroll
      for (int r = 0; r < 4; r++) cur[T][r] = fmax(acc[T][r], 0.0);
  }
  put_h(hs, 0, cur);
  for (int l = 1; l < K.nl - 1; l++) {
    dense<KT>(lds + K.frag[l] + lane, lds + K.bias + l * SIM_KMAXW, kq, cur, acc);
#pragma unroll
    for (int T = 0; T < KT; T++)
#pragma unroll
      for (int r = 0; r < 4; r++) cur[T][r] = fmax(acc[T][r], 0.0);
    put_h(hs, l, cur);
  }
  dense<NTL>(lds + K.frag[K.nl - 1] + lane, lds + K.bias + (K.nl - 1) * SIM_KMAXW, kq, cur, acc);
#pragma unroll
  for (int T = 0; T < KT; T++) out[T] = T < NTL ? acc[T] : d4{0, 0, 0, 0};
}

// one layer of the backward for the wave's 16 samples: dl = delta_l (NTO tiles, C/D layout), ain =
// the layer's input a_{l-1} (NTI tiles).  dW_l += delta_l a_{l-1}' and db_l += its row sums, in the
// wave's slot: dW as its [NTO][NTI] tiles in the C/D layout ([r][lane]: 512-B rows, no guards -- the
// padding rows and columns are exact zeros), db [64].  PROP: dl <- (W_l' delta_l) . [ain > 0] =
// delta_{l-1} (WT: W_l' fragments + lane).
template <int NTO, int NTI, bool PROP>
DEVI void layer_backward(double* tile, double* dW, double* db, const double* WT, int lane, const d4 (&ain)[KT],
                         d4 (&dl)[KT], bool first) {
  const int kq = lane >> 4, col = lane & 15;
  dW = opaque(dW), db = opaque(db), WT = opaque(WT);
  double tA[NTO][4], tB[NTI][4];
#pragma unroll
  for (int T = 0; T < NTO; T++) transpose(tile, lane, dl[T], tA[T]);
#pragma unroll
  for (int T = 0; T < NTI; T++) transpose(tile, lane, ain[T], tB[T]);
  // the row sums of delta_l: 4 samples in the lane, then the 4 lane groups
#pragma unroll
  for (int T = 0; T < NTO; T++) {
    double s = (tA[T][0] + tA[T][1]) + (tA[T][2] + tA[T][3]);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (kq == 0) accum(db + 16 * T + col, s, first);
  }
  // delta_l a_{l-1}': the K side is the 16 samples
  sched_fence();
#pragma unroll
  for (int Tr = 0; Tr < NTO; Tr++) {
#pragma unroll
    for (int Tc = 0; Tc < NTI; Tc++) {
      d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; s++) acc = mfma(tA[Tr][s], tB[Tc][s], acc);
#pragma unroll
      for (int r = 0; r < 4; r++) accum(dW + ((Tr * NTI + Tc) * 4 + r) * 64 + lane, acc[r], first);
    }
    sched_fence();
  }
  if (PROP) {
    d4 acc[KT];
#pragma unroll
    for (int T = 0; T < KT; T++) acc[T] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int Ts = 0; Ts < NTO; Ts++) {  // 16 fragment loads in flight, then their MFMAs
      double w[4][KT];
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int T = 0; T < KT; T++) w[r][T] = WT[(T * 4 * NTO + 4 * Ts + r) * 64];
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int T = 0; T < KT; T++) acc[T] = mfma(w[r][T], dl[Ts][r], acc[T]);
      sched_fence();
    }
#pragma unroll
    for (int T = 0; T < KT; T++)
#pragma unroll
      for (int r = 0; r < 4; r++) dl[T][r] = ain[T][r] > 0.0 ? acc[T][r] : 0.0;
  }
}

// the encoder's backward: dl = dLoss/d(output) (zero past the output's NTL tiles), xb the encode's
// input, hs its kept activations
template <int NTL>
DEVI void encode_backward(const KDev& K, const TDev& D, const double* blob, double* tile, double* slot,
                          int lane, const double xb[2], const double* hs, d4 (&dl)[KT], bool first) {
  d4 ain[KT];
  int L = K.nl - 1;
  get_h(hs, L - 1, ain);
  layer_backward<NTL, KT, true>(tile, slot + D.sw[L], slot + D.sb[L], blob + D.wt[L] + lane, lane, ain, dl, first);
  for (L = K.nl - 2; L >= 1; L--) {
    get_h(hs, L - 1, ain);
    layer_backward<KT, KT, true>(tile, slot + D.sw[L], slot + D.sb[L], blob + D.wt[L] + lane, lane, ain, dl, first);
  }
  ain[0] = d4{xb[0], xb[1], 0.0, 0.0};
  layer_backward<KT, 1, false>(tile, slot + D.sw[0], slot + D.sb[0], blob, lane, ain, dl, first);
}

// z^_{i+1} = [A | B] [z^_i; u_i] (+ the bilinear term) for the wave's 16 samples, from z^_i = (zx, zf)
// and u_i = ub in the B layout: zn's tile 0 = the x rows, tiles 1.. = the features.  AB: [A | B]'s
// fragments + lane (opaque).  k_koopman_stats' rollout; k_koopman_grad carries the same lines in its
// loop (called from there the compiler allocates that kernel's registers differently, and it has none
// to spare)
template <int NTL, bool BIL>
DEVI void model_step(const KDev& K, const TDev& D, const double* blob, const double* AB, int lane,
                     const double (&zx)[2], const d4 (&zf)[KT], const double (&ub)[2], d4 (&zn)[1 + NTL]) {
  constexpr int NZT = 1 + NTL;            // tiles of the lifted state
  constexpr int ABKS = 2 + 4 * NTL + 2;   // k-steps of [A | B]
  constexpr int ATKS = 2 + 4 * NTL;       // k-steps of A'
  const int col = lane & 15;
#pragma unroll
  for (int q = 0; q < NZT; q++) zn[q] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s0 = 0; s0 < ABKS; s0 += 4) {  // (ABKS is a multiple of 4) 4 NZT fragment loads, then their MFMAs
    double w[4][NZT];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int q = 0; q < NZT; q++) w[j][q] = AB[(q * ABKS + s0 + j) * 64];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int s = s0 + j;
      const double b = s < 2 ? zx[s] : (s < 2 + 4 * NTL ? zf[(s - 2) >> 2][(s - 2) & 3] : ub[s - 2 - 4 * NTL]);
#pragma unroll
      for (int q = 0; q < NZT; q++) zn[q] = mfma(w[j][q], b, zn[q]);
    }
    sched_fence();
  }
  if constexpr (BIL) {  // + sum_c H_c (u_c z^_i): A's k-loop per c, the B operand scaled by the sample's u_c
    for (int c = 0; c < K.ud; c++) {
      // ub is in the B layout: u_c sits in register c >> 2 of the lane with kq = c & 3 and this column
      const double uc = __shfl(c < 4 ? ub[0] : ub[1], (c & 3) * 16 + col);
      const double* HF = opaque(blob + D.at + (size_t)(1 + c) * (NZT * ATKS * 64) + lane);
      double sz[ATKS];
      sz[0] = uc * zx[0], sz[1] = uc * zx[1];
#pragma unroll
      for (int q = 0; q < NTL; q++)
#pragma unroll
        for (int r = 0; r < 4; r++) sz[2 + 4 * q + r] = uc * zf[q][r];
#pragma unroll
      for (int s0 = 0; s0 < ATKS; s0 += 2) {  // (ATKS is even) 2 NZT fragment loads, then their MFMAs
        double w[2][NZT];
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
          for (int q = 0; q < NZT; q++) w[j][q] = HF[(q * ATKS + s0 + j) * 64];
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
          for (int q = 0; q < NZT; q++) zn[q] = mfma(w[j][q], sz[s0 + j], zn[q]);
        sched_fence();
      }
    }
  }
}

// the per-step table of the nmse loss (k_koopman_nmse_table): read from a wave-uniform address in the
// constant address space, so it costs scalar loads and no VGPRs
typedef const double __attribute__((address_space(4))) * ctab_t;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
DEVI ctab_t tab_of(const int* step) { return (ctab_t)(reinterpret_cast<const double*>(step) + ktrain::STEP_DOUBLES); }
#pragma clang diagnostic pop

// (blob, ws and scratch are not __restrict__: the fragment loads of [A | B], A' and the last layer's W'
// are invariant across the steps, and with the promise that the slot's stores do not alias them the
// compiler keeps all of them in registers across the loop -- 200 VGPRs at four feature tiles, and spills)
//
// BIL: the bilinear DBKN step z^_{i+1} = A z^_i + B u_i + sum_c H_c (u_{i,c} z^_i), c < u_dim.  Its blocks
// follow the linear ones (koopman_train_plan.h): the H_c fragments [ud][NZT][ATKS][64] right after A',
// then the H_c' ones; dH_c's tiles [ud][NZT][NZT] right after [dA | dB] in the slot.  u_c of the lane's
// sample is a scalar on the N side, so it scales the B operand (forward), the transposed z^ tiles
// (dH_c = lambda_{i+1} (u_c z^_i)') and the C/D output (u_c H_c' lambda_{i+1}); c is a runtime loop.
//
// LOSS (include/koopman_mpc.h SIM_KLOSS_*) changes g_{i+1}, the target encode's output gradient and the
// loss partials alone; the kernel sits at the register limit, so the choice is made at compile time.
//   mse           g = c_i (2 / (n nz) e, + 2 / (n x_dim) ex on the x rows); four sums (koopman, pred, dis, angle).
//   weighted_mse  g = c_i 2 weight(row) e: per-lane constants for the x tile's two registers, one scalar for
//                 the features.  The "first three columns" / "rest" halves of the four sums: per lane the
//                 x tile's two rows and the features are summed apart and sorted into the halves at the end.
//   nmse          g = c_i (2 / D^k_i e, + 2 / D^p_i ex on the x rows); the label is not detached, so the
//                 target encode's output gradient gains -c_i 2 N^k_i / (D^k_i)^2 z_f.  The coefficients come
//                 from the table [P][4] (k_koopman_nmse_table) that follows the step count in step's buffer
//                 (tab_of: the argument list is the same for every loss), the losses too: no sums here.
template <int NTL, bool BIL, int LOSS>
__global__ __launch_bounds__(256) void k_koopman_grad(KDev K, TDev D, const double* blob, int n, int N,
                                                       const float* __restrict__ rows, int ld, int x_off, int u_off,
                                                       const int* __restrict__ traj_idx, int t0,
                                                       double* ws, double* scratch,
                                                       int* __restrict__ step, int bump) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  stage(lds, blob, K.total);
  if (bump && blockIdx.x == 0 && threadIdx.x == 0) step[0] += 1;
  constexpr int NZT = 1 + NTL;            // tiles of the lifted state
  constexpr int ABKS = 2 + 4 * NTL + 2;   // k-steps of [A | B]
  constexpr int ATKS = 2 + 4 * NTL;       // k-steps of A'
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, col = lane & 15;
  const int wave = blockIdx.x * (blockDim.x >> 6) + wid;
  if (wave * 16 >= n) return;  // (whole waves: no workgroup barrier below)
  const int e = wave * 16 + col;
  const bool live = e < n;
  int tr = 0;
  if (live) tr = traj_idx ? min(max(traj_idx[e], 0), N - 1) : e;
  const size_t ts = (size_t)N * ld;
  const float* __restrict__ r0 = rows + (size_t)t0 * ts + (size_t)tr * ld;
  double* tile = lds + K.total + wid * 16 * TILE_LD;
  double* slot = ws + (size_t)wave * D.slot_stride;
  double* scr = scratch + (size_t)wave * D.scr_stride + lane;
  double* hs = scr + (size_t)D.P * 2 * NZT * 256;  // one encode's hidden activations: [nl - 1][KT][4][64]
  const int P = D.P;
  double cont = 0.0;
  {
    double b = 1.0;
    for (int i = 0; i < P; i++) cont += b, b *= D.gamma;
  }
  // mse: the two means' factors.  weighted_mse: wx[s] = 2 (koopman's + pred's weight) of x row 4 s + kq
  // (rows >= x_dim carry a zero error), ck = 2 the feature rows' one weight
  double ck = 2.0 / ((double)n * K.nz), cp = 2.0 / ((double)n * K.xd);
  double wx[2] = {0.0, 0.0};
  if constexpr (LOSS == SIM_KLOSS_WEIGHTED_MSE) {
    const double lo = 2.0 / (30.0 * n), hk = 18.0 / (10.0 * n * (K.nz - 3)), hp = 18.0 / (10.0 * n * (K.xd - 3));
#pragma unroll
    for (int s = 0; s < 2; s++) wx[s] = 4 * s + kq < 3 ? lo + lo : hk + hp;
    ck = hk;
  }
  ctab_t ct = tab_of(step);

  double x0[2], zx[2];
  load_pair(r0 + x_off, live, K.xd, kq, x0);
  d4 zf[KT];
  encode<NTL>(K, lds, lane, x0, zf);
  zx[0] = x0[0], zx[1] = x0[1];
  // mse: koopman, pred, dis, angle.  weighted_mse: x row kq, x row 4 + kq, the features (sd)
  double sk = 0.0, sp = 0.0, sd = 0.0, sa = 0.0;
  double gx[2] = {0.0, 0.0};
  d4 gf[NTL];
  double beta = 1.0;
  for (int i = 0; i < P; i++) {
    const float* __restrict__ ri = r0 + (size_t)i * ts;
    double ub[2], xn[2];
    load_pair(ri + u_off, live, K.ud, kq, ub);
    load_pair(ri + ts + x_off, live, K.xd, kq, xn);
    // z^_i to the scratch: [i][0][tile][r][64]
    double* si = opaque(scr + (size_t)i * 2 * NZT * 256);
    const double* AB = opaque(blob + D.ab + lane);
    si[0] = zx[0], si[64] = zx[1];
#pragma unroll
    for (int q = 0; q < NTL; q++)
#pragma unroll
      for (int r = 0; r < 4; r++) si[((1 + q) * 4 + r) * 64] = zf[q][r];
    // z^_{i+1} = [A | B] [z^_i; u_i]: tile 0 = the x rows, tiles 1.. = the features
    d4 zn[NZT];
#pragma unroll
    for (int q = 0; q < NZT; q++) zn[q] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s0 = 0; s0 < ABKS; s0 += 4) {  // (ABKS is a multiple of 4) 4 NZT fragment loads, then their MFMAs
      double w[4][NZT];
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int q = 0; q < NZT; q++) w[j][q] = AB[(q * ABKS + s0 + j) * 64];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int s = s0 + j;
        const double b = s < 2 ? zx[s] : (s < 2 + 4 * NTL ? zf[(s - 2) >> 2][(s - 2) & 3] : ub[s - 2 - 4 * NTL]);
#pragma unroll
        for (int q = 0; q < NZT; q++) zn[q] = mfma(w[j][q], b, zn[q]);
      }
      sched_fence();
    }
    if constexpr (BIL) {  // + sum_c H_c (u_c z^_i): A's k-loop per c, the B operand scaled by the sample's u_c
      for (int c = 0; c < K.ud; c++) {
        // ub is in the B layout: u_c sits in register c >> 2 of the lane with kq = c & 3 and this column
        const double uc = __shfl(c < 4 ? ub[0] : ub[1], (c & 3) * 16 + col);
        const double* HF = opaque(blob + D.at + (size_t)(1 + c) * (NZT * ATKS * 64) + lane);
        double sz[ATKS];
        sz[0] = uc * zx[0], sz[1] = uc * zx[1];
#pragma unroll
        for (int q = 0; q < NTL; q++)
#pragma unroll
          for (int r = 0; r < 4; r++) sz[2 + 4 * q + r] = uc * zf[q][r];
#pragma unroll
        for (int s0 = 0; s0 < ATKS; s0 += 2) {  // (ATKS is even) 2 NZT fragment loads, then their MFMAs
          double w[2][NZT];
#pragma unroll
          for (int j = 0; j < 2; j++)
#pragma unroll
            for (int q = 0; q < NZT; q++) w[j][q] = HF[(q * ATKS + s0 + j) * 64];
#pragma unroll
          for (int j = 0; j < 2; j++)
#pragma unroll
            for (int q = 0; q < NZT; q++) zn[q] = mfma(w[j][q], sz[s0 + j], zn[q]);
          sched_fence();
        }
      }
    }
    // Psi(x_{t0+i+1}), its hidden activations kept for the backward below
    d4 out[KT];
    encode_keep<NTL>(K, lds, lane, xn, hs, out);
    // the error, the loss partials, g_{i+1}
    const double c = beta / cont;
    d4 dl[KT];
    if constexpr (LOSS == SIM_KLOSS_NMSE) ck = 2.0 * ct[4 * i], cp = 2.0 * ct[4 * i + 2];  // 2 / D^k_i, 2 / D^p_i
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const int row = 4 * s + kq;
      const double ex = live ? zn[0][s] - xn[s] : 0.0;  // (rows >= x_dim: both are zero)
      const double e2 = beta * ex * ex;
      if constexpr (LOSS == SIM_KLOSS_MSE) {
        sk += e2, sp += e2;
        if (row < D.npos) sd += e2; else sa += e2;
      }
      if constexpr (LOSS == SIM_KLOSS_WEIGHTED_MSE) {
        if (s == 0) sk += e2; else sp += e2;
        gx[s] = c * wx[s] * ex;
      } else {
        gx[s] = c * (ck + cp) * ex;
      }
    }
#pragma unroll
    for (int q = 0; q < NTL; q++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const double ef = live ? zn[1 + q][r] - out[q][r] : 0.0;  // (rows >= the output width: both zero)
        if constexpr (LOSS == SIM_KLOSS_MSE) sk += beta * ef * ef;
        if constexpr (LOSS == SIM_KLOSS_WEIGHTED_MSE) sd += beta * ef * ef;
        gf[q][r] = c * ck * ef;
      }
    double* sg = si + NZT * 256;  // g_{i+1}: [i][1][tile][r][64]
    sg[0] = gx[0], sg[64] = gx[1];
#pragma unroll
    for (int q = 0; q < NTL; q++)
#pragma unroll
      for (int r = 0; r < 4; r++) sg[((1 + q) * 4 + r) * 64] = gf[q][r];
    // the target encode's output gradient is -g_{i+1}'s feature rows
#pragma unroll
    for (int T = 0; T < KT; T++) dl[T] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < NTL; q++) dl[q] = -gf[q];
    if constexpr (LOSS == SIM_KLOSS_NMSE) {  // the normaliser D^k_i's own gradient: -c_i 2 N^k_i / (D^k_i)^2 z_f
      const double cn = live ? c * 2.0 * ct[4 * i + 1] : 0.0;
#pragma unroll
      for (int q = 0; q < NTL; q++) dl[q] -= cn * out[q];
    }
    encode_backward<NTL>(K, D, blob, tile, slot, lane, xn, hs, dl, i == 0);
    zx[0] = zn[0][0], zx[1] = zn[0][1];
#pragma unroll
    for (int q = 0; q < NTL; q++) zf[q] = zn[1 + q];
    beta *= D.gamma;
  }

  // reverse: lambda_{i+1} in (lx, lf); dA, dB; lambda_i = g_i + A' lambda_{i+1}
  double lx[2] = {gx[0], gx[1]};
  d4 lf[NTL];
#pragma unroll
  for (int q = 0; q < NTL; q++) lf[q] = gf[q];
  for (int i = P - 1; i >= 0; i--) {
    const float* __restrict__ ri = r0 + (size_t)i * ts;
    const double* si = opaque(scr + (size_t)i * 2 * NZT * 256);
    const double* AT = opaque(blob + D.at + lane);
    double* sA = opaque(slot + D.sA + lane);
    double ub[2];
    load_pair(ri + u_off, live, K.ud, kq, ub);
    d4 zt[NZT];
    zt[0] = d4{si[0], si[64], 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < NTL; q++)
#pragma unroll
      for (int r = 0; r < 4; r++) zt[1 + q][r] = si[((1 + q) * 4 + r) * 64];
    double tA[NZT][4], tB[NZT + 1][4];
    transpose(tile, lane, d4{lx[0], lx[1], 0.0, 0.0}, tA[0]);
#pragma unroll
    for (int q = 0; q < NTL; q++) transpose(tile, lane, lf[q], tA[1 + q]);
#pragma unroll
    for (int q = 0; q < NZT; q++) transpose(tile, lane, zt[q], tB[q]);
    transpose(tile, lane, d4{ub[0], ub[1], 0.0, 0.0}, tB[NZT]);
    const bool first = i == P - 1;
    sched_fence();
#pragma unroll
    for (int Tr = 0; Tr < NZT; Tr++) {
#pragma unroll
      for (int Tc = 0; Tc < NZT + 1; Tc++) {
        d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; s++) acc = mfma(tA[Tr][s], tB[Tc][s], acc);
#pragma unroll
        for (int r = 0; r < 4; r++) accum(sA + ((Tr * (NZT + 1) + Tc) * 4 + r) * 64, acc[r], first);
      }
      sched_fence();
    }
    if constexpr (BIL) {  // dH_c += lambda_{i+1} (u_c z^_i)': dA's products, the transposed z^ tiles scaled
      for (int c = 0; c < K.ud; c++) {
        double* sH = opaque(slot + D.sA + NZT * (NZT + 1) * 256 + c * (NZT * NZT * 256) + lane);
        double tS[NZT][4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
          // the transposed u tile's row c: u_c of sample 4 s + kq sits in the lane of that kq with column c
          const double us = __shfl(tB[NZT][s], kq * 16 + c);
#pragma unroll
          for (int q = 0; q < NZT; q++) tS[q][s] = us * tB[q][s];
        }
        sched_fence();
#pragma unroll
        for (int Tr = 0; Tr < NZT; Tr++) {
#pragma unroll
          for (int Tc = 0; Tc < NZT; Tc++) {
            d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 4; s++) acc = mfma(tA[Tr][s], tS[Tc][s], acc);
#pragma unroll
            for (int r = 0; r < 4; r++) accum(sH + ((Tr * NZT + Tc) * 4 + r) * 64, acc[r], first);
          }
          sched_fence();
        }
      }
    }
    d4 ln[NZT];
#pragma unroll
    for (int q = 0; q < NZT; q++) ln[q] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s0 = 0; s0 < ATKS; s0 += 2) {  // (ATKS is even)
      double w[2][NZT];
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int q = 0; q < NZT; q++) w[j][q] = AT[(q * ATKS + s0 + j) * 64];
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int s = s0 + j;
        const double b = s < 2 ? lx[s] : lf[(s - 2) >> 2][(s - 2) & 3];
#pragma unroll
        for (int q = 0; q < NZT; q++) ln[q] = mfma(w[j][q], b, ln[q]);
      }
      sched_fence();
    }
    if constexpr (BIL) {  // + sum_c u_c (H_c' lambda_{i+1}): A's loop into a fresh accumulator, its output scaled
      for (int c = 0; c < K.ud; c++) {
        const double uc = __shfl(c < 4 ? ub[0] : ub[1], (c & 3) * 16 + col);
        const double* HT = opaque(blob + D.at + (size_t)(1 + K.ud + c) * (NZT * ATKS * 64) + lane);
        d4 lh[NZT];
#pragma unroll
        for (int q = 0; q < NZT; q++) lh[q] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s0 = 0; s0 < ATKS; s0 += 2) {
          double w[2][NZT];
#pragma unroll
          for (int j = 0; j < 2; j++)
#pragma unroll
            for (int q = 0; q < NZT; q++) w[j][q] = HT[(q * ATKS + s0 + j) * 64];
#pragma unroll
          for (int j = 0; j < 2; j++) {
            const int s = s0 + j;
            const double b = s < 2 ? lx[s] : lf[(s - 2) >> 2][(s - 2) & 3];
#pragma unroll
            for (int q = 0; q < NZT; q++) lh[q] = mfma(w[j][q], b, lh[q]);
          }
          sched_fence();
        }
#pragma unroll
        for (int q = 0; q < NZT; q++) ln[q] += uc * lh[q];
      }
    }
    if (i > 0) {  // + g_i
      const double* sg = opaque(scr + ((size_t)(i - 1) * 2 + 1) * NZT * 256);
      ln[0][0] += sg[0], ln[0][1] += sg[64];
#pragma unroll
      for (int q = 0; q < NTL; q++)
#pragma unroll
        for (int r = 0; r < 4; r++) ln[1 + q][r] += sg[((1 + q) * 4 + r) * 64];
    }
    lx[0] = ln[0][0], lx[1] = ln[0][1];
#pragma unroll
    for (int q = 0; q < NTL; q++) lf[q] = ln[1 + q];
  }
  {  // the encode of x_t0: its output gradient is (A' lambda_1)'s feature rows
    d4 out[KT], dl[KT];
    encode_keep<NTL>(K, lds, lane, x0, hs, out);
#pragma unroll
    for (int T = 0; T < KT; T++) dl[T] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < NTL; q++) dl[q] = lf[q];
    encode_backward<NTL>(K, D, blob, tile, slot, lane, x0, hs, dl, false);
  }
  // the wave's loss sums: a fixed butterfly, the same bits in every lane
  if constexpr (LOSS == SIM_KLOSS_MSE) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      sk += __shfl_xor(sk, m), sp += __shfl_xor(sp, m);
      sd += __shfl_xor(sd, m), sa += __shfl_xor(sa, m);
    }
    if (lane == 0) {
      double* sl = slot + D.slot_stride - 8;
      sl[0] = sk, sl[1] = sp, sl[2] = sd, sl[3] = sa;
    }
  }
  if constexpr (LOSS == SIM_KLOSS_WEIGHTED_MSE) {
    // the lane's two x rows into the halves: [0] columns < 3 of x, [1] the other x columns, [2] the
    // features, then dis (columns < npos) and angle (the rest) split at their own column 3
    double v[7] = {0.0, 0.0, sd, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const int row = 4 * s + kq;
      const bool dis = row < D.npos, own = (dis ? row : row - D.npos) < 3;  // (selects: v stays in registers)
      const double e2 = s == 0 ? sk : sp;
      v[0] += row < 3 ? e2 : 0.0, v[1] += row < 3 ? 0.0 : e2;
      v[3] += dis && own ? e2 : 0.0, v[4] += dis && !own ? e2 : 0.0;
      v[5] += !dis && own ? e2 : 0.0, v[6] += !dis && !own ? e2 : 0.0;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1)
#pragma unroll
      for (int k = 0; k < 7; k++) v[k] += __shfl_xor(v[k], m);
    if (lane == 0) {  // koopman, pred, dis, angle: each its first three columns, then its rest
      double* sl = slot + D.slot_stride - 8;
      sl[0] = v[0], sl[1] = v[1] + v[2], sl[2] = v[0], sl[3] = v[1];
      sl[4] = v[3], sl[5] = v[4], sl[6] = v[5], sl[7] = v[6];
    }
  }
}

// the nmse normalisers, forward only: k_koopman_grad's mapping, early return and rollout of z^ with the
// plain encode of each target; per wave and step the partial sums
//   stat[wave][i][8] = N^k, D^k, N^p, D^p, N^dis, D^dis, N^ang, D^ang
// (N: squared errors, D: squared labels; k over all of z, p over x, dis / ang over x's columns < / >= npos),
// a fixed butterfly and one lane's stores.  Every wave below ceil(n / 16) writes all P rows.
template <int NTL, bool BIL>
__global__ __launch_bounds__(256) void k_koopman_stats(KDev K, TDev D, const double* blob, int n, int N,
                                                        const float* __restrict__ rows, int ld, int x_off, int u_off,
                                                        const int* __restrict__ traj_idx, int t0, double* stat) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  stage(lds, blob, K.total);
  constexpr int NZT = 1 + NTL;
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, col = lane & 15;
  const int wave = blockIdx.x * (blockDim.x >> 6) + wid;
  if (wave * 16 >= n) return;  // (whole waves: no workgroup barrier below)
  const int e = wave * 16 + col;
  const bool live = e < n;
  int tr = 0;
  if (live) tr = traj_idx ? min(max(traj_idx[e], 0), N - 1) : e;
  const size_t ts = (size_t)N * ld;
  const float* __restrict__ r0 = rows + (size_t)t0 * ts + (size_t)tr * ld;
  double* st = stat + (size_t)wave * D.P * 8;
  double zx[2];
  load_pair(r0 + x_off, live, K.xd, kq, zx);
  d4 zf[KT];
  encode<NTL>(K, lds, lane, zx, zf);
  for (int i = 0; i < D.P; i++) {
    const float* __restrict__ ri = r0 + (size_t)i * ts;
    double ub[2], xn[2];
    load_pair(ri + u_off, live, K.ud, kq, ub);
    load_pair(ri + ts + x_off, live, K.xd, kq, xn);
    d4 zn[NZT], out[KT];
    model_step<NTL, BIL>(K, D, blob, opaque(blob + D.ab + lane), lane, zx, zf, ub, zn);
    encode<NTL>(K, lds, lane, xn, out);
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // N, D of: the features, dis, angle
#pragma unroll
    for (int q = 0; q < NTL; q++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const double zt = live ? out[q][r] : 0.0, ef = live ? zn[1 + q][r] - zt : 0.0;
        v[0] += ef * ef, v[1] += zt * zt;
      }
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const double ex = live ? zn[0][s] - xn[s] : 0.0;  // (xn is zero in a dead lane and in rows >= x_dim)
      const bool dis = 4 * s + kq < D.npos;  // (selects: v stays in registers)
      const double e2 = ex * ex, x2 = xn[s] * xn[s];
      v[2] += dis ? e2 : 0.0, v[3] += dis ? x2 : 0.0;
      v[4] += dis ? 0.0 : e2, v[5] += dis ? 0.0 : x2;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1)
#pragma unroll
      for (int k = 0; k < 6; k++) v[k] += __shfl_xor(v[k], m);
    if (lane == 0) {
      const double np = v[2] + v[4], dp = v[3] + v[5];
      double* o = st + i * 8;
      o[0] = np + v[0], o[1] = dp + v[1], o[2] = np, o[3] = dp;
      o[4] = v[2], o[5] = v[3], o[6] = v[4], o[7] = v[5];
    }
    zx[0] = zn[0][0], zx[1] = zn[0][1];
#pragma unroll
    for (int q = 0; q < NTL; q++) zf[q] = zn[1 + q];
  }
}

// the nmse table, one workgroup: the waves' partials of each (step, sum) added in a fixed order (lane l
// takes waves l, l + 64, .. in turn, then a fixed butterfly), once; then per step
//   tab[i][4] = 1 / D^k_i, N^k_i / (D^k_i)^2, 1 / D^p_i, 0      (k_koopman_grad reads these)
// and the six losses at tab[4 P ..].  A zero normaliser gives inf / NaN, as in torch.
__global__ __launch_bounds__(1024) void k_koopman_nmse_table(const double* __restrict__ stat, double* __restrict__ tab,
                                                              int nslot, int P, double gamma) {
  __shared__ double red[ktrain::MAXP * 8];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  for (int pr = wid; pr < P * 8; pr += nw) {
    double s = 0.0;
    for (int w = lane; w < nslot; w += 64) s += stat[(size_t)w * P * 8 + pr];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
    if (lane == 0) red[pr] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < P) {
    const double* r = red + 8 * threadIdx.x;
    double* t = tab + 4 * threadIdx.x;
    t[0] = 1.0 / r[1], t[1] = r[0] / (r[1] * r[1]), t[2] = 1.0 / r[3], t[3] = 0.0;
  }
  if (threadIdx.x == 0) {
    double cont = 0.0, b = 1.0, s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < P; i++) {
      const double* r = red + 8 * i;
#pragma unroll
      for (int k = 0; k < 4; k++) s[k] += b * (r[2 * k] / r[2 * k + 1]);
      cont += b, b *= gamma;
    }
    double* l = tab + 4 * P;
    const double koop = s[0] / cont, pred = s[1] / cont;
    l[0] = koop + pred, l[1] = koop, l[2] = pred;
    l[3] = 0.0;  // recon: lC Psi(x) = x exactly
    l[4] = s[2] / cont, l[5] = s[3] / cont;
  }
}

struct ADev {
  int nparam, nslot, slot_stride, n, P, xd, nz, npos, update;
  double gamma, lr, beta1, beta2, eps;
  const double* ws;
  double *grad, *losses, *params, *m, *v, *blob;
  const int* step;
  const int* map;   // [2][nparam]
  const int* gidx;  // [nparam]: where a wave's slot holds the parameter's gradient
};

// LOSS: how the six losses come out of the slots' eight trailing sums (mse: four; weighted_mse: the halves
// of each, NaN for a mean over no column, as torch's) or, for nmse, out of the table
template <int LOSS>
__global__ __launch_bounds__(256) void k_koopman_apply(ADev a) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < a.nparam) {
    double g = 0.0;
    const double* w = a.ws + a.gidx[p];
#pragma unroll 8
    for (int s = 0; s < a.nslot; s++) g += w[(size_t)s * a.slot_stride];  // (8 loads in flight; the adds in slot order)
    if (a.grad) a.grad[p] = g;
    if (a.update) {
      const double t = (double)a.step[0];
      const double bc1 = 1.0 - pow(a.beta1, t), bc2 = 1.0 - pow(a.beta2, t);
      const double m = a.beta1 * a.m[p] + (1.0 - a.beta1) * g;
      const double v = a.beta2 * a.v[p] + (1.0 - a.beta2) * g * g;
      const double q = a.params[p] - (a.lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + a.eps));
      a.m[p] = m, a.v[p] = v, a.params[p] = q;
      const int c0 = a.map[p], c1 = a.map[a.nparam + p];
      if (c0 >= 0) a.blob[c0] = q;
      if (c1 >= 0) a.blob[c1] = q;
    }
  }
  if constexpr (LOSS == SIM_KLOSS_MSE) {
    if (p == 0 && a.losses) {
      double s[4] = {0.0, 0.0, 0.0, 0.0};
      for (int w = 0; w < a.nslot; w++) {
        const double* sl = a.ws + (size_t)(w + 1) * a.slot_stride - 8;
#pragma unroll
        for (int k = 0; k < 4; k++) s[k] += sl[k];
      }
      double cont = 0.0, b = 1.0;
      for (int i = 0; i < a.P; i++) cont += b, b *= a.gamma;
      const double nn = (double)a.n * cont;
      const double koop = s[0] / (nn * a.nz), pred = s[1] / (nn * a.xd);
      a.losses[0] = koop + pred;
      a.losses[1] = koop;
      a.losses[2] = pred;
      a.losses[3] = 0.0;  // recon: lC Psi(x) = x exactly
      a.losses[4] = s[2] / (nn * a.npos);
      a.losses[5] = s[3] / (nn * (a.xd - a.npos));
    }
  }
  if constexpr (LOSS == SIM_KLOSS_WEIGHTED_MSE) {
    if (p == 0 && a.losses) {
      double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int w = 0; w < a.nslot; w++) {
        const double* sl = a.ws + (size_t)(w + 1) * a.slot_stride - 8;
#pragma unroll
        for (int k = 0; k < 8; k++) s[k] += sl[k];
      }
      double cont = 0.0, b = 1.0;
      for (int i = 0; i < a.P; i++) cont += b, b *= a.gamma;
      const double nn = (double)a.n * cont;
      // (mse of the first three columns + 9 mse of the d - 3 others) / 10 of a d-column slice
      auto wm = [&](double lo, double hi, int d) { return d > 3 ? (lo / (nn * 3) + 9.0 * (hi / (nn * (d - 3)))) / 10.0 : NAN; };
      const double koop = wm(s[0], s[1], a.nz), pred = wm(s[2], s[3], a.xd);
      a.losses[0] = koop + pred;
      a.losses[1] = koop;
      a.losses[2] = pred;
      a.losses[3] = 0.0;
      a.losses[4] = wm(s[4], s[5], a.npos);
      a.losses[5] = wm(s[6], s[7], a.xd - a.npos);
    }
  }
  if constexpr (LOSS == SIM_KLOSS_NMSE) {
    if (p < 6 && a.losses) a.losses[p] = tab_of(a.step)[4 * a.P + p];
  }
}

typedef void (*GradFn)(KDev, TDev, const double*, int, int, const float*, int, int, int, const int*, int, double*,
                       double*, int*, int);
#define GRAD_ROW(BIL, LOSS) \
  {k_koopman_grad<1, BIL, LOSS>, k_koopman_grad<2, BIL, LOSS>, k_koopman_grad<3, BIL, LOSS>, k_koopman_grad<4, BIL, LOSS>}
const GradFn GRAD[3][2][4] = {{GRAD_ROW(false, SIM_KLOSS_MSE), GRAD_ROW(true, SIM_KLOSS_MSE)},  // [loss][bil][ntl - 1]
                              {GRAD_ROW(false, SIM_KLOSS_NMSE), GRAD_ROW(true, SIM_KLOSS_NMSE)},
                              {GRAD_ROW(false, SIM_KLOSS_WEIGHTED_MSE), GRAD_ROW(true, SIM_KLOSS_WEIGHTED_MSE)}};
#undef GRAD_ROW
typedef void (*ApplyFn)(ADev);
const ApplyFn APPLY[3] = {k_koopman_apply<SIM_KLOSS_MSE>, k_koopman_apply<SIM_KLOSS_NMSE>, k_koopman_apply<SIM_KLOSS_WEIGHTED_MSE>};

typedef void (*StatsFn)(KDev, TDev, const double*, int, int, const float*, int, int, int, const int*, int, double*);
const StatsFn STATS[2][4] = {
    {k_koopman_stats<1, false>, k_koopman_stats<2, false>, k_koopman_stats<3, false>, k_koopman_stats<4, false>},
    {k_koopman_stats<1, true>, k_koopman_stats<2, true>, k_koopman_stats<3, true>, k_koopman_stats<4, true>}};

}  // namespace

struct sim_koopman_trainer {
  int device = 0, max_batch = 0, max_slot = 0;
  int loss = SIM_KLOSS_MSE;  // how loss_grad / train_step launch (sim_koopman_trainer_set_loss)
  double* d_stat = nullptr;  // nmse: the waves' sums [max_slot][P][8]; its table follows the count in d_step
  sim_koopman_train_opts opts{};
  ktrain::Plan pl{};
  KDev kd{};
  TDev td{};
  std::vector<int32_t> map;  // host copy of the index map (set_params packs with it)
  double *d_params = nullptr, *d_m = nullptr, *d_v = nullptr, *d_blob = nullptr, *d_ws = nullptr, *d_scr = nullptr;
  int *d_step = nullptr, *d_map = nullptr, *d_gidx = nullptr;
};

#define TCHECK(x)                                                                                  \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) return soarm_set_error(SIM_E_HIP, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

namespace {

int upload_params(sim_koopman_trainer* t, const double* params) {
  std::vector<double> blob;
  ktrain::pack_blob(t->pl, t->map, params, blob);
  TCHECK(hipMemcpy(t->d_params, params, (size_t)t->pl.nparam * sizeof(double), hipMemcpyHostToDevice));
  TCHECK(hipMemcpy(t->d_blob, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice));
  return SIM_OK;
}

int reset_optimizer(sim_koopman_trainer* t) {
  TCHECK(hipMemset(t->d_m, 0, (size_t)t->pl.nparam * sizeof(double)));
  TCHECK(hipMemset(t->d_v, 0, (size_t)t->pl.nparam * sizeof(double)));
  TCHECK(hipMemset(t->d_step, 0, sizeof(int)));
  TCHECK(hipDeviceSynchronize());
  return SIM_OK;
}

int launch(sim_koopman_trainer* t, int n, int N, int T, const float* rows, int ld, int x_off, int u_off,
           const int32_t* traj_idx, int t0, double lr, double* losses, double* grad, int update, void* stream) {
  if (!t) return soarm_set_error(SIM_E_ARG, "null trainer");
  std::string err;
  if (int rc = ktrain::check_step_args(t->pl, t->max_batch, n, N, T, rows, ld, x_off, u_off, traj_idx != nullptr, t0, err))
    return soarm_set_error(rc, (update ? "train_step: " : "loss_grad: ") + err);
  if (n == 0) return SIM_OK;
  const ktrain::Plan& pl = t->pl;
  const int waves = (n + 15) / 16;
  const dim3 grid((waves + ktrain::WAVES - 1) / ktrain::WAVES), block(64 * ktrain::WAVES);
  if (t->loss == SIM_KLOSS_NMSE) {  // the normalisers first: every sample's backward needs the whole batch's
    hipLaunchKernelGGL(STATS[pl.bil][pl.ntl - 1], grid, block, pl.lds_bytes, (hipStream_t)stream, t->kd, t->td, t->d_blob,
                       n, N, rows, ld, x_off, u_off, (const int*)traj_idx, t0, t->d_stat);
    TCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_koopman_nmse_table, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const double*)t->d_stat,
                       reinterpret_cast<double*>(t->d_step) + ktrain::STEP_DOUBLES, waves, pl.P, t->opts.gamma);
    TCHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(GRAD[t->loss][pl.bil][pl.ntl - 1], grid, block, pl.lds_bytes, (hipStream_t)stream, t->kd, t->td,
                     t->d_blob, n, N, rows, ld, x_off, u_off, (const int*)traj_idx, t0, t->d_ws, t->d_scr, t->d_step, update);
  TCHECK(hipGetLastError());
  ADev a{};
  a.nparam = pl.nparam, a.nslot = waves, a.slot_stride = pl.slot_stride, a.n = n, a.P = pl.P, a.xd = pl.xd;
  a.nz = pl.nz, a.npos = pl.npos, a.update = update;
  a.gamma = t->opts.gamma, a.lr = lr, a.beta1 = t->opts.beta1, a.beta2 = t->opts.beta2, a.eps = t->opts.eps;
  a.ws = t->d_ws, a.grad = grad, a.losses = losses, a.params = t->d_params, a.m = t->d_m, a.v = t->d_v;
  a.blob = t->d_blob, a.step = t->d_step, a.map = t->d_map, a.gidx = t->d_gidx;
  hipLaunchKernelGGL(APPLY[t->loss], dim3((pl.nparam + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
  TCHECK(hipGetLastError());
  return SIM_OK;
}

int nparam_of(const sim_koopman_desc* desc, bool bil) {
  if (!desc) return soarm_set_error(SIM_E_ARG, "null argument");
  sim_koopman_train_opts o{};
  o.pre_length = 1, o.npos = 1, o.gamma = 1.0, o.beta1 = 0.9, o.beta2 = 0.999, o.eps = 1e-8;
  sim_koopman_desc d = *desc;
  ktrain::Plan pl;
  std::string err;
  // (the layout does not depend on the options; npos = 1 needs x_dim >= 2, checked by create)
  if (d.x_dim < 2) return soarm_set_error(SIM_E_MODEL, "trainer: x_dim must be >= 2");
  if (int rc = ktrain::make_plan(d, o, pl, err, bil, 0)) return soarm_set_error(rc, err);
  return pl.nparam;
}

int create(const sim_koopman_desc* desc, const double* params, bool bil, int u_z, int max_batch,
           const sim_koopman_train_opts* opts, int device, sim_koopman_trainer** out) {
  if (!desc || !params || !opts || !out) return soarm_set_error(SIM_E_ARG, "null argument");
  *out = nullptr;
  if (int rc = check_struct(opts, "sim_koopman_train_opts")) return rc;
  if (max_batch < 1) return soarm_set_error(SIM_E_ARG, "trainer: max_batch must be >= 1");
  ktrain::Plan pl;
  std::string err;
  if (int rc = ktrain::make_plan(*desc, *opts, pl, err, bil, u_z)) return soarm_set_error(rc, err);
  std::vector<int32_t> map, gidx;
  if (!ktrain::index_map(pl, map) || !ktrain::grad_index(pl, gidx))
    return soarm_set_error(SIM_E_MODEL, "trainer: inconsistent index map");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return soarm_set_error(SIM_E_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return soarm_set_error(SIM_E_ARG, "bad device ordinal");
  TCHECK(hipSetDevice(device));
  sim_koopman_trainer* t = new sim_koopman_trainer;
  t->device = device, t->max_batch = max_batch, t->max_slot = (max_batch + 15) / 16, t->opts = *opts, t->pl = pl;
  t->map = std::move(map);
  KDev& K = t->kd;
  K.xd = pl.xd, K.ud = pl.ud, K.nl = pl.nl, K.nz = pl.nz, K.H = desc->horizon, K.outw = pl.outw;
  for (int l = 0; l < pl.nl; l++) K.ntile[l] = pl.ntile[l], K.ks[l] = pl.ks[l], K.frag[l] = pl.frag[l];
  K.bias = pl.bias, K.gain = pl.enc_total, K.ks_gain = 0, K.total = pl.enc_total, K.gr_ks = 0, K.uclip = desc->u_clip;
  TDev& D = t->td;
  for (int l = 0; l < pl.nl; l++) D.wt[l] = pl.wt[l], D.sw[l] = pl.sw[l], D.sb[l] = pl.sb[l];
  D.ab = pl.ab, D.at = pl.at, D.sA = pl.sA;
  D.slot_stride = pl.slot_stride, D.scr_stride = pl.scr_stride, D.P = pl.P, D.npos = pl.npos, D.gamma = opts->gamma;
  const size_t np = (size_t)pl.nparam * sizeof(double);
  if (hipMalloc(&t->d_params, np) != hipSuccess || hipMalloc(&t->d_m, np) != hipSuccess ||
      hipMalloc(&t->d_v, np) != hipSuccess || hipMalloc(&t->d_step, ktrain::step_bytes(pl)) != hipSuccess ||
      hipMalloc(&t->d_blob, (size_t)pl.blob_total * sizeof(double)) != hipSuccess ||
      hipMalloc(&t->d_map, t->map.size() * sizeof(int32_t)) != hipSuccess ||
      hipMalloc(&t->d_gidx, gidx.size() * sizeof(int32_t)) != hipSuccess ||
      hipMalloc(&t->d_ws, (size_t)t->max_slot * pl.slot_stride * sizeof(double)) != hipSuccess ||
      hipMalloc(&t->d_scr, (size_t)t->max_slot * pl.scr_stride * sizeof(double)) != hipSuccess ||
      hipMalloc(&t->d_stat, ktrain::stat_doubles(pl, t->max_slot) * sizeof(double)) != hipSuccess) {
    sim_koopman_trainer_free(t);
    return soarm_set_error(SIM_E_HIP, "hipMalloc failed");
  }
  int rc = upload_params(t, params);
  if (!rc) rc = reset_optimizer(t);
  if (!rc && hipMemcpy(t->d_map, t->map.data(), t->map.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
    rc = soarm_set_error(SIM_E_HIP, "hipMemcpy failed");
  if (!rc && hipMemcpy(t->d_gidx, gidx.data(), gidx.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
    rc = soarm_set_error(SIM_E_HIP, "hipMemcpy failed");
  // every kernel set_loss can select: the dynamic LDS is raised here, not at the first step
  const void* dyn[4] = {(const void*)GRAD[0][pl.bil][pl.ntl - 1], (const void*)GRAD[1][pl.bil][pl.ntl - 1],
                        (const void*)GRAD[2][pl.bil][pl.ntl - 1], (const void*)STATS[pl.bil][pl.ntl - 1]};
  for (const void* f : dyn)
    if (!rc && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ktrain::LDS_BYTES) != hipSuccess)
      rc = soarm_set_error(SIM_E_HIP, "hipFuncSetAttribute failed");
  if (rc) {
    sim_koopman_trainer_free(t);
    return rc;
  }
  *out = t;
  return SIM_OK;
}

}  // namespace

extern "C" {

int sim_koopman_trainer_nparam(const sim_koopman_desc* desc) { return nparam_of(desc, false); }
int sim_koopman_trainer_nparam_bilinear(const sim_koopman_desc* desc) { return nparam_of(desc, true); }

int sim_koopman_trainer_create(const sim_koopman_desc* desc, const double* params, int max_batch,
                               const sim_koopman_train_opts* opts, int device, sim_koopman_trainer** out) {
  return create(desc, params, false, 0, max_batch, opts, device, out);
}

int sim_koopman_trainer_create_bilinear(const sim_koopman_desc* desc, const double* params, int u_z, int max_batch,
                                        const sim_koopman_train_opts* opts, int device, sim_koopman_trainer** out) {
  return create(desc, params, true, u_z, max_batch, opts, device, out);
}

void sim_koopman_trainer_free(sim_koopman_trainer* t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  (void)hipFree(t->d_params), (void)hipFree(t->d_m), (void)hipFree(t->d_v), (void)hipFree(t->d_step);
  (void)hipFree(t->d_blob), (void)hipFree(t->d_map), (void)hipFree(t->d_gidx), (void)hipFree(t->d_ws), (void)hipFree(t->d_scr);
  (void)hipFree(t->d_stat);
  delete t;
}

int sim_koopman_trainer_set_loss(sim_koopman_trainer* t, int loss) {
  if (!t) return soarm_set_error(SIM_E_ARG, "null trainer");
  if (loss != SIM_KLOSS_MSE && loss != SIM_KLOSS_NMSE && loss != SIM_KLOSS_WEIGHTED_MSE)
    return soarm_set_error(SIM_E_ARG, "set_loss: unknown loss id " + std::to_string(loss));
  if (loss == SIM_KLOSS_WEIGHTED_MSE && t->pl.xd < 4)
    return soarm_set_error(SIM_E_ARG, "set_loss: weighted_mse splits x at column 3 and needs x_dim >= 4");
  t->loss = loss;
  return SIM_OK;
}

int sim_koopman_trainer_get_loss(const sim_koopman_trainer* t) {
  if (!t) return soarm_set_error(SIM_E_ARG, "null trainer");
  return t->loss;
}

int sim_koopman_trainer_get_params(sim_koopman_trainer* t, double* host_params) {
  if (!t || !host_params) return soarm_set_error(SIM_E_ARG, "null argument");
  TCHECK(hipSetDevice(t->device));
  TCHECK(hipDeviceSynchronize());
  TCHECK(hipMemcpy(host_params, t->d_params, (size_t)t->pl.nparam * sizeof(double), hipMemcpyDeviceToHost));
  return SIM_OK;
}

int sim_koopman_trainer_set_params(sim_koopman_trainer* t, const double* host_params, int reset) {
  if (!t || !host_params) return soarm_set_error(SIM_E_ARG, "null argument");
  TCHECK(hipSetDevice(t->device));
  TCHECK(hipDeviceSynchronize());
  if (int rc = upload_params(t, host_params)) return rc;
  if (reset)
    if (int rc = reset_optimizer(t)) return rc;
  TCHECK(hipDeviceSynchronize());
  return SIM_OK;
}

int sim_koopman_loss_grad(sim_koopman_trainer* t, int n, int N, int T, const float* rows, int ld, int x_off, int u_off,
                          const int32_t* traj_idx, int t0, double* losses, double* grad, void* stream) {
  return launch(t, n, N, T, rows, ld, x_off, u_off, traj_idx, t0, 0.0, losses, grad, 0, stream);
}

int sim_koopman_train_step(sim_koopman_trainer* t, int n, int N, int T, const float* rows, int ld, int x_off, int u_off,
                           const int32_t* traj_idx, int t0, double lr, double* losses, void* stream) {
  return launch(t, n, N, T, rows, ld, x_off, u_off, traj_idx, t0, lr, losses, nullptr, 1, stream);
}

}  // extern "C"
