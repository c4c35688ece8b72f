// koopman_frag.h — the f64-MFMA device helpers shared by the Koopman units (koopman_mpc.hip,
// koopman_bilinear.hip, koopman_predict.hip, koopman_box.hip, koopman_train.hip): the device-side
// layout of an encoder's fragment blob, the MFMA wrapper, LDS staging, the register-chained encoder
// and the loads of a control step's operands.  The host-side layout is koopman_layout.h's.
//
// Layouts (v_mfma_f64_16x16x4_f64, one wave, samples on the N side):
//   A operand  lane l holds A[row l & 15][k l >> 4] of the k-step;
//   B operand  lane l holds B[k l >> 4][column l & 15];
//   C/D        lane l, register r holds row (l >> 4) + 4 r, column l & 15.
// The C/D layout of a 16-row tile is the B layout of the 4 k-steps that cover those rows (register r
// = k-step r), so an output tile feeds the next product without leaving registers.
#ifndef KOOPMAN_FRAG_H
#define KOOPMAN_FRAG_H

#include <hip/hip_runtime.h>

#include "../../include/koopman_mpc.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int KT = SIM_KMAXW / 16;  // 16-row tiles of a layer's output (4)

// device-side layout of one controller (kernel argument; offsets in doubles into the fragment blob)
struct KDev {
  int xd, ud, nl, nz, H, outw;
  int ntile[SIM_KMAXLAYER];  // 16-row output tiles of layer l
  int ks[SIM_KMAXLAYER];     // 4-deep k-steps of layer l (2 for layer 0: x padded to 8)
  int frag[SIM_KMAXLAYER];   // A fragments of layer l: [ntile][ks][64]
  int bias;                  // [nl][64]
  int gain;                  // [Gz | Gu] fragments: [ks_gain][64], rows = u (one tile)
  int ks_gain;               // 2 (x) + 4 * ntile[nl-1] (features) + 2 (u_prev)
  int total;                 // doubles staged in LDS by k_mpc_step / k_encode
  int gr_ks;                 // Gr fragments (feedforward): [gr_ks][64], K = H * nz
  double uclip;
};

#define DEVI __device__ __forceinline__

DEVI d4 mfma(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// stage `count` doubles global -> LDS (16-B copies; count is a multiple of 2, offsets 16-B aligned)
DEVI void stage(double* lds, const double* __restrict__ g, int count) {
  const double2* src = reinterpret_cast<const double2*>(g);
  double2* dst = reinterpret_cast<double2*>(lds);
  for (int i = threadIdx.x; i < count / 2; i += blockDim.x) dst[i] = src[i];
  __syncthreads();
}

// LDS written by other lanes of this wave is read after this (the wave's LDS operations complete
// in order once issued; the fence keeps the compiler from moving them across)
DEVI void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the encoder for this wave's 16 envs: xb = x as the B operand of k-steps 0..1 (lane: row
// 4s + (lane >> 4), env lane & 15); returns the last layer's output tiles in `act`.
// Shapes are static so every MFMA, LDS offset and register index is a compile-time constant:
// layer 0 is 4 tiles x 2 k-steps (x padded to 8 rows), hidden layers 4 tiles x 16 k-steps
// (widths zero-padded to 64), the last layer NTL tiles x 16 k-steps.
template <int NTL>
DEVI void encode(const KDev& K, const double* lds, int lane, const double xb[2], d4 (&act)[KT]) {
  const int kq = lane >> 4;
  d4 acc[KT];
  {  // layer 0 (ReLU: nl >= 2)
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
      for (int r = 0; r < 4; r++) act[T][r] = fmax(acc[T][r], 0.0);
  }
  for (int l = 1; l < K.nl - 1; l++) {  // hidden layers: one static body, runtime count
    const double* A = lds + K.frag[l] + lane;
    const double* bias = lds + K.bias + l * SIM_KMAXW;
#pragma unroll
    for (int T = 0; T < KT; T++)
#pragma unroll
      for (int r = 0; r < 4; r++) acc[T][r] = bias[16 * T + kq + 4 * r];
    // k-steps outer, tiles inner: KT independent accumulator chains
#pragma unroll
    for (int s = 0; s < 4 * KT; s++)
#pragma unroll
      for (int T = 0; T < KT; T++) acc[T] = mfma(A[(T * 16 + s) * 64], act[s >> 2][s & 3], acc[T]);
#pragma unroll
    for (int T = 0; T < KT; T++)
#pragma unroll
      for (int r = 0; r < 4; r++) act[T][r] = fmax(acc[T][r], 0.0);
  }
  {  // last layer: no ReLU (models/KoopmanBase.py:20-25)
    const double* A = lds + K.frag[K.nl - 1] + lane;
    const double* bias = lds + K.bias + (K.nl - 1) * SIM_KMAXW;
#pragma unroll
    for (int T = 0; T < NTL; T++)
#pragma unroll
      for (int r = 0; r < 4; r++) acc[T][r] = bias[16 * T + kq + 4 * r];
#pragma unroll
    for (int s = 0; s < 4 * KT; s++)
#pragma unroll
      for (int T = 0; T < NTL; T++) acc[T] = mfma(A[(T * 16 + s) * 64], act[s >> 2][s & 3], acc[T]);
#pragma unroll
    for (int T = 0; T < KT; T++) act[T] = T < NTL ? acc[T] : d4{0, 0, 0, 0};
  }
}

// row 4 s + kq (s = 0, 1) of a float32 row p[0 .. dim), widened, as a B operand pair
DEVI void load_pair(const float* __restrict__ p, bool ok, int dim, int kq, double out[2]) {
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const int row = 4 * s + kq;
    out[s] = (ok && row < dim) ? (double)p[row] : 0.0;
  }
}

DEVI double clipd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// ---- the kernels of 4 waves x 16 envs (k_encode, k_mpc_step, k_feedforward, k_box_step)
// this lane's env: column lane & 15 of its wave's 16
DEVI int lane_env(int lane) { return blockIdx.x * 64 + (threadIdx.x >> 6) * 16 + (lane & 15); }

// rows 4 s + kq of u_prev [ud][n] as the B operands of the last two k-steps
DEVI void load_uprev(const KDev& K, const double* __restrict__ uprev, int n, int e, bool live, int kq, double up[2]) {
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const int row = 4 * s + kq;
    up[s] = (live && row < K.ud) ? uprev[(size_t)row * n + e] : 0.0;
  }
}

// the lifted state of this lane's env as B operands, xb (the x rows) and act (the feature tiles): z0 [nz][n]
// where it is given (get_control(p), MPC_Controler.py:143), else Psi_o(x) by the encoder (x [n][xd] f32,
// widened as torch.DoubleTensor(obs); the encoder's fragments staged in lds)
template <int NTL>
DEVI void load_lifted(const KDev& K, const double* lds, int lane, int n, int e, bool live,
                      const float* __restrict__ x, const double* __restrict__ z0, double xb[2], d4 (&act)[KT]) {
  const int kq = lane >> 4;
  if (z0) {
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const int row = 4 * s + kq;
      xb[s] = (live && row < K.xd) ? z0[(size_t)row * n + e] : 0.0;
    }
#pragma unroll
    for (int T = 0; T < KT; T++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = 16 * T + kq + 4 * r;
        act[T][r] = (live && T < NTL && row < K.outw) ? z0[(size_t)(K.xd + row) * n + e] : 0.0;
      }
  } else {
    load_pair(x + (size_t)e * K.xd, live, K.xd, kq, xb);  // (a tail lane's address is formed, never read)
    encode<NTL>(K, lds, lane, xb, act);
  }
}

}  // namespace
#endif  // KOOPMAN_FRAG_H
