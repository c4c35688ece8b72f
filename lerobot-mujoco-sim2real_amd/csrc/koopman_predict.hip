// koopman_predict.hip — open-loop prediction of a Koopman model (include/koopman_mpc.h:
// sim_koopman_set_model, sim_koopman_predict) on float64 MFMA, over the controller's encoder.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "koopman_internal.h"

namespace {

// ---------------------------------------------------------------- open-loop prediction
// The multi-step prediction error of a Koopman model (evaluate(), train.py:35-87, over
// pred_and_eval_loss_old / _new, models/losses.py:132-215): x^_0 = x_0, z = Psi(x_0); per step
// z <- A z + (B + sum_j z_j Hhat_j) u_t, x^_{t+1} = z[:x_dim] (the frozen decoder lC = [I | 0]),
// and with RL ("relift", the _old form evaluate() runs) z <- Psi(x^_{t+1}).  One wave serves 16
// trajectories for all T steps of one launch; the lifted state never leaves registers:
//   z is held as the B operands it was produced as: xb[2] (the x rows padded to 8) and act[KT] (the
//     feature tiles).  [A | B] is packed by the host with one output tile for the x rows and NTL
//     output feature tiles over the k order [x (8) | features (16 NTL) | u (8)] -- the gain
//     fragments' order -- so a step's output tiles ARE the next step's B operands (the C/D layout
//     is the B layout, as between the encoder's layers), and B u_t is two more k-steps.  With RL
//     only the x tile is computed: the features come from the encoder.
//   DBKN: the Kronecker index is taken u-major, k = c (8 + 16 NTL) + j, so for a fixed input c the B
//     operand is u_c(env) times z's own B operand: one multiply, no cross-lane traffic.  The Hhat
//     fragments [tile][c][k-step][lane] (77 KB at the reference shape) do not fit LDS beside the
//     encoder: they are read from global memory (lane-contiguous, L2-resident), the x tile's first.
//   u_{t+1} and the label x_{t+2} are loaded before step t's MFMA chain.
//   err: each lane sums |x^ - x| of its two rows over t (rows < npos and rows >= npos apart); the
//     4 lanes of a trajectory are added once at the end (xor 16, xor 32): a fixed order, no atomics.
// Tail lanes (e >= n) run the MFMAs on zero inputs (their columns are independent) and never
// load or store.  The workgroup is 4 waves (1 or 2 on request: blockDim), see sim_koopman_set_model.

// every input of this lane's trajectory (DBKN: u_c scales z's B operands)
DEVI void load_all(const float* __restrict__ p, bool ok, int dim, double out[SIM_KMAXU]) {
#pragma unroll
  for (int c = 0; c < SIM_KMAXU; c++) out[c] = (ok && c < dim) ? (double)p[c] : 0.0;
}

template <int NTL, bool RL>
__global__ __launch_bounds__(256) void k_predict(KDev K, PDev P, const double* __restrict__ frag,
                                                 const double* __restrict__ mfrag, int n, int T,
                                                 const float* __restrict__ rows, int ld, int x_off, int u_off,
                                                 int npos, double* __restrict__ pred, double* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  stage(lds, frag, K.total);
  stage(lds + P.afrag, mfrag, P.acount);
  constexpr int NT = RL ? 1 : 1 + NTL;  // output tiles of a step
  const int lane = threadIdx.x & 63, kq = lane >> 4;
  const int e = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16 + (lane & 15);
  const bool live = e < n;
  const bool bl = P.bilinear != 0;
  const size_t ts = (size_t)n * ld;  // floats between the rows of t and t + 1
  const float* __restrict__ r0 = rows + (live ? (size_t)e * ld : 0);
  double xb[2], ub[2], lab[2], uc[SIM_KMAXU];
  load_pair(r0 + x_off, live, K.xd, kq, xb);
  load_pair(r0 + u_off, live && T > 0, K.ud, kq, ub);
  load_pair(r0 + ts + x_off, live && T > 0, K.xd, kq, lab);
  load_all(r0 + u_off, live && bl && T > 0, K.ud, uc);
  d4 act[KT];
  encode<NTL>(K, lds, lane, xb, act);
  if (live && pred) {
#pragma unroll
    for (int s = 0; s < 2; s++)
      if (4 * s + kq < K.xd) pred[(size_t)e * K.xd + 4 * s + kq] = xb[s];
  }
  double ep = 0.0, ea = 0.0;
  const double* Am = lds + P.afrag + lane;
  const double* Hm = mfrag + P.acount + lane;
  for (int t = 0; t < T; t++) {
    // the next step's inputs and label, in flight during this step's MFMAs
    double nub[2], nlab[2], nuc[SIM_KMAXU];
    const float* __restrict__ r1 = r0 + (size_t)(t + 1) * ts;
    load_pair(r1 + u_off, live && t + 1 < T, K.ud, kq, nub);
    load_all(r1 + u_off, live && bl && t + 1 < T, K.ud, nuc);
    load_pair(r1 + ts + x_off, live && t + 2 <= T, K.xd, kq, nlab);
    // z' = [A | B] [z; u]: tile 0 = the x rows, tiles 1.. = the features
    d4 zn[NT];
#pragma unroll
    for (int q = 0; q < NT; q++) zn[q] = d4{0.0, 0.0, 0.0, 0.0};
    d4 zo = {0.0, 0.0, 0.0, 0.0};  // RL: the x tile's odd k-steps (two chains instead of one)
#pragma unroll
    for (int s = 0; s < 2 + 4 * NTL + 2; s++) {
      const double b = s < 2 ? xb[s] : (s < 2 + 4 * NTL ? act[(s - 2) >> 2][(s - 2) & 3] : ub[s - 2 - 4 * NTL]);
      if (RL && (s & 1)) {
        zo = mfma(Am[s * 64], b, zo);
      } else {
#pragma unroll
        for (int q = 0; q < NT; q++) zn[q] = mfma(Am[(q * P.ks + s) * 64], b, zn[q]);
      }
    }
    if (RL) zn[0] += zo;
    if (bl) {  // + sum_c sum_j Hhat[j][.][c] (u_c z_j): accumulators of their own, added at the end
      d4 hn[NT];
#pragma unroll
      for (int q = 0; q < NT; q++) hn[q] = d4{0.0, 0.0, 0.0, 0.0};
      d4 ho = {0.0, 0.0, 0.0, 0.0};
      // one input per iteration (not unrolled: the fragment loads in flight stay those of one c)
#pragma unroll 1
      for (int c = 0; c < K.ud; c++) {
        double ucv = 0.0;
#pragma unroll
        for (int c2 = 0; c2 < SIM_KMAXU; c2++) ucv = c == c2 ? uc[c2] : ucv;
        const double* Hc = Hm + (size_t)c * P.hks * 64;
#pragma unroll
        for (int s = 0; s < 2 + 4 * NTL; s++) {
          const double b = ucv * (s < 2 ? xb[s] : act[(s - 2) >> 2][(s - 2) & 3]);
          if (RL && (s & 1)) {
            ho = mfma(Hc[s * 64], b, ho);
          } else {
#pragma unroll
            for (int q = 0; q < NT; q++) hn[q] = mfma(Hc[((size_t)q * K.ud * P.hks + s) * 64], b, hn[q]);
          }
        }
      }
      if (RL) hn[0] += ho;
#pragma unroll
      for (int q = 0; q < NT; q++) zn[q] += hn[q];
    }
    // x^_{t+1} = rows 0..7 of tile 0 (registers 0, 1: the B operands of k-steps 0, 1); rows >= x_dim
    // are exact zeros (zero fragment rows) and so are their labels
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const int row = 4 * s + kq;
      const double d = fabs(zn[0][s] - lab[s]);
      if (row < npos) ep += d; else ea += d;
      if (live && pred && row < K.xd) pred[((size_t)(t + 1) * n + e) * K.xd + row] = zn[0][s];
      xb[s] = zn[0][s];
      ub[s] = nub[s], lab[s] = nlab[s];
    }
#pragma unroll
    for (int c = 0; c < SIM_KMAXU; c++) uc[c] = nuc[c];
    if (RL) {
      encode<NTL>(K, lds, lane, xb, act);  // pred_and_eval_loss_old: x0 = x1_pred is lifted again
    } else {
#pragma unroll
      for (int q = 0; q < NTL; q++) act[q] = zn[RL ? 0 : 1 + q];
    }
  }
  // the 4 lanes (kq) of a trajectory: (k0 + k1) + (k2 + k3) in every lane
  ep += __shfl_xor(ep, 16), ea += __shfl_xor(ea, 16);
  ep += __shfl_xor(ep, 32), ea += __shfl_xor(ea, 32);
  if (live && err && kq == 0) err[e] = ep, err[(size_t)n + e] = ea;
}

typedef void (*PredictFn)(KDev, PDev, const double*, const double*, int, int, const float*, int, int, int, int,
                          double*, double*);
const PredictFn PREDICT[4][2] = {{k_predict<1, false>, k_predict<1, true>}, {k_predict<2, false>, k_predict<2, true>},
                                 {k_predict<3, false>, k_predict<3, true>}, {k_predict<4, false>, k_predict<4, true>}};

}  // namespace

extern "C" {

int sim_koopman_set_model(sim_koopman* k, const double* A, const double* B, const double* Hhat) {
  if (!k || !A || !B) return soarm_set_error(SIM_E_ARG, "null argument");
  const KDev& K = k->kd;
  const klayout::Encoder e = koopman_layout_of(K);
  const int nz = K.nz, ud = K.ud, ntl = e.ntl;
  PDev P{};
  P.afrag = K.total;
  P.ks = klayout::ks_zu(e);
  P.hks = klayout::ks_z(e);
  P.acount = (1 + ntl) * P.ks * 64;
  P.bilinear = Hhat ? 1 : 0;
  k->model_state = 0;
  if ((size_t)(K.total + P.acount) * 8 > KOOPMAN_LDS_BYTES) {
    k->model_state = 2;
    return soarm_set_error(SIM_E_MODEL, "open-loop prediction: the encoder and [A | B] fragments (" +
                                            std::to_string((size_t)(K.total + P.acount) * 8) +
                                            " bytes) do not fit the 160 KiB of LDS");
  }
  // rows: tile 0 = the x rows, tile 1 + T = features 16 T ..; k: the B operands' order [x | features | u]
  auto zrow = [&](int row) { return klayout::z_of_row(e, row >> 4, row & 15); };
  const size_t hcount = Hhat ? (size_t)(1 + ntl) * ud * P.hks * 64 : 0;
  std::vector<double> blob((size_t)P.acount + hcount, 0.0);
  klayout::fill_frag(blob.data(), 1 + ntl, P.ks, [&](int row, int kk) {
    const int i = zrow(row), j = klayout::z_of_k(e, kk), c = klayout::u_of_k(e, kk);
    if (i >= 0 && c >= 0) return B[(size_t)i * ud + c];
    return (i >= 0 && j >= 0) ? A[(size_t)i * nz + j] : 0.0;
  });
  if (Hhat)  // Hhat [j][i][c]: the coefficient of z_j u_c in row i
    for (int tile = 0; tile <= ntl; tile++)
      for (int c = 0; c < ud; c++)
        klayout::fill_frag(blob.data() + P.acount + ((size_t)tile * ud + c) * P.hks * 64, 1, P.hks, [&](int r, int kk) {
          const int i = klayout::z_of_row(e, tile, r), j = klayout::z_of_k(e, kk);
          return (i >= 0 && j >= 0) ? Hhat[((size_t)j * nz + i) * ud + c] : 0.0;
        });
  KCHECK(hipSetDevice(k->device));
  (void)hipFree(k->d_model);
  k->d_model = nullptr;
  KCHECK(hipMalloc(&k->d_model, blob.size() * sizeof(double)));
  KCHECK(hipMemcpy(k->d_model, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice));
  for (int rl = 0; rl < 2; rl++) KCHECK(koopman_raise_lds((const void*)PREDICT[ntl - 1][rl]));
  // waves per workgroup: 4, as the other kernels here.  Measured at 4096 trajectories x 199 steps
  // (DESIGN.md §4): 1, 2 and 4 run within 1% of each other with relift (a wave is bound by its own
  // SIMD's f64 MFMA rate wherever it runs) and 4 is 5% ahead without (a quarter of the staging).
  // SOARM_KPREDICT_WAVES = 1 | 2 | 4 overrides it (tools/bench_koopman_predict.py measures all three)
  k->wpw = 4;
  if (const char* w = getenv("SOARM_KPREDICT_WAVES")) {
    const int v = atoi(w);
    if (v == 1 || v == 2 || v == 4) k->wpw = v;
  }
  k->pd = P;
  k->model_state = 1;
  return SIM_OK;
}

int sim_koopman_predict(sim_koopman* k, int n, int T, const float* rows, int ld, int x_off, int u_off, int relift,
                        int npos, double* pred, double* err, void* stream) {
  if (!k || !rows) return soarm_set_error(SIM_E_ARG, "null argument");
  const KDev& K = k->kd;
  if (n < 0 || T < 0) return soarm_set_error(SIM_E_ARG, "predict: n and T must be >= 0");
  if (npos < 0 || npos > K.xd) return soarm_set_error(SIM_E_ARG, "predict: npos must be in 0..x_dim");
  if (ld < 1 || x_off < 0 || u_off < 0 || (long long)x_off + K.xd > ld || (long long)u_off + K.ud > ld)
    return soarm_set_error(SIM_E_ARG, "predict: the x / u columns run past the row length ld");
  if (k->model_state == 2) return soarm_set_error(SIM_E_MODEL, "predict: sim_koopman_set_model refused this model (LDS)");
  if (k->model_state != 1) return soarm_set_error(SIM_E_ARG, "sim_koopman_set_model was not called");
  if (n == 0) return SIM_OK;
  const int waves = (n + 15) / 16, wpw = k->wpw;  // one wave per 16 trajectories
  hipLaunchKernelGGL(PREDICT[K.ntile[K.nl - 1] - 1][relift ? 1 : 0], dim3((waves + wpw - 1) / wpw), dim3(64 * wpw),
                     (size_t)(K.total + k->pd.acount) * sizeof(double), (hipStream_t)stream, K, k->pd, k->d_frag,
                     k->d_model, n, T, rows, ld, x_off, u_off, npos, pred, err);
  KCHECK(hipGetLastError());
  return SIM_OK;
}

}  // extern "C"
