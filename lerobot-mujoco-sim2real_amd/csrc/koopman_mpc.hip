// koopman_mpc.hip — batched Koopman-MPC (include/koopman_mpc.h) on float64 MFMA.
//
// Reference: control/MPC_Controler.py (MPCController: Psi_o :154-167, setup_mpc :65-98,
// setup_delta_mpc :100-141, get_control :143-152) and the tracking loop Koopman_MPC.py:197-222,
// one env, casadi/IPOPT, float64.  Here one wave serves 16 envs:
//
//   encoder  z = [x, MLP(x)]  (models/KoopmanBase.py:45-47): every Linear layer is a chain of
//            v_mfma_f64_16x16x4_f64 with the 16 envs on the MFMA's N side and the layer's output
//            rows in 16-row tiles.  The f64 MFMA's C/D layout (lane l, register r holds row
//            (l >> 4) + 4r, column l & 15) is exactly its B-operand layout for the k-step that
//            covers those 4 rows (B: lane l holds row k = l >> 4 of the step, column l & 15), so a
//            layer's output tile T register r IS the next layer's B operand for k-step 4T + r:
//            activations never leave registers, no LDS round trip, no shuffles.
//   control  u0 = ff + [Gz | Gu] [z0; u_prev] is one more 16-row MFMA tile over the same B
//            operands (z0's tiles, then u_prev), with ff as the accumulator's initial value.
//
// The weights of every layer are stored by the host in MFMA fragment order (tile, k-step, lane),
// so a workgroup stages them into LDS with linear 16-B copies and every A-operand read is a
// conflict-free, lane-contiguous ds_read_b64.  4096 envs = 256 waves = 64 workgroups of 4 waves.
//
// This unit: the handle (create / free), k_encode, k_feedforward and k_mpc_step.  The DBKN steps are
// koopman_bilinear.hip, open-loop prediction koopman_predict.hip, the DKUC step with input limits
// koopman_box.hip; koopman_internal.h is what they share.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "koopman_internal.h"

namespace {

// Psi_o for m states: z [nz][m]
template <int NTL>
__global__ __launch_bounds__(256) void k_encode(KDev K, const double* __restrict__ frag, int m,
                                                const float* __restrict__ x, double* __restrict__ z) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  stage(lds, frag, K.total);
  const int lane = threadIdx.x & 63, kq = lane >> 4;
  const int e = lane_env(lane);
  const bool live = e < m;  // every lane runs the MFMAs (they need the full wave)
  double xb[2];
  d4 act[KT];
  load_lifted<NTL>(K, lds, lane, m, e, live, x, nullptr, xb, act);
  if (!live) return;
#pragma unroll
  for (int s = 0; s < 2; s++)
    if (4 * s + kq < K.xd) z[(size_t)(4 * s + kq) * m + e] = xb[s];
#pragma unroll
  for (int T = 0; T < NTL; T++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = 16 * T + kq + 4 * r;
      if (row < K.outw) z[(size_t)(K.xd + row) * m + e] = act[T][r];
    }
}

// u0 = ff + Gz z0 + Gu u_prev (z0 = Psi_o(x) unless given); u_prev <- u0; action = clip(u0)
template <int NTL>
__global__ __launch_bounds__(256) void k_mpc_step(KDev K, const double* __restrict__ frag, int n,
                                                  const float* __restrict__ x, const double* __restrict__ z0,
                                                  const double* __restrict__ ff, double* __restrict__ uprev,
                                                  float* __restrict__ action) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  stage(lds, frag, K.total);
  const int lane = threadIdx.x & 63, kq = lane >> 4;
  const int e = lane_env(lane);
  const bool live = e < n;
  // issued before the encoder: consumed after it
  double up[2], f0[4];
  load_uprev(K, uprev, n, e, live, kq, up);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = kq + 4 * r;
    f0[r] = (live && ff && row < K.ud) ? ff[(size_t)row * n + e] : 0.0;
  }
  double xb[2];
  d4 act[KT];
  load_lifted<NTL>(K, lds, lane, n, e, live, x, z0, xb, act);
  // one output tile: rows = u index (kq + 4r), columns = envs; ff is the initial accumulator
  d4 u = {f0[0], f0[1], f0[2], f0[3]};
  const double* G = lds + K.gain + lane;
  u = mfma(G[0], xb[0], u);
  u = mfma(G[64], xb[1], u);
#pragma unroll
  for (int s = 0; s < 4 * NTL; s++) u = mfma(G[(2 + s) * 64], act[s >> 2][s & 3], u);
#pragma unroll
  for (int s = 0; s < 2; s++) u = mfma(G[(2 + 4 * NTL + s) * 64], up[s], u);
  if (!live) return;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = kq + 4 * r;
    if (row < K.ud) {
      uprev[(size_t)row * n + e] = u[r];
      action[(size_t)e * K.ud + row] = (float)fmin(fmax(u[r], -K.uclip), K.uclip);
    }
  }
}

// ff[f][u][e] = sum_{t<H} Gr_t zref[f+1+t][:][e]  (zero past nref); FR frames per workgroup.
// gr_ks is a multiple of 4 (zero fragments past K = H nz): 4 static accumulator chains.
constexpr int FR = 16;
__global__ __launch_bounds__(256) void k_feedforward(KDev K, const double* __restrict__ grfrag, int nframe,
                                                     int nref, int n, const double* __restrict__ zref,
                                                     double* __restrict__ ff) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  stage(lds, grfrag, K.gr_ks * 64);
  const int lane = threadIdx.x & 63, kq = lane >> 4;
  const int e = lane_env(lane);
  const bool live = e < n;
  const int kk = K.H * K.nz;
  const int f1 = min(nframe, (int)(blockIdx.y + 1) * FR);
  for (int f = blockIdx.y * FR; f < f1; f++) {
    d4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    // this lane's reference element of k-step s: g = 4s + kq -> (t, j) = divmod(g, nz)
    int t = 0, j = kq;
    while (j >= K.nz) j -= K.nz, t++;
    for (int s0 = 0; s0 < K.gr_ks; s0 += 4) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int g = 4 * (s0 + q) + kq;
        const int fr = f + 1 + t;
        const double b = (live && g < kk && fr < nref) ? zref[((size_t)fr * K.nz + j) * n + e] : 0.0;
        acc[q] = mfma(lds[(s0 + q) * 64 + lane], b, acc[q]);
        j += 4;
        while (j >= K.nz) j -= K.nz, t++;
      }
    }
    if (live) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = kq + 4 * r;
        if (row < K.ud) ff[((size_t)f * K.ud + row) * n + e] = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
      }
    }
  }
}

typedef void (*EncodeFn)(KDev, const double*, int, const float*, double*);
typedef void (*StepFn)(KDev, const double*, int, const float*, const double*, const double*, double*, float*);
const EncodeFn ENCODE[4] = {k_encode<1>, k_encode<2>, k_encode<3>, k_encode<4>};
const StepFn STEP[4] = {k_mpc_step<1>, k_mpc_step<2>, k_mpc_step<3>, k_mpc_step<4>};

}  // namespace

extern "C" {

int sim_koopman_create(const sim_koopman_desc* d, const double* weights, const double* gain, int device,
                       sim_koopman** out) {
  if (!d || !weights || !gain || !out) return soarm_set_error(SIM_E_ARG, "null argument");
  *out = nullptr;
  std::string err;
  if (int rc = klayout::check_desc(*d, err)) return soarm_set_error(rc, err);
  const klayout::Encoder e = klayout::encoder(*d);
  const int ud = e.ud, nl = e.nl;
  KDev K{};
  K.xd = e.xd, K.ud = ud, K.nl = nl, K.H = d->horizon, K.outw = e.outw, K.nz = e.nz;
  K.uclip = d->u_clip;
  if (K.H * K.nz > 1024) return soarm_set_error(SIM_E_MODEL, "horizon * nz must be <= 1024");
  for (int l = 0; l < nl; l++) K.ntile[l] = e.ntile[l], K.ks[l] = e.ks[l], K.frag[l] = e.frag[l];
  K.bias = e.bias;
  K.gain = e.total;  // [Gz | Gu] behind the encoder
  K.ks_gain = klayout::ks_zu(e);
  K.total = K.gain + K.ks_gain * 64;
  K.gr_ks = 4 * ((K.H * K.nz + 15) / 16);  // a multiple of 4 k-steps (zero fragments past H nz)
  if ((size_t)K.total * 8 > KOOPMAN_LDS_BYTES || (size_t)K.gr_ks * 64 * 8 > KOOPMAN_LDS_BYTES)
    return soarm_set_error(SIM_E_MODEL, "controller does not fit in LDS");

  // host packing: fragment order, zero padding
  std::vector<double> blob(K.total, 0.0), gr((size_t)K.gr_ks * 64, 0.0);
  const double* w = weights;
  for (int l = 0; l < nl; l++) {
    const int in = d->width[l], ou = d->width[l + 1];
    klayout::fill_frag(&blob[K.frag[l]], K.ntile[l], K.ks[l],
                       [&](int row, int col) { return (row < ou && col < in) ? w[(size_t)row * in + col] : 0.0; });
    w += (size_t)ou * in;
    for (int r = 0; r < ou; r++) blob[K.bias + l * SIM_KMAXW + r] = w[r];
    w += ou;
  }
  // gain columns: [Gr (H*nz) | Gz (nz) | Gu (ud)]; one tile of rows (the inputs); the step kernel's k
  // order is the padded one, [x (8) | features | u_prev (8)], the feedforward's is Gr's own
  const int hz = K.H * K.nz, gcols = hz + K.nz + ud;
  klayout::fill_frag(&blob[K.gain], 1, K.ks_gain, [&](int row, int kk) {
    const int c = klayout::zu_col(e, kk, hz);
    return (row < ud && c >= 0) ? gain[(size_t)row * gcols + c] : 0.0;
  });
  klayout::fill_frag(gr.data(), 1, K.gr_ks,
                     [&](int row, int c) { return (row < ud && c < hz) ? gain[(size_t)row * gcols + c] : 0.0; });

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return soarm_set_error(SIM_E_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return soarm_set_error(SIM_E_ARG, "bad device ordinal");
  KCHECK(hipSetDevice(device));
  sim_koopman* k = new sim_koopman;
  k->device = device, k->desc = *d, k->kd = K;
  if (hipMalloc(&k->d_frag, blob.size() * sizeof(double)) != hipSuccess ||
      hipMalloc(&k->d_grfrag, gr.size() * sizeof(double)) != hipSuccess) {
    sim_koopman_free(k);
    return soarm_set_error(SIM_E_HIP, "hipMalloc failed");
  }
  KCHECK(hipMemcpy(k->d_frag, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice));
  KCHECK(hipMemcpy(k->d_grfrag, gr.data(), gr.size() * sizeof(double), hipMemcpyHostToDevice));
  const int ti = K.ntile[nl - 1] - 1;
  KCHECK(koopman_raise_lds((const void*)ENCODE[ti]));
  KCHECK(koopman_raise_lds((const void*)STEP[ti]));
  KCHECK(koopman_raise_lds((const void*)k_feedforward));
  *out = k;
  return SIM_OK;
}

void sim_koopman_free(sim_koopman* k) {
  if (!k) return;
  (void)hipSetDevice(k->device);
  (void)hipFree(k->d_frag);
  (void)hipFree(k->d_grfrag);
  (void)hipFree(k->d_A);
  (void)hipFree(k->d_B);
  (void)hipFree(k->d_Hh);
  (void)hipFree(k->d_model);
  koopman_box_release(k->box);
  delete k;
}

int sim_koopman_encode(sim_koopman* k, int m, const float* x, double* z, void* stream) {
  if (!k || !x || !z || m < 0) return soarm_set_error(SIM_E_ARG, "bad argument");
  if (m == 0) return SIM_OK;
  hipLaunchKernelGGL(ENCODE[k->kd.ntile[k->kd.nl - 1] - 1], dim3((m + 63) / 64), dim3(256),
                     k->kd.total * sizeof(double), (hipStream_t)stream, k->kd, k->d_frag, m, x, z);
  KCHECK(hipGetLastError());
  return SIM_OK;
}

int sim_koopman_feedforward(sim_koopman* k, int nframe, int nref, int n, const double* zref, double* ff,
                            void* stream) {
  if (!k || !zref || !ff || nframe < 0 || nref < 0 || n < 0) return soarm_set_error(SIM_E_ARG, "bad argument");
  if (nframe == 0 || n == 0) return SIM_OK;
  hipLaunchKernelGGL(k_feedforward, dim3((n + 63) / 64, (nframe + FR - 1) / FR), dim3(256),
                     k->kd.gr_ks * 64 * sizeof(double), (hipStream_t)stream, k->kd, k->d_grfrag, nframe, nref, n,
                     zref, ff);
  KCHECK(hipGetLastError());
  return SIM_OK;
}

int sim_koopman_mpc_step(sim_koopman* k, int n, const float* x, const double* z0, const double* ff,
                         double* u_prev, float* action, void* stream) {
  if (!k || (!x && !z0) || !u_prev || !action || n < 0) return soarm_set_error(SIM_E_ARG, "bad argument");
  if (n == 0) return SIM_OK;
  hipLaunchKernelGGL(STEP[k->kd.ntile[k->kd.nl - 1] - 1], dim3((n + 63) / 64), dim3(256),
                     k->kd.total * sizeof(double), (hipStream_t)stream, k->kd, k->d_frag, n, x, z0, ff, u_prev,
                     action);
  KCHECK(hipGetLastError());
  return SIM_OK;
}

}  // extern "C"
