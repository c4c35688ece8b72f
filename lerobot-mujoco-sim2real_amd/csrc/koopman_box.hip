// koopman_box.hip — the DKUC control step with input limits (include/koopman_mpc.h:
// sim_koopman_set_box, sim_koopman_box_step): one box-constrained QP per env and frame, float64 MFMA.
//
// The reference (control/MPC_Controler.py:65-152) solves the horizon QP without bounds and clips the
// first move; k_mpc_step is that.  Here the plan itself respects the limit.  In the model inputs w
// (N = H nu; 'delta_mpc': w_t = u_prev + sum_{i<=t} du_i, 'mpc': w_t = v_t) the cost is
// 1/2 w'Pw - g'w with P = 2 (q Gam'Gam + r D'D | r I) the same for every env and frame, and the
// limits are simple bounds lo <= w <= hi (+-u_max; 'mpc': block 0 shifted by -u_prev, because
// v_0 + u_prev is what is applied).  One wave serves 16 envs, envs on the MFMA's N side, the plan in
// 16-row tiles whose C/D layout is the B layout of the next product (koopman_frag.h), so the
// iterate never leaves registers:
//
//   wu = K [window; z0; u_prev]   the unconstrained minimiser P^-1 g, K [N][H nz + nz + nu] from the
//                                 host; its fragments (184 KB at the reference shape) are read from
//                                 global memory, lane-contiguous and L2-resident.  z0 = Psi_o(x) by
//                                 the register-chained encoder unless given.
//   wu in the box  ->  done, iters 0.  When that holds for the whole workgroup nothing else is
//                                 staged; a wave whose 16 envs are interior leaves before the loop.
//   else ADMM on  min 1/2 x'Px - g'x + I_box(z), x = z, scaled dual y, over-relaxed (alpha 1.6):
//       x = wu + Mrho (z - y - wu)        Mrho = rho (P + rho I)^-1, rho = sqrt(lmin lmax)
//       xh = alpha x + (1 - alpha) z;  z <- clip(xh + y);  y <- y + xh - z
//     and the stop test of the ABI on the projected iterate z: grad = P (z - wu) (= P z - g: g is
//     never formed), res = z - clip(z - grad / Lhat), ||res||_inf <= tol.  Two N x N by N x 16
//     products per iteration, P and Mrho staged in LDS over the encoder's fragments (dead by then).
//     Start: z = clip(wu), or (warm) clip(plan) where that is provably the closer start, res(clip(plan))
//     < res(clip(wu)) mu / (4 Lhat); y = -grad / rho where z sits on a bound the gradient pushes
//     against, else 0: the multiplier estimate of the start, so a solution handed back as a warm
//     start is a fixed point and stops at iters 0.
//   An env that is done is frozen (its z, y no longer change) while its wave runs on; the columns of
//   an MFMA are independent, so an env's bits do not depend on its neighbours or on n.
// control/koopman.box_plan is the same iteration in numpy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "koopman_internal.h"

namespace {

constexpr double BOX_ALPHA = 1.6;   // over-relaxation (control/koopman.py BOX_ALPHA)
constexpr int BOX_MAX_ITER = 256;   // default
constexpr double BOX_TOL = 1e-9;

struct XDev {
  int N, NT, delta;  // NT: 16-row tiles of the plan
  int ksw;           // k-steps of K's window columns: ceil(H nz / 4)
  int kst;           // k-steps of K: ksw + 2 (x) + 4 NTL (features) + 2 (u_prev)
  int kcount;        // doubles of K's fragments [NT][kst][64]; P's follow, then Mrho's
  int pm;            // doubles of P's (and of Mrho's) fragments [NT][4 NT][64]
  int max_iter;
  int vote;          // doubles of LDS before the workgroup's vote word: max(K.total, 2 pm)
  int _pad;
  double umax, tol, rho, invL, alpha;
  double wfac;       // mu / (4 Lhat): a warm start is taken when res(plan) < wfac res(cold start)
};

// bounds of row 16 T + kq + 4 r (0 past N: those rows stay exact zeros); up[r] = u_prev of row
// kq + 4 r of tile 0, zero past nu
DEVI void bounds(const XDev& X, int T, int r, int kq, const double up[2], double& lo, double& hi) {
  const double m = 16 * T + kq + 4 * r < X.N ? X.umax : 0.0;
  const double sh = (!X.delta && T == 0 && r < 2) ? up[r] : 0.0;
  lo = -m - sh, hi = m - sh;
}

// out = F v for the [NT][4 NT][64] fragments F (in LDS, + lane); k-steps outer, tiles inner
DEVI void matvec(const double* F, int NT, const d4 (&v)[4], d4 (&out)[4]) {
#pragma unroll
  for (int T = 0; T < 4; T++) out[T] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 16; s++)
    if ((s >> 2) < NT) {
#pragma unroll
      for (int T = 0; T < 4; T++)
        if (T < NT) out[T] = mfma(F[(T * 4 * NT + s) * 64], v[s >> 2][s & 3], out[T]);
    }
}

// grad = P (z - wu) and ||z - clip(z - grad / Lhat)||_inf of this lane's env (in all 4 of its lanes)
DEVI double residual(const XDev& X, const double* Pf, int kq, const double up[2], const d4 (&z)[4],
                     const d4 (&wu)[4], d4 (&grad)[4]) {
  d4 d[4];
#pragma unroll
  for (int T = 0; T < 4; T++) d[T] = z[T] - wu[T];
  matvec(Pf, X.NT, d, grad);
  double rr = 0.0;
#pragma unroll
  for (int T = 0; T < 4; T++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      double lo, hi;
      bounds(X, T, r, kq, up, lo, hi);
      rr = fmax(rr, fabs(z[T][r] - clipd(z[T][r] - grad[T][r] * X.invL, lo, hi)));
    }
  rr = fmax(rr, __shfl_xor(rr, 16));
  return fmax(rr, __shfl_xor(rr, 32));
}

template <int NTL>
__global__ __launch_bounds__(256) void k_box_step(KDev K, XDev X, const double* __restrict__ frag,
                                                  const double* __restrict__ bfrag, int n,
                                                  const float* __restrict__ x, const double* __restrict__ z0,
                                                  const double* __restrict__ win, double* __restrict__ uprev,
                                                  double* __restrict__ plan, int warm, float* __restrict__ action,
                                                  int32_t* __restrict__ ok, int32_t* __restrict__ iters) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  // the workgroup's vote (does any env need the iteration?) sits behind the staged fragments
  int* vote = reinterpret_cast<int*>(lds + X.vote);
  if (threadIdx.x == 0) *vote = 0;
  __syncthreads();
  if (!z0) stage(lds, frag, K.total);  // (uniform: the encoder's fragments)
  const int lane = threadIdx.x & 63, kq = lane >> 4;
  const int e = lane_env(lane);
  const bool live = e < n;  // tail lanes run on zero inputs (interior) and never load or store
  double up[2], xb[2];
  d4 act[KT];
  load_uprev(K, uprev, n, e, live, kq, up);
  load_lifted<NTL>(K, lds, lane, n, e, live, x, z0, xb, act);
  // wu = K [window; z0; u_prev]: NT output tiles, the A fragments from global memory
  const int NT = X.NT, kst = X.kst;
  d4 wu[4];
#pragma unroll
  for (int T = 0; T < 4; T++) wu[T] = d4{0.0, 0.0, 0.0, 0.0};
  const double* Kf = bfrag + lane;
  {
    const int hz = K.H * K.nz;
    for (int s = 0; s < X.ksw; s++) {
      const int g = 4 * s + kq;
      const double b = (live && g < hz) ? win[(size_t)g * n + e] : 0.0;
#pragma unroll
      for (int T = 0; T < 4; T++)
        if (T < NT) wu[T] = mfma(Kf[((size_t)T * kst + s) * 64], b, wu[T]);
    }
    const double* Kz = Kf + (size_t)X.ksw * 64;
#pragma unroll
    for (int s = 0; s < 2 + 4 * NTL + 2; s++) {
      const double b = s < 2 ? xb[s] : (s < 2 + 4 * NTL ? act[(s - 2) >> 2][(s - 2) & 3] : up[s - 2 - 4 * NTL]);
#pragma unroll
      for (int T = 0; T < 4; T++)
        if (T < NT) wu[T] = mfma(Kz[((size_t)T * kst + s) * 64], b, wu[T]);
    }
  }
  // interior: clip(wu) == wu in every row of the env
  d4 z[4];
  int out = 0;
#pragma unroll
  for (int T = 0; T < 4; T++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      double lo, hi;
      bounds(X, T, r, kq, up, lo, hi);
      z[T][r] = clipd(wu[T][r], lo, hi);
      out |= z[T][r] != wu[T][r];
    }
  if (!live) out = 0;  // (a tail column has nothing to solve)
  out |= __shfl_xor(out, 16);
  out |= __shfl_xor(out, 32);
  int it_e = 0, done = 1;
  // (every wave of the workgroup takes this barrier; the encoder's fragments are dead after it)
  if (out) *vote = 1;
  __syncthreads();
  if (*vote) {
    stage(lds, bfrag + X.kcount, 2 * X.pm);
    if (__any(out)) {
      const double* Pf = lds + lane;
      const double* Mf = lds + X.pm + lane;
      d4 grad[4], y[4];
      double rr = residual(X, Pf, kq, up, z, wu, grad);
      if (warm && plan) {
        // the given plan is the start where it is provably the closer one: res / 2 <= ||z - z*|| <=
        // 2 (Lhat / mu) res, so where res(clip(plan)) < res(clip(wu)) mu / (4 Lhat)
        d4 zp[4], gp[4];
#pragma unroll
        for (int T = 0; T < 4; T++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int row = 16 * T + kq + 4 * r;
            double lo, hi;
            bounds(X, T, r, kq, up, lo, hi);
            zp[T][r] = (live && out && row < X.N) ? clipd(plan[(size_t)row * n + e], lo, hi) : z[T][r];
          }
        const double rp = residual(X, Pf, kq, up, zp, wu, gp);
        if (out && (rp <= X.tol || rp < rr * X.wfac)) {  // (or the plan already is a solution)
          rr = rp;
#pragma unroll
          for (int T = 0; T < 4; T++) z[T] = zp[T], grad[T] = gp[T];
        }
      }
      done = rr <= X.tol || !out;
      const double nir = -1.0 / X.rho;
#pragma unroll
      for (int T = 0; T < 4; T++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          double lo, hi;
          bounds(X, T, r, kq, up, lo, hi);
          const double g = grad[T][r];
          y[T][r] = ((z[T][r] <= lo && g > 0.0) || (z[T][r] >= hi && g < 0.0)) ? g * nir : 0.0;
        }
      for (int it = 1; it <= X.max_iter && !__all(done); it++) {
        d4 v[4], xm[4];
#pragma unroll
        for (int T = 0; T < 4; T++) v[T] = z[T] - y[T] - wu[T];
        matvec(Mf, NT, v, xm);
#pragma unroll
        for (int T = 0; T < 4; T++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            double lo, hi;
            bounds(X, T, r, kq, up, lo, hi);
            const double xh = X.alpha * (wu[T][r] + xm[T][r]) + (1.0 - X.alpha) * z[T][r];
            const double zn = clipd(xh + y[T][r], lo, hi);
            const double yn = y[T][r] + xh - zn;
            z[T][r] = done ? z[T][r] : zn;
            y[T][r] = done ? y[T][r] : yn;
          }
        rr = residual(X, Pf, kq, up, z, wu, grad);
        if (!done && rr <= X.tol) done = 1, it_e = it;
      }
      if (!done) it_e = X.max_iter;
    }
  }
  if (!live) return;
#pragma unroll
  for (int T = 0; T < 4; T++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = 16 * T + kq + 4 * r;
      if (plan && row < X.N) plan[(size_t)row * n + e] = z[T][r];
    }
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const int row = kq + 4 * r;
    if (row < K.ud) {
      const double u0 = X.delta ? z[0][r] : clipd(z[0][r] + up[r], -X.umax, X.umax);
      uprev[(size_t)row * n + e] = u0;
      action[(size_t)e * K.ud + row] = (float)u0;
    }
  }
  if (kq == 0) {
    if (ok) ok[e] = done;
    if (iters) iters[e] = it_e;
  }
}

typedef void (*BoxFn)(KDev, XDev, const double*, const double*, int, const float*, const double*, const double*,
                      double*, double*, int, float*, int32_t*, int32_t*);
const BoxFn BOXSTEP[4] = {k_box_step<1>, k_box_step<2>, k_box_step<3>, k_box_step<4>};

}  // namespace

struct KBox {  // a handle's state of this unit (sim_koopman::box)
  int device = 0;
  XDev xd{};
  double* d = nullptr;  // [K | P | Mrho] fragments
};

namespace {

// ---- host linear algebra (row-major, N <= 64)
typedef std::vector<double> Mat;
Mat matmul(const Mat& a, int m, int k, const Mat& b, int n) {  // [m,k] [k,n]
  Mat c((size_t)m * n, 0.0);
  for (int i = 0; i < m; i++)
    for (int l = 0; l < k; l++) {
      const double v = a[(size_t)i * k + l];
      if (v != 0.0)
        for (int j = 0; j < n; j++) c[(size_t)i * n + j] += v * b[(size_t)l * n + j];
    }
  return c;
}
// Cholesky S = L L' in place (lower); false when S is not positive definite
bool cholesky(Mat& s, int n) {
  for (int j = 0; j < n; j++) {
    double d = s[(size_t)j * n + j];
    for (int k = 0; k < j; k++) d -= s[(size_t)j * n + k] * s[(size_t)j * n + k];
    if (!(d > 0.0)) return false;
    d = std::sqrt(d);
    s[(size_t)j * n + j] = d;
    for (int i = j + 1; i < n; i++) {
      double v = s[(size_t)i * n + j];
      for (int k = 0; k < j; k++) v -= s[(size_t)i * n + k] * s[(size_t)j * n + k];
      s[(size_t)i * n + j] = v / d;
    }
  }
  return true;
}
// X <- (L L')^-1 X for X [n][m]
void chol_solve(const Mat& L, int n, Mat& X, int m) {
  for (int i = 0; i < n; i++)
    for (int c = 0; c < m; c++) {
      double v = X[(size_t)i * m + c];
      for (int k = 0; k < i; k++) v -= L[(size_t)i * n + k] * X[(size_t)k * m + c];
      X[(size_t)i * m + c] = v / L[(size_t)i * n + i];
    }
  for (int i = n - 1; i >= 0; i--)
    for (int c = 0; c < m; c++) {
      double v = X[(size_t)i * m + c];
      for (int k = i + 1; k < n; k++) v -= L[(size_t)k * n + i] * X[(size_t)k * m + c];
      X[(size_t)i * m + c] = v / L[(size_t)i * n + i];
    }
}
// extreme eigenvalues of a symmetric matrix by cyclic Jacobi
void sym_eig_range(Mat a, int n, double& lmin, double& lmax) {
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) (i == j ? diag : off) += a[(size_t)i * n + j] * a[(size_t)i * n + j];
    if (off <= 1e-30 * diag) break;
    for (int p = 0; p < n; p++)
      for (int q = p + 1; q < n; q++) {
        const double apq = a[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double th = (a[(size_t)q * n + q] - a[(size_t)p * n + p]) / (2.0 * apq);
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; k++) {
          const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
          a[(size_t)k * n + p] = c * akp - s * akq, a[(size_t)k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; k++) {
          const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
          a[(size_t)p * n + k] = c * apk - s * aqk, a[(size_t)q * n + k] = s * apk + c * aqk;
        }
      }
  }
  lmin = lmax = a[0];
  for (int i = 1; i < n; i++) lmin = std::min(lmin, a[(size_t)i * n + i]), lmax = std::max(lmax, a[(size_t)i * n + i]);
}

int check_opts(const sim_koopman_box_opts* o) {
  if (!o) return SIM_OK;
  if (o->struct_size != (int32_t)sizeof(sim_koopman_box_opts) || o->abi_version != SIM_ABI_VERSION)
    return soarm_set_error(SIM_E_ARG, "sim_koopman_box_opts: struct_size / abi_version do not match this library");
  if (!(o->u_max > 0.0)) return soarm_set_error(SIM_E_ARG, "box MPC: u_max must be positive");
  if (!(o->tol > 0.0)) return soarm_set_error(SIM_E_ARG, "box MPC: tol must be positive");
  if (o->max_iter < 1) return soarm_set_error(SIM_E_ARG, "box MPC: max_iter must be >= 1");
  return SIM_OK;
}
int check_shape(int nz, int nu, int H) {
  if (H * nu > 64)
    return soarm_set_error(SIM_E_MODEL, "box MPC: N = H * u_dim = " + std::to_string(H * nu) + " must be <= 64");
  if (nz > 64) return soarm_set_error(SIM_E_MODEL, "box MPC: nz = " + std::to_string(nz) + " must be <= 64");
  return SIM_OK;
}

}  // namespace

// the option checks, for sim_koopman_set_bilinear_box (koopman_bilinear.hip): one helper serves both steps
int koopman_box_check_opts(const sim_koopman_box_opts* opts) { return check_opts(opts); }

void koopman_box_release(KBox* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  (void)hipFree(b->d);
  delete b;
}

extern "C" {

int sim_koopman_box_check(const sim_koopman_desc* d, const sim_koopman_box_opts* opts) {
  if (!d) return soarm_set_error(SIM_E_ARG, "null argument");
  if (int rc = check_opts(opts)) return rc;
  if (d->nlayer < 1 || d->nlayer > SIM_KMAXLAYER || d->x_dim < 1 || d->u_dim < 1 || d->horizon < 1)
    return soarm_set_error(SIM_E_ARG, "box MPC: bad controller description");
  return check_shape(d->x_dim + d->width[d->nlayer], d->u_dim, d->horizon);
}

int sim_koopman_set_box(sim_koopman* k, const double* A, const double* B, int delta, double q, double r,
                        const sim_koopman_box_opts* opts) {
  if (!k || !A || !B) return soarm_set_error(SIM_E_ARG, "null argument");
  const KDev& K = k->kd;
  const klayout::Encoder enc = koopman_layout_of(K);
  // a refusal below leaves box_step refused and everything else as it was
  koopman_box_release(k->box);
  k->box = nullptr;
  if (int rc = check_opts(opts)) return rc;
  if (!(q > 0.0) || !(r > 0.0)) return soarm_set_error(SIM_E_ARG, "box MPC: q and r must be positive");
  const int nz = K.nz, nu = K.ud, H = K.H, N = H * nu, ntl = enc.ntl;
  if (int rc = check_shape(nz, nu, H)) return rc;
  XDev X{};
  X.N = N, X.NT = (N + 15) / 16, X.delta = delta ? 1 : 0;
  X.ksw = (H * nz + 3) / 4;
  X.kst = X.ksw + klayout::ks_zu(enc);
  X.kcount = X.NT * X.kst * 64;
  X.pm = X.NT * 4 * X.NT * 64;
  X.umax = opts ? opts->u_max : K.uclip;
  X.tol = opts ? opts->tol : BOX_TOL;
  X.max_iter = opts ? opts->max_iter : BOX_MAX_ITER;
  X.alpha = BOX_ALPHA;
  if (!(X.umax > 0.0)) return soarm_set_error(SIM_E_ARG, "box MPC: u_max must be positive");
  X.vote = std::max(K.total, 2 * X.pm);
  const size_t lds_bytes = (size_t)(X.vote + 2) * sizeof(double);  // (+ the vote word)
  if (lds_bytes > KOOPMAN_LDS_BYTES)
    return soarm_set_error(SIM_E_MODEL, "box MPC: the LDS plan (" + std::to_string(lds_bytes) + " bytes) must be <= 160 KiB");

  // Gam[t][s] = A^(t-s) B, Phi = [A; A^2; ..; A^H]
  const int hz = H * nz, kc = hz + nz + nu;
  Mat Am(A, A + (size_t)nz * nz), Bm(B, B + (size_t)nz * nu);
  std::vector<Mat> pw(H + 1);
  pw[0].assign((size_t)nz * nz, 0.0);
  for (int i = 0; i < nz; i++) pw[0][(size_t)i * nz + i] = 1.0;
  for (int t = 1; t <= H; t++) pw[t] = matmul(Am, nz, nz, pw[t - 1], nz);
  Mat Gam((size_t)hz * N, 0.0), Phi((size_t)hz * nz);
  for (int d = 0; d < H; d++) {
    const Mat ab = matmul(pw[d], nz, nz, Bm, nu);
    for (int s = 0; s + d < H; s++)
      for (int i = 0; i < nz; i++)
        for (int c = 0; c < nu; c++) Gam[((size_t)(s + d) * nz + i) * N + s * nu + c] = ab[(size_t)i * nu + c];
    std::copy(pw[d + 1].begin(), pw[d + 1].end(), Phi.begin() + (size_t)d * nz * nz);
  }
  Mat GamT((size_t)N * hz);
  for (int i = 0; i < hz; i++)
    for (int j = 0; j < N; j++) GamT[(size_t)j * hz + i] = Gam[(size_t)i * N + j];
  // P = 2 (q Gam'Gam + r Rm), Rm = D'D ('delta_mpc': diagonal blocks 2 I, the last I, -I beside) or I
  Mat P = matmul(GamT, N, hz, Gam, N);
  for (int i = 0; i < N; i++)
    for (int j = 0; j < N; j++) {
      double rm = i == j ? 1.0 : 0.0;
      if (X.delta) {
        if (i == j) rm = i / nu == H - 1 ? 1.0 : 2.0;
        else if (i - j == nu || j - i == nu) rm = -1.0;
      }
      P[(size_t)i * N + j] = 2.0 * (q * P[(size_t)i * N + j] + r * rm);
    }
  for (int i = 0; i < N; i++)
    for (int j = 0; j < i; j++) P[(size_t)i * N + j] = P[(size_t)j * N + i] = 0.5 * (P[(size_t)i * N + j] + P[(size_t)j * N + i]);
  // [Gw | Gz | Gu] = [2 q Gam' | -Gw Phi | 2 r E0 ('delta_mpc') or 0], then K = P^-1 of it
  const Mat GwPhi = matmul(GamT, N, hz, Phi, nz);
  Mat Kall((size_t)N * kc, 0.0);
  for (int i = 0; i < N; i++) {
    for (int j = 0; j < hz; j++) Kall[(size_t)i * kc + j] = 2.0 * q * GamT[(size_t)i * hz + j];
    for (int j = 0; j < nz; j++) Kall[(size_t)i * kc + hz + j] = -2.0 * q * GwPhi[(size_t)i * nz + j];
    if (X.delta && i < nu) Kall[(size_t)i * kc + hz + nz + i] = 2.0 * r;
  }
  Mat L = P;
  if (!cholesky(L, N)) return soarm_set_error(SIM_E_MODEL, "box MPC: the Hessian is not positive definite");
  chol_solve(L, N, Kall, kc);
  double lmin, lmax, lhat = 0.0;
  sym_eig_range(P, N, lmin, lmax);
  if (!(lmin > 0.0)) return soarm_set_error(SIM_E_MODEL, "box MPC: the Hessian is not positive definite");
  for (int i = 0; i < N; i++) {
    double s = 0.0;
    for (int j = 0; j < N; j++) s += std::fabs(P[(size_t)i * N + j]);
    lhat = std::max(lhat, s);
  }
  X.rho = std::sqrt(lmin * lmax), X.invL = 1.0 / lhat, X.wfac = lmin / (4.0 * lhat);
  Mat S = P, Mr((size_t)N * N, 0.0);
  for (int i = 0; i < N; i++) S[(size_t)i * N + i] += X.rho, Mr[(size_t)i * N + i] = X.rho;
  if (!cholesky(S, N)) return soarm_set_error(SIM_E_MODEL, "box MPC: P + rho I is not positive definite");
  chol_solve(S, N, Mr, N);

  // fragments: K's k order is [window (H nz, flat) | x rows 0..7 | feature rows (16 per tile) | u_prev 0..7]
  std::vector<double> blob((size_t)X.kcount + 2 * X.pm, 0.0);
  klayout::fill_frag(blob.data(), X.NT, X.kst, [&](int row, int kk) {
    const int c = kk < 4 * X.ksw ? (kk < hz ? kk : -1) : klayout::zu_col(enc, kk - 4 * X.ksw, hz);
    return (row < N && c >= 0) ? Kall[(size_t)row * kc + c] : 0.0;
  });
  klayout::each_frag(X.NT, 4 * X.NT, [&](int pos, int row, int c) {
    const bool in = row < N && c < N;
    blob[(size_t)X.kcount + pos] = in ? P[(size_t)row * N + c] : 0.0;
    blob[(size_t)X.kcount + X.pm + pos] = in ? Mr[(size_t)row * N + c] : 0.0;
  });
  KCHECK(hipSetDevice(k->device));
  KBox* b = new KBox;
  b->device = k->device, b->xd = X;
  if (hipMalloc(&b->d, blob.size() * sizeof(double)) != hipSuccess) {
    delete b;
    return soarm_set_error(SIM_E_HIP, "hipMalloc failed");
  }
  // the state is published only once the upload and the kernel's LDS attribute are in place
  hipError_t he = hipMemcpy(b->d, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice);
  if (he == hipSuccess)
    he = koopman_raise_lds((const void*)BOXSTEP[ntl - 1]);
  if (he != hipSuccess) {
    koopman_box_release(b);
    return soarm_set_error(SIM_E_HIP, std::string("box MPC: upload failed: ") + hipGetErrorString(he));
  }
  k->box = b;
  return SIM_OK;
}

int sim_koopman_box_step(sim_koopman* k, int n, const float* x, const double* z0, const double* window,
                         double* u_prev, double* plan, int warm, float* action, int32_t* ok, int32_t* iters,
                         void* stream) {
  if (!k || !window || !u_prev || !action || (!x && !z0) || n < 0) return soarm_set_error(SIM_E_ARG, "bad argument");
  const KBox* b = k->box;
  if (!b) return soarm_set_error(SIM_E_ARG, "sim_koopman_set_box was not called (or refused the model)");
  if (n == 0) return SIM_OK;
  const KDev& K = k->kd;
  hipLaunchKernelGGL(BOXSTEP[K.ntile[K.nl - 1] - 1], dim3((n + 63) / 64), dim3(256),
                     (size_t)(b->xd.vote + 2) * sizeof(double), (hipStream_t)stream, K, b->xd, k->d_frag, b->d,
                     n, x, z0, window, u_prev, plan, warm, action, ok, iters);
  KCHECK(hipGetLastError());
  return SIM_OK;
}

}  // extern "C"
