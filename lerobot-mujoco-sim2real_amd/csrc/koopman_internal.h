// koopman_internal.h — what the Koopman controller's units share on the host: the handle
// (include/koopman_mpc.h: sim_koopman) with the kernel argument structs it holds, the error helpers and
// the functions one unit calls in another.  Units: koopman_mpc.hip (create / free, encode, feedforward,
// mpc_step), koopman_bilinear.hip (the DBKN steps), koopman_predict.hip (open-loop prediction) and
// koopman_box.hip (the DKUC step with input limits).
#ifndef KOOPMAN_INTERNAL_H
#define KOOPMAN_INTERNAL_H

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/koopman_mpc.h"
#include "koopman_frag.h"
#include "koopman_layout.h"

int soarm_set_error(int code, const std::string& msg);  // soarm_model.hip (sim_last_error)

#define KCHECK(x)                                                                                  \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) return soarm_set_error(SIM_E_HIP, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

// let `kernel` be launched with up to the CU's whole LDS as dynamic LDS
inline hipError_t koopman_raise_lds(const void* kernel) {
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)KOOPMAN_LDS_BYTES);
}

// The kernel argument structs live in the unnamed namespace like KDev (koopman_frag.h) and the kernels
// that take them; every unit sees the same definitions from this header.
namespace {

// k_bilinear / k_bilinear_box (koopman_bilinear.hip)
struct BDev {
  int nz, nu, H, N, delta, per_env;  // per_env: doubles of LDS per env
  int epw;                           // envs (waves) per workgroup
  int xreg;                          // doubles of the X / Gram / packed-Hessian region
  int xs;                            // X_k's stride (>= nz nu, = nu mod 32: the rhs phase's lanes
                                     // (X_{t-s} column c) then fall in distinct LDS banks)
  int mreg;                          // doubles of the M region (M, Zs; Y; the Cholesky's column buffer)
  double q, r, uclip;
};

// k_predict (koopman_predict.hip)
struct PDev {
  int afrag;     // [A | B] fragments in LDS, after the K.total doubles of the controller: [1 + NTL][ks][64]
  int ks;        // 2 (x) + 4 NTL (features) + 2 (u)
  int acount;    // doubles of the [A | B] fragments
  int hks;       // k-steps of z: 2 + 4 NTL
  int bilinear;  // Hhat fragments follow at mfrag + acount: [1 + NTL][ud][hks][64]
};

}  // namespace

struct KBox;  // the constrained DKUC step's state (koopman_box.hip)

struct sim_koopman {
  int device = 0;
  sim_koopman_desc desc;
  KDev kd;
  double* d_frag = nullptr;    // encoder + [Gz | Gu] fragments, biases
  double* d_grfrag = nullptr;  // Gr fragments
  // DBKN (sim_koopman_set_bilinear): A [nz][nz], B [nz][nu], Hhat [j][(i nu + c)]
  BDev bd{};
  double *d_A = nullptr, *d_B = nullptr, *d_Hh = nullptr;
  // the DBKN step with input limits (sim_koopman_set_bilinear_box; dropped by set_bilinear)
  bool bbox = false;
  double bb_umax = 0.0, bb_tol = 0.0;
  int bb_max_iter = 0;
  // open-loop prediction (sim_koopman_set_model): [A | B] fragments, then the Hhat fragments
  PDev pd{};
  double* d_model = nullptr;
  int model_state = 0;  // 0: not set, 1: set, 2: set_model refused the shape (SIM_E_MODEL)
  int wpw = 4;          // waves per workgroup (SOARM_KPREDICT_WAVES: 1, 2 or 4)
  KBox* box = nullptr;  // sim_koopman_set_box
};

// the padded-k maps of a handle's encoder (klayout::z_of_row, z_of_k, u_of_k)
inline klayout::Encoder koopman_layout_of(const KDev& K) {
  klayout::Encoder e{};
  e.xd = K.xd, e.ud = K.ud, e.nl = K.nl, e.outw = K.outw, e.nz = K.nz, e.ntl = K.ntile[K.nl - 1];
  return e;
}

// koopman_box.hip
void koopman_box_release(KBox* box);                           // frees the state (null: nothing)
int koopman_box_check_opts(const sim_koopman_box_opts* opts);  // the option checks, for both box steps

#endif  // KOOPMAN_INTERNAL_H
