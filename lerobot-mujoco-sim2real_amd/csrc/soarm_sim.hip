// soarm_sim.hip — the kernels of the MI355X batched SO-ARM101 simulator, their launches behind
// the C ABI (include/soarm_sim.h) and the batch's lifetime (buffers, per-device model upload,
// graph cache).  The model itself is built by soarm_model.hip, the CPU backend is soarm_cpu.hip.
// Build: build.py (hipcc --offload-arch=gfx950 -O3 -shared -fPIC).
//
//   k_step   : ctrl[:nact] = action; frame_skip x mj_step; obs     (SOARM101_Env.py:108-142)
//   k_reset  : mj_resetData + init qpos/qvel + mj_forward + obs     (SOARM101_Env.py:77-106)
//   k_observe: mj_kinematics + _get_state                           (SOARM101_Env.py:69-75)
//   k_ik     : batched damped-least-squares site IK                 (control/TrajectoryGenerator.py:96-107)
//   k_ik_box : batched box-bounded site IK, frames chained          (control/casadi_ik.py:27-167)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>
#include <dlfcn.h>

#include "../../include/soarm_sim.h"
#ifdef SOARM_DIAG_SKIPP
// (diagnostic build: SOARM_DIAG_SKIP names pairs k_collide returns from at once; SOARM_DIAG_STAGE:
// 1 midphase only, 2 no mask atomics, 3 native GJK without EPA, else everything)
__device__ uint32_t g_diag_skip[4];
__device__ int g_diag_stage;
#define SOARM_DIAG_NO_EPA (g_diag_stage == 3)
#endif
#ifdef SOARM_DIAG_SUPPORT
__device__ unsigned long long g_diag_sup[16][4];  // (soarm_collide.h diag_support)
__device__ uint32_t g_diag_prev[2][128 * 8192];
#endif
#include "soarm_collide.h"
#include "soarm_env.h"
#include "soarm_ikbox.h"
#include "sim_internal.h"
#include "soarm_pgs.h"

using namespace soarm;

// ------------------------------------------------------------------ errors
// (the one error slot is soarm_model.hip's)
static int fail(int code, const std::string& msg) { return soarm_set_error(code, msg); }
#define HIPCHECK(x)                                                                   \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) return fail(SIM_E_HIP, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

// ------------------------------------------------------------------ tracing
// roctx ranges (SURVEY.md §5 tracing): with SOARM_ROCTX=1 every ABI call, and each stage of the
// contact env-step (geom poses, collide, substep, per substep), is bracketed by a roctx range
// that `rocprofv3 --marker-trace` records beside the kernel trace.  The roctx library is opened
// at run time, so the product has no link dependency on the profiler; the env-step is then
// launched stage by stage (no hipGraph replay) so that the ranges bracket real launches.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    const char* on = getenv("SOARM_ROCTX");
    if (!on || on[0] != '1') return;
    void* h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
    pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!push || !pop) push = nullptr, pop = nullptr;
  }
};
static const Roctx& roctx() {
  static const Roctx r;
  return r;
}
struct TraceRange {
  const bool on;
  explicit TraceRange(const char* name) : on(roctx().push != nullptr) {
    if (on) roctx().push(name);
  }
  ~TraceRange() {
    if (on) roctx().pop();
  }
};

// read-only model data on one device (constants, pair records, hull tables):
// uploaded by the first batch created on that device, shared by every later
// batch of the same model there, freed with the model
struct DevModel {
  int device = -1;
  DModel* d_model = nullptr;
  PairRec* d_prec = nullptr;  // the collide's records in dispatch order (dmodel.h PairRec)
  uint4 *d_hrec = nullptr, *d_hlutrec = nullptr;
  uint16_t* d_hovf = nullptr;
  float* d_hsb = nullptr;
  ~DevModel() {
    (void)hipSetDevice(device);
    (void)hipFree(d_model);
    (void)hipFree(d_prec);
    (void)hipFree(d_hrec);
    (void)hipFree(d_hlutrec);
    (void)hipFree(d_hovf);
    (void)hipFree(d_hsb);
  }
};

sim_model::~sim_model() {
  for (DevModel* d : dev) delete d;
}

struct sim_batch {
  const sim_model* model = nullptr;
  int n = 0, device = 0;
  CpuBatch* cpu = nullptr;     // device = -1: the CPU backend (soarm_cpu.hip) runs every call
  DModel* d_model = nullptr;   // shared per (model, device): DevModel
  const PairRec* d_prec = nullptr;  // likewise: k_collide's per-row records
  float* d_scratch = nullptr;  // contact rows, [slot][env]
  size_t scratch_floats = 0;
  float* d_gpose = nullptr;    // body world frames [body*BREC+k][env] (soarm_collide.h load_pose)
  float* d_cbuf = nullptr;     // collide output [slot*7+f][env]
  // [pair][env] ints that nothing writes or reads: solve_constraints and k_substep only test the
  // pointer they are handed for null (no candidate pairs), k_gather ignores it
  int* d_ccount = nullptr;
  uint32_t* d_pmask = nullptr; // pairs with contacts, bit p%32 of word p/32: [word][env]
  float* d_sepax = nullptr;    // separating-axis cache [pair*3+k][env] (soarm_collide.h SepCache)
  // profiling (sim_profile_begin/end)
  bool prof = false;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  std::vector<std::pair<int, size_t>> ev_marks;  // (kind, index of start event)
  sim_params params{nullptr, nullptr, nullptr};
  // hipGraph cache of the contact env-step's 1 + 2 x frame_skip launches, keyed by the
  // buffers the kernels are bound to (SOARM_NO_GRAPH=1 disables)
  struct GraphKey {
    sim_state s;
    const float* action;
    float* obs;
    int frame_skip;
    bool rs;  // the RS substep chosen (SOARM_RS, read per call): part of what the graph captured
    bool operator==(const GraphKey& o) const {
      return !memcmp(&s, &o.s, sizeof(s)) && action == o.action && obs == o.obs && frame_skip == o.frame_skip &&
             rs == o.rs;
    }
  };
  bool use_graphs = true;
  int rs_cap = 0;  // envs the RS substep runs in one round (4 per wave, one wave per SIMD)
  hipStream_t cap_stream = nullptr;
  std::vector<std::pair<GraphKey, hipGraphExec_t>> graphs;
  void drop_graphs() {
    for (auto& g : graphs) (void)hipGraphExecDestroy(g.second);
    graphs.clear();
  }
  ~sim_batch() {
    if (device < 0) {
      cpu_batch_free(cpu);
      return;
    }
    (void)hipSetDevice(device);
#ifdef SOARM_DIAG_SUPPORT
    {  // (diagnostic build: the support-query counters of every collide so far)
      unsigned long long c[CON_MAXG][4];
      (void)hipMemcpyFromSymbol(c, HIP_SYMBOL(g_diag_sup), sizeof(c), 0, hipMemcpyDeviceToHost);
      for (int g = 0; g < CON_MAXG; g++)
        if (c[g][0])
          fprintf(stderr, "support geom %d: queries %llu, same cell %llu, same answer %llu, climb trips %llu\n", g,
                  c[g][0], c[g][1], c[g][2], c[g][3]);
    }
#endif
    (void)hipFree(d_scratch);
    (void)hipFree(d_gpose);
    (void)hipFree(d_cbuf);
    (void)hipFree(d_ccount);
    (void)hipFree(d_pmask);
    (void)hipFree(d_sepax);
    for (auto e : ev_pool) (void)hipEventDestroy(e);
    drop_graphs();
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
  }
};

#include "soarm_substep.h"


// mj_collision, one lane per (env, candidate pair); blockIdx.y = pair
#ifndef SOARM_COLLIDE_BLOCK
#define SOARM_COLLIDE_BLOCK 256  // envs (lanes) per collide workgroup
#endif
#ifndef SOARM_EPA_SLOTS
#define SOARM_EPA_SLOTS 8  // EPA polytopes per native-collide workgroup in LDS (2.1 KB each)
#endif
#ifndef SOARM_COLLIDE_WAVES
#define SOARM_COLLIDE_WAVES 3  // min waves per SIMD (VGPR cap 512 / 3 = 168)
#endif
// CCD: one instantiation per narrowphase, so the MPR kernel carries none of EPA's private-memory
// polytope (2.2 KB of scratch per lane)
// prec: row blockIdx.y's pair record (DModel::pair_order: the heavy pairs dispatch first) -- the
// kernel reads no other model data
template <int CCD>
__global__ __launch_bounds__(SOARM_COLLIDE_BLOCK, SOARM_COLLIDE_WAVES) void k_collide(const PairRec* __restrict__ prec, int n,
                                                 const float* __restrict__ gpose,
                                                 float* __restrict__ cbuf,
                                                 uint32_t* __restrict__ pmask,
                                                 float* __restrict__ sepax,
                                                 unsigned long long* __restrict__ pcyc) {
  // (env chunks numbered per XCD as in k_geom / k_substep: the geom records this reads and the
  // contact buffer it writes stay in the L2 of the XCD whose substep waves own those envs)
  // native: LDS slots for the EPA polytopes of this workgroup's penetrating lanes (EpaPool)
  constexpr int NSLOT = CCD == SIM_CCD_NATIVE ? SOARM_EPA_SLOTS : 0;
  __shared__ EpaPoly s_epa[NSLOT > 0 ? NSLOT : 1];
  __shared__ int s_epa_used;
  if constexpr (NSLOT > 0) {
    if (threadIdx.x == 0) s_epa_used = 0;
    __syncthreads();
  }
  const EpaPool pool{s_epa, &s_epa_used, NSLOT};
  const int e = xcd_block() * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const PairRec& pr = prec[blockIdx.y];
  const int p = pr.pair;
#ifdef SOARM_DIAG_SKIPP
  if ((g_diag_skip[p >> 5] >> (p & 31)) & 1u) return;  // (diagnostic: the pairs SOARM_DIAG_SKIP names cost nothing)
#endif
  const long long t0 = pcyc ? clock64() : 0;
  PairOut o{cbuf, n, e, pr.slot, pr.cap, 0};
#ifdef SOARM_DIAG_SKIPP
  if (g_diag_stage == 1) {
    GeomPose P1, P2;
    if (midphase(pr, gpose, n, e, P1, P2)) soa(cbuf, 0, n, e) = P1.p[0] + P2.p[0];
    return;
  }
#endif
  collide_pair<CCD>(pr, gpose, n, e, o, SepCache{sepax, n, e}, NSLOT > 0 ? &pool : nullptr);
#ifdef SOARM_DIAG_SKIPP
  if (g_diag_stage == 2) return;
#endif
  // (no per-pair count is stored: the pair mask bit and, for multi-contact pairs, its 2-bit
  // count word carry it -- an empty pair costs no store)
  if (o.n > 0) {
    atomicOr(&pmask[(size_t)(p >> 5) * n + e], 1u << (p & 31));
    const int cq = pr.cq;
    if (cq >= 0) atomicOr(&pmask[(size_t)pr.cqword * n + e], (uint32_t)(o.n - 1) << (2 * cq));
  }
#ifdef SOARM_COLLIDE_STATS
  // diagnostic build: per pair, how many envs each test decided (13-bit counters: codes 0-3 in
  // the first word, 4-7 in the second; see PairOut::xc)
  if (pcyc) atomicAdd(&pcyc[(o.xc >> 2) * gridDim.y + p], 1ull << (13 * (o.xc & 3)));
#else
  if (pcyc && (threadIdx.x & 63) == 0) {
    const unsigned long long dt = (unsigned long long)(clock64() - t0);
    atomicAdd(&pcyc[p], dt);
    atomicMax(&pcyc[gridDim.y + p], dt);
  }
#endif
}

// the collide launch: (env, pair) lanes, SOARM_COLLIDE_BLOCK-env blocks x npair
static void launch_collide(const sim_batch* b, hipStream_t q, unsigned long long* pcyc) {
  auto kern = b->model->desc.ccd == SIM_CCD_NATIVE ? k_collide<SIM_CCD_NATIVE> : k_collide<SIM_CCD_MPR>;
  int rows = b->model->desc.npair;
#ifdef SOARM_DIAG_SKIPP
  // (diagnostic: SOARM_DIAG_ROWS=k launches only the first k rows of the dispatch order -- timings only)
  if (const char* v = getenv("SOARM_DIAG_ROWS")) rows = std::min(rows, std::max(1, atoi(v)));
#endif
  hipLaunchKernelGGL(kern, dim3((b->n + SOARM_COLLIDE_BLOCK - 1) / SOARM_COLLIDE_BLOCK, rows),
                     dim3(SOARM_COLLIDE_BLOCK), 0, q, b->d_prec, b->n,
                     b->d_gpose, b->d_cbuf, b->d_pmask, b->d_sepax, pcyc);
}

// walk the pairs in order and append their contacts (deterministic indexing)
DEVI int gather_contacts(const DModel& m, int n, int e, const float* __restrict__ cbuf, const PairMask& pm,
                         const ConLds& C, int& status) {
  int ncon = 0;
  for (int p = 0; p < m.npair; p++) {
    const int c = (pm.w[p >> 5] >> (p & 31)) & 1u ? pm.count(m, p) : 0;
    const int s0 = m.pair_slot[p];
    for (int k = 0; k < c; k++) {
      if (ncon >= SIM_MAXCON) {
        status |= SIM_ST_CONOVERFLOW;
        break;
      }
      C.dist(ncon) = cbuf[((size_t)(s0 + k) * 7) * n + e];
#pragma unroll
      for (int f = 0; f < 3; f++) {
        C.pos(ncon, f) = cbuf[((size_t)(s0 + k) * 7 + 1 + f) * n + e];
        C.n(ncon, f) = cbuf[((size_t)(s0 + k) * 7 + 4 + f) * n + e];
      }
      C.set_pair(ncon, p);
      ncon++;
    }
  }
  return ncon;
}

// diagnostic: compacted contact list [N][SIM_MAXCON][8] (dist, pos, normal, pair) + count
__global__ __launch_bounds__(64) void k_gather(const DModel* __restrict__ dm, int n,
                                               const float* __restrict__ cbuf,
                                               const int* __restrict__ ccount, uint32_t* __restrict__ pmask,
                                               float* __restrict__ out, int* __restrict__ nout) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  PairMask pm;
  pm.load(pmask, *dm, n, e);  // the pairs with contacts (and multi-contact counts)
  for (int w = 0; w < pmask_words(*dm); w++) soa(pmask, w, n, e) = 0u;
  __shared__ float s_con[SIM_MAXCON * 8][64];
  const ConLds C{s_con, (int)threadIdx.x};
  int status = 0;
  const int nc = gather_contacts(*dm, n, e, cbuf, pm, C, status);
  for (int c = 0; c < nc; c++)
    for (int f = 0; f < 8; f++) out[((size_t)e * SIM_MAXCON + c) * 8 + f] = s_con[c * 8 + f][threadIdx.x];
  nout[e] = nc;
}

template <int NA, int NF>
__global__ __launch_bounds__(64) void k_reset(const DModel* __restrict__ dm, int n, sim_state st,
                                              const float* __restrict__ init_qpos,
                                              const float* __restrict__ init_qvel,
                                              const float* __restrict__ extra_qpos, uint32_t k0,
                                              uint32_t k1, long long env_offset,
                                              const uint8_t* __restrict__ mask,
                                              float* __restrict__ obs) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) env_reset<NA, NF>(dm, n, e, st, init_qpos, init_qvel, extra_qpos, k0, k1, env_offset, mask, obs);
}

// Keyed uniform draws for the rollout's action / phase streams: out[e][j] = lo + width u, u from
// Philox4x32-10 keyed by `seed`, counter (gid, gid >> 32, counter, 1 + j / 4) — sim_reset's draws
// use the 4th word 0, so the streams never overlap.  Keyed by global env id, so a dataset is the
// same for any env chunking / GPU count.  Host mirror: workloads.keyed_uniform.
__global__ __launch_bounds__(64) void k_rand(int n, uint32_t k0, uint32_t k1, long long env_offset,
                                             uint32_t counter, int k, float lo, float width,
                                             float* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) env_rand(e, k0, k1, env_offset, counter, k, lo, width, out);
}

// qfrc_bias at the current state (mj_comVel + mj_rne with flg_acc = 0, as left by mj_forward)
template <int NA, int NF>
__global__ __launch_bounds__(64) void k_bias(const DModel* __restrict__ dm, int n, sim_state st,
                                             float* __restrict__ bias, sim_params pp) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) env_bias<NA, NF>(dm, n, e, st, bias, pp);
}

template <int NA, int NF>
__global__ __launch_bounds__(64) void k_observe(const DModel* __restrict__ dm, int n, sim_state st,
                                                float* __restrict__ obs) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) env_observe<NA, NF>(dm, n, e, st, obs);
}

// DLS site IK (soarm_env.h env_ik)
template <int NA>
__global__ __launch_bounds__(64) void k_ik(const DModel* __restrict__ dm, int n,
                                           const float* __restrict__ target, const float* __restrict__ tq,
                                           float* __restrict__ q, int32_t* __restrict__ ok,
                                           int32_t* __restrict__ iters, sim_ik_opts o) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) env_ik<NA>(dm, n, e, target, tq, q, ok, iters, o);
}

// box-bounded site IK, the frames chained in the lane (soarm_ikbox.h env_ik_box)
template <int NA>
__global__ __launch_bounds__(64) void k_ik_box(const DModel* __restrict__ dm, int n, int nframe,
                                               const float* __restrict__ target, const float* __restrict__ tq,
                                               float* __restrict__ q, float* __restrict__ q_traj,
                                               int32_t* __restrict__ ok, int32_t* __restrict__ iters,
                                               sim_ik_box_opts o) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) env_ik_box<NA>(dm, n, e, nframe, target, tq, q, q_traj, ok, iters, o);
}

static inline dim3 grid_for(int n) { return dim3((n + 63) / 64); }

// profiling: kind >= 0 records a start event for that kernel kind, -1 the matching stop
static void prof_mark(sim_batch* b, int kind, hipStream_t st) {
  if (!b->prof) return;
  if (b->ev_used == b->ev_pool.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    b->ev_pool.push_back(e);
  }
  if (kind >= 0) b->ev_marks.emplace_back(kind, b->ev_used);
  (void)hipEventRecord(b->ev_pool[b->ev_used++], st);
}

// n elements of device memory, zeroed if asked
template <class T>
static int dev_alloc(T*& p, size_t n, bool zero) {
  HIPCHECK(hipMalloc(&p, n * sizeof(T)));
  if (zero) HIPCHECK(hipMemset(p, 0, n * sizeof(T)));
  return SIM_OK;
}

// the model's device copy on `device` (the tables the collide reads through PairRec, the DModel
// bound to them, the pair records): made by the first batch there, reused after
static int upload_model(const sim_model* m, int device, DModel** out, const PairRec** prec) {
  std::lock_guard<std::mutex> lk(m->mu);
  for (DevModel* d : m->dev)
    if (d->device == device) {
      *out = d->d_model, *prec = d->d_prec;
      return SIM_OK;
    }
  std::unique_ptr<DevModel> D(new DevModel());  // (a failing call below frees it: nothing half-uploaded is cached)
  D->device = device;
  auto up = [&](auto*& dst, const auto& src) -> int {
    if (int rc = dev_alloc(dst, std::max<size_t>(src.size(), 1), false)) return rc;
    if (!src.empty()) HIPCHECK(hipMemcpy(dst, src.data(), src.size() * sizeof(*dst), hipMemcpyHostToDevice));
    return SIM_OK;
  };
  if (int rc = up(D->d_hrec, m->hull_rec)) return rc;
  if (int rc = up(D->d_hlutrec, m->hull_lutrec)) return rc;
  if (int rc = up(D->d_hovf, m->hull_ovf)) return rc;
  if (int rc = up(D->d_hsb, m->hull_sb)) return rc;
  const DModel dm = bind_tables(*m, D->d_hrec, D->d_hlutrec, D->d_hovf, D->d_hsb);
  if (int rc = dev_alloc(D->d_model, 1, false)) return rc;
  HIPCHECK(hipMemcpy(D->d_model, &dm, sizeof(dm), hipMemcpyHostToDevice));
  if (int rc = up(D->d_prec, pair_records(dm))) return rc;
  *out = D->d_model, *prec = D->d_prec;
  m->dev.push_back(D.release());
  return SIM_OK;
}

// ============================================================== C ABI
extern "C" {

const char* sim_version(void) { return "soarm_sim 0.2.0 gfx950 (abi 2)"; }

int sim_batch_create(const sim_model* m, int n_envs, int device, sim_batch** out) {
  if (!m || !out || n_envs <= 0) return fail(SIM_E_ARG, "bad argument");
  if (device == -1) {  // the CPU backend: host buffers, synchronous calls
    std::unique_ptr<sim_batch> B(new sim_batch());
    B->model = m;
    B->n = n_envs;
    B->device = -1;
    if (int rc = cpu_batch_create(m, n_envs, &B->cpu)) return rc;
    *out = B.release();
    return SIM_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SIM_E_NODEVICE, "no HIP device");
  if (device < 0 || device >= ndev) return fail(SIM_E_ARG, "bad device ordinal");
  HIPCHECK(hipSetDevice(device));
  std::unique_ptr<sim_batch> B(new sim_batch());  // (a failing call below frees what was allocated)
  B->model = m;
  B->n = n_envs;
  if (const char* ng = getenv("SOARM_NO_GRAPH")) B->use_graphs = ng[0] != '1';
  B->device = device;
  {  // the RS kernel holds one wave per SIMD (256 VGPRs + AGPRs): past 4 envs per SIMD its waves
     // run in a second round, where the quad kernel's 16-env waves still fit in one (r05: 8192
     // envs 5.2 M env-steps/s RS against 7.9 M quad)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess)
      B->rs_cap = cus * 4 * RS_EPW;
#ifdef SOARM_DIAG_SKIPP
  {  // SOARM_DIAG_SKIP: "p,p,..." pairs to skip; a leading '~' skips every pair but those
    static uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (const char* v = getenv("SOARM_DIAG_SKIP")) {
      const bool inv = *v == '~';
      for (const char* c = v + inv; *c;) {
        const int p = atoi(c);
        if (p >= 0 && p < 128) w[p >> 5] |= 1u << (p & 31);
        while (*c && *c != ',') c++;
        if (*c) c++;
      }
      if (inv)
        for (auto& x : w) x = ~x;
    }
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_diag_skip), w, sizeof(w), 0, hipMemcpyHostToDevice);
    const int stage = getenv("SOARM_DIAG_STAGE") ? atoi(getenv("SOARM_DIAG_STAGE")) : 0;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_diag_stage), &stage, sizeof(stage), 0, hipMemcpyHostToDevice);
  }
#endif
  }
  if (int rc = upload_model(m, device, &B->d_model, &B->d_prec)) return rc;
  if (!m->desc.disable_contact) {
    const size_t n = (size_t)n_envs;
    // contact rows, then two rows of Newton's zone history (zero: none)
    B->scratch_floats = ((size_t)4 * SIM_MAXCON * (2 * m->desc.nv + 4) + 2) * n;
    if (int rc = dev_alloc(B->d_scratch, B->scratch_floats, true)) return rc;
    if (int rc = dev_alloc(B->d_gpose, (size_t)m->desc.nbody * BREC * n, false)) return rc;
    if (int rc = dev_alloc(B->d_cbuf, (size_t)std::max(m->dm.nslot, 1) * 7 * n, false)) return rc;
    if (int rc = dev_alloc(B->d_ccount, (size_t)std::max(m->desc.npair, 1) * n, false)) return rc;
    if (int rc = dev_alloc(B->d_pmask, (size_t)std::max(pmask_words(m->dm), 1) * n, true)) return rc;
    if (int rc = dev_alloc(B->d_sepax, (size_t)std::max(m->desc.npair, 1) * 3 * n, true)) return rc;
  }
  *out = B.release();
  return SIM_OK;
}

void sim_batch_free(sim_batch* b) { delete b; }

int sim_batch_set_params(sim_batch* b, const sim_params* p) {
  if (!b) return fail(SIM_E_ARG, "null batch");
  b->params = p ? *p : sim_params{nullptr, nullptr, nullptr};
  b->drop_graphs();  // the parameters are bound into captured launches
  return SIM_OK;
}

static int check_state(const sim_batch* b, const sim_state* s) {
  if (!b || !s) return fail(SIM_E_ARG, "null argument");
  if (!s->qpos || !s->qvel || !s->qacc_warmstart || !s->ctrl || !s->status)
    return fail(SIM_E_ARG, "state buffers must all be set");
  return SIM_OK;
}

int sim_reset(sim_batch* b, const sim_state* s, const float* init_qpos, const float* init_qvel,
              const float* extra_qpos, uint64_t seed, int64_t env_offset, const uint8_t* mask,
              float* obs, void* stream) {
  const TraceRange tr_("sim_reset");
  if (int rc = check_state(b, s)) return rc;
  if (b->cpu) return cpu_reset(b->cpu, s, init_qpos, init_qvel, extra_qpos, seed, env_offset, mask, obs);
  hipStream_t st = (hipStream_t)stream;
  dispatch_nf(b->model->nf, [&](auto nfc) {
    constexpr int NA = 6, NF = decltype(nfc)::value;
    hipLaunchKernelGGL((k_reset<NA, NF>), grid_for(b->n), dim3(64), 0, st,
                                             b->d_model, b->n, *s, init_qpos, init_qvel, extra_qpos,
                                             (uint32_t)seed, (uint32_t)(seed >> 32), (long long)env_offset,
                                             mask, obs);
  });
  HIPCHECK(hipGetLastError());
  return SIM_OK;
}

// the row-space PGS substep (k_substep<..., RS>) for the scene with a free body, up to rs_cap envs
// (one round of waves); SOARM_RS=0 selects the quad kernel (16 envs per wave), read per env-step call
// (and part of the graph cache's key)
static bool rs_on() {
  const char* v = getenv("SOARM_RS");
  return !(v && v[0] == '0');
}

int sim_step(sim_batch* b, const sim_state* s, const float* action, int frame_skip, float* obs,
             void* stream) {
  const TraceRange tr_("sim_step");
  if (int rc = check_state(b, s)) return rc;
  if (frame_skip < 1) return fail(SIM_E_ARG, "frame_skip must be >= 1");
  if (b->cpu) return cpu_step(b->cpu, s, b->params, action, frame_skip, obs);
  hipStream_t st = (hipStream_t)stream;
  const bool con = !b->model->desc.disable_contact;
  const int sol = b->model->desc.solver;
  if (!con) {
    dispatch_nf(b->model->nf, [&](auto nfc) {
      dispatch_sol(sol, [&](auto solc) {
        constexpr int NA = 6, NF = decltype(nfc)::value, SOL = decltype(solc)::value;
        prof_mark(b, 0, st);
        if (s->qfrc_applied)
          hipLaunchKernelGGL((k_step<NA, NF, true, SOL>), grid_for(b->n), dim3(64), 0, st, b->d_model, b->n,
                             frame_skip, *s, action, obs, b->params);
        else
          hipLaunchKernelGGL((k_step<NA, NF, false, SOL>), grid_for(b->n), dim3(64), 0, st, b->d_model, b->n,
                             frame_skip, *s, action, obs, b->params);
        prof_mark(b, -1, st);
      });
    });
    HIPCHECK(hipGetLastError());
    return SIM_OK;
  }
  // contacts: geom poses, then per substep (env, pair)-parallel collide + per-env dynamics
  const int np = b->model->desc.npair;
  const bool rs = rs_on() && b->n <= b->rs_cap;
  auto enqueue = [&](hipStream_t q) {
    dispatch_nf(b->model->nf, [&](auto nfc) {
     dispatch_sol(sol, [&](auto solc) {
      constexpr int NA = 6, NF = decltype(nfc)::value, SOL = decltype(solc)::value;
      prof_mark(b, 3, q);
      {
        const TraceRange tr_("geom_poses");
        hipLaunchKernelGGL((k_geom<NA, NF>), geom_grid(b->n), dim3(64), 0, q, b->d_model, b->n, *s,
                           b->d_gpose);
      }
      prof_mark(b, -1, q);
      for (int sub = 0; sub < frame_skip; sub++) {
        if (np > 0) {
          prof_mark(b, 1, q);
          const TraceRange tr_("collide");
          launch_collide(b, q, nullptr);
          prof_mark(b, -1, q);
        }
        const bool last = sub == frame_skip - 1;
        const TraceRange tr_("substep");
        prof_mark(b, 2, q);
        auto kern = s->qfrc_applied ? k_substep<NA, NF, true, SOL> : k_substep<NA, NF, false, SOL>;
        int epb = 64 / QUAD_LPE;  // envs per 64-thread workgroup
        if constexpr (NF == 1 && SOL == SIM_SOL_PGS) {
          if (rs) {
            kern = s->qfrc_applied ? k_substep<NA, NF, true, SOL, true> : k_substep<NA, NF, false, SOL, true>;
            epb = RS_EPW;
          }
        }
        size_t lds_pad = 0;
#ifdef SOARM_PHASE_PROF
        // (diagnostic build: SOARM_LDS_PAD bytes of unused dynamic LDS cap the workgroups per CU)
        if (const char* v = getenv("SOARM_LDS_PAD")) lds_pad = (size_t)atol(v);
        // (SOARM_DIAG_NOGPOSE: the substep writes no geom records -- timing only, wrong contacts)
        const bool nogpose = getenv("SOARM_DIAG_NOGPOSE") != nullptr;
        {  // (static: a captured graph's memcpy node reads this address at every replay)
          static int f11;
          f11 = getenv("SOARM_RS_FORCE11") != nullptr;
          (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_rs_force11), &f11, sizeof(f11), 0, hipMemcpyHostToDevice, q);
        }
#else
        constexpr bool nogpose = false;
#endif
        hipLaunchKernelGGL(kern, dim3((b->n + epb - 1) / epb), dim3(64), lds_pad, q,
                           b->d_model, b->n, *s,
                           sub == 0 ? action : nullptr, last ? obs : nullptr, b->params, b->d_scratch,
                           b->d_cbuf, np > 0 ? b->d_ccount : nullptr, np > 0 ? b->d_pmask : nullptr,
                           last || nogpose ? nullptr : b->d_gpose, b->d_gpose);
        prof_mark(b, -1, q);
      }
     });
    });
  };
  if (b->prof || !b->use_graphs || roctx().push) {  // profiling / tracing brackets every launch: no graph
    enqueue(st);
    HIPCHECK(hipGetLastError());
    return SIM_OK;
  }
  // replay a captured graph of the whole env-step (one launch instead of 1 + 2 x frame_skip)
  const sim_batch::GraphKey key{*s, action, obs, frame_skip, rs};
  hipGraphExec_t exec = nullptr;
  for (auto& g : b->graphs)
    if (g.first == key) exec = g.second;
  if (!exec) {
    if (!b->cap_stream) HIPCHECK(hipStreamCreateWithFlags(&b->cap_stream, hipStreamNonBlocking));
    HIPCHECK(hipStreamBeginCapture(b->cap_stream, hipStreamCaptureModeThreadLocal));
    enqueue(b->cap_stream);
    hipGraph_t graph = nullptr;
    HIPCHECK(hipStreamEndCapture(b->cap_stream, &graph));
    const hipError_t inst = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);  // (the exec keeps what it needs; on failure nothing does)
    HIPCHECK(inst);
    if (b->graphs.size() >= 8) {  // small LRU-less cache: start over
      b->drop_graphs();
    }
    b->graphs.emplace_back(key, exec);
  }
  HIPCHECK(hipGraphLaunch(exec, st));
  return SIM_OK;
}

int sim_profile_begin(sim_batch* b) {
  if (!b) return fail(SIM_E_ARG, "null batch");
  if (b->cpu) return fail(SIM_E_ARG, "launch profiling needs a GPU batch");
  b->prof = true;
  b->ev_used = 0;
  b->ev_marks.clear();
  return SIM_OK;
}

int sim_profile_end(sim_batch* b, double* ms, int32_t* launches) {
  if (!b || !ms || !launches) return fail(SIM_E_ARG, "null argument");
  b->prof = false;
  for (int k = 0; k < SIM_PROF_KINDS; k++) ms[k] = 0, launches[k] = 0;
  for (auto& mk : b->ev_marks) {
    HIPCHECK(hipEventSynchronize(b->ev_pool[mk.second + 1]));
    float t = 0.f;
    HIPCHECK(hipEventElapsedTime(&t, b->ev_pool[mk.second], b->ev_pool[mk.second + 1]));
    ms[mk.first] += t;
    launches[mk.first] += 1;
  }
  b->ev_marks.clear();
  b->ev_used = 0;
  return SIM_OK;
}

int sim_contacts(sim_batch* b, const sim_state* s, float* out, int32_t* ncon, void* stream) {
  const TraceRange tr_("sim_contacts");
  if (int rc = check_state(b, s)) return rc;
  if (!out || !ncon) return fail(SIM_E_ARG, "null output");
  if (b->cpu) return cpu_contacts(b->cpu, s, out, ncon);
  if (b->model->desc.disable_contact) return fail(SIM_E_ARG, "model compiled with contacts disabled");
  hipStream_t st = (hipStream_t)stream;
  const int np = b->model->desc.npair;
  dispatch_nf(b->model->nf, [&](auto nfc) {
    constexpr int NA = 6, NF = decltype(nfc)::value;
    hipLaunchKernelGGL((k_geom<NA, NF>), geom_grid(b->n), dim3(64), 0, st, b->d_model, b->n, *s,
                       b->d_gpose);
  });
  if (np > 0)
    launch_collide(b, st, nullptr);
  hipLaunchKernelGGL(k_gather, grid_for(b->n), dim3(64), 0, st, b->d_model, b->n, b->d_cbuf, b->d_ccount, b->d_pmask,
                     out, ncon);
  HIPCHECK(hipGetLastError());
  return SIM_OK;
}

int sim_contact_forces(sim_batch* b, const sim_state* s, float* contacts, float* force, int32_t* ncon,
                       void* stream) {
  const TraceRange tr_("sim_contact_forces");
  if (int rc = check_state(b, s)) return rc;
  if (!force || !ncon) return fail(SIM_E_ARG, "null output");
  if (b->cpu) return cpu_contact_forces(b->cpu, s, b->params, contacts, force, ncon);
  if (b->model->desc.disable_contact) return fail(SIM_E_ARG, "model compiled with contacts disabled");
  hipStream_t st = (hipStream_t)stream;
  dispatch_nf(b->model->nf, [&](auto nfc) {
    constexpr int NA = 6, NF = decltype(nfc)::value;
    hipLaunchKernelGGL((k_geom<NA, NF>), geom_grid(b->n), dim3(64), 0, st, b->d_model, b->n, *s,
                       b->d_gpose);
  });
  if (b->model->desc.npair > 0)
    launch_collide(b, st, nullptr);
  HIPCHECK(hipGetLastError());
  // (soarm_cforce.hip: its own translation unit, so this one's kernels stay as they are)
  HIPCHECK((hipError_t)launch_contact_force(b->model->nf, b->model->desc.solver, b->d_model, b->n, *s, b->params,
                                            b->d_cbuf, b->d_pmask, contacts, force, ncon, stream));
  return SIM_OK;
}

int sim_collide_profile(sim_batch* b, const sim_state* s, double* cycles, void* stream) {
  if (int rc = check_state(b, s)) return rc;
  if (!cycles) return fail(SIM_E_ARG, "null output");
  if (b->cpu) return fail(SIM_E_ARG, "collide profiling needs a GPU batch");
  if (b->model->desc.disable_contact) return fail(SIM_E_ARG, "model compiled with contacts disabled");
  hipStream_t st = (hipStream_t)stream;
  const int np = b->model->desc.npair;
  if (np <= 0) return SIM_OK;
  unsigned long long* d_cyc = nullptr;
  HIPCHECK(hipMalloc(&d_cyc, 2 * np * sizeof(unsigned long long)));
  std::vector<unsigned long long> h(2 * np);
  const int rc = [&]() -> int {
    HIPCHECK(hipMemsetAsync(d_cyc, 0, 2 * np * sizeof(unsigned long long), st));
    dispatch_nf(b->model->nf, [&](auto nfc) {
      constexpr int NA = 6, NF = decltype(nfc)::value;
      hipLaunchKernelGGL((k_geom<NA, NF>), geom_grid(b->n), dim3(64), 0, st, b->d_model, b->n, *s,
                         b->d_gpose);
    });
    launch_collide(b, st, d_cyc);
    HIPCHECK(hipMemsetAsync(b->d_pmask, 0, (size_t)pmask_words(b->model->dm) * b->n * sizeof(uint32_t), st));
    HIPCHECK(hipMemcpyAsync(h.data(), d_cyc, 2 * np * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return SIM_OK;
  }();
  const hipError_t freed = hipFree(d_cyc);  // on every path
  if (rc) return rc;
  HIPCHECK(freed);
  for (int p = 0; p < 2 * np; p++) cycles[p] = (double)h[p];
  return SIM_OK;
}

int sim_phase_profile(double* out, int reset) {
  if (!out) return fail(SIM_E_ARG, "null output");
#ifdef SOARM_PHASE_PROF
  unsigned long long nw[24];
  std::vector<unsigned long long> w((size_t)WPH_MAXW * WPH);
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpyFromSymbol(w.data(), HIP_SYMBOL(g_wphase), w.size() * sizeof(w[0])));
  HIPCHECK(hipMemcpyFromSymbol(nw, HIP_SYMBOL(g_newton), sizeof(nw)));
  // per-wave rows (soarm_prof.h g_wphase): maxima where g_phase's layout keeps a max, sums elsewhere
  const auto is_max = [](int k) {
    return k == 8 || k == 10 || k == 15 || (k >= 23 && k <= 26) || k == 59 || k == 60 || (k >= 65 && k <= 68) ||
           k == 83;
  };
  unsigned long long h[WPH] = {};
  for (int r = 0; r < WPH_MAXW; r++)
    for (int k = 0; k < WPH; k++) {
      const unsigned long long v = w[(size_t)r * WPH + k];
      h[k] = is_max(k) ? std::max(h[k], v) : h[k] + v;
    }
  for (int k = 0; k < 77; k++) out[k] = (double)h[k];
  for (int k = 0; k < 24; k++) out[77 + k] = (double)nw[k];
  // the RS solve's split, in the slots the Newton profiler leaves free in PGS builds
  out[77 + 8] = (double)h[77], out[77 + 9] = (double)h[78], out[77 + 10] = (double)h[79];
  out[77 + 11] = (double)h[80], out[77 + 16] = (double)h[81];
  out[77 + 17] = (double)h[82], out[77 + 18] = (double)h[83], out[77 + 19] = (double)h[84];  // RS fallback waves
  for (int k = 0; k < 7; k++) out[101 + k] = (double)h[85 + k];  // (callers pass >= 108 doubles)
  if (reset) {
    void* a = nullptr;
    HIPCHECK(hipGetSymbolAddress(&a, HIP_SYMBOL(g_wphase)));
    HIPCHECK(hipMemset(a, 0, w.size() * sizeof(w[0])));
    const unsigned long long z[24] = {};
    HIPCHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_newton), z, sizeof(nw)));
  }
  return SIM_OK;
#else
  (void)reset;
  for (int k = 0; k < 19; k++) out[k] = 0.0;
  return SIM_E_ARG;  // not a profiling build
#endif
}

int sim_rand_uniform(sim_batch* b, uint64_t seed, int64_t env_offset, uint32_t counter, int k, float lo,
                     float hi, float* out, void* stream) {
  const TraceRange tr_("sim_rand_uniform");
  if (!b || !out) return fail(SIM_E_ARG, "null argument");
  if (k < 1 || k > 64) return fail(SIM_E_ARG, "k must be in [1, 64]");
  if (b->cpu) return cpu_rand_uniform(b->cpu, seed, env_offset, counter, k, lo, hi, out);
  hipLaunchKernelGGL(k_rand, grid_for(b->n), dim3(64), 0, (hipStream_t)stream, b->n, (uint32_t)seed,
                     (uint32_t)(seed >> 32), (long long)env_offset, counter, k, lo, hi - lo, out);
  HIPCHECK(hipGetLastError());
  return SIM_OK;
}

int sim_substeps(sim_batch* b, const sim_state* s, int nsub, void* stream) {
  return sim_step(b, s, nullptr, nsub, nullptr, stream);
}

int sim_bias(sim_batch* b, const sim_state* s, float* qfrc_bias, void* stream) {
  const TraceRange tr_("sim_bias");
  if (int rc = check_state(b, s)) return rc;
  if (!qfrc_bias) return fail(SIM_E_ARG, "qfrc_bias is null");
  if (b->cpu) return cpu_bias(b->cpu, s, b->params, qfrc_bias);
  hipStream_t st = (hipStream_t)stream;
  dispatch_nf(b->model->nf, [&](auto nfc) {
    constexpr int NA = 6, NF = decltype(nfc)::value;
    hipLaunchKernelGGL((k_bias<NA, NF>), grid_for(b->n), dim3(64), 0, st, b->d_model, b->n, *s, qfrc_bias,
                       b->params);
  });
  HIPCHECK(hipGetLastError());
  return SIM_OK;
}

int sim_observe(sim_batch* b, const sim_state* s, float* obs, void* stream) {
  const TraceRange tr_("sim_observe");
  if (int rc = check_state(b, s)) return rc;
  if (!obs) return fail(SIM_E_ARG, "obs is null");
  if (b->cpu) return cpu_observe(b->cpu, s, obs);
  hipStream_t st = (hipStream_t)stream;
  dispatch_nf(b->model->nf, [&](auto nfc) {
    constexpr int NA = 6, NF = decltype(nfc)::value;
    hipLaunchKernelGGL((k_observe<NA, NF>), grid_for(b->n), dim3(64), 0, st,
                                             b->d_model, b->n, *s, obs);
  });
  HIPCHECK(hipGetLastError());
  return SIM_OK;
}

int sim_ik_dls_pose(sim_batch* b, const float* target, const float* target_quat, float* q, int32_t* ok,
                    int32_t* iters, const sim_ik_opts* opts, void* stream) {
  const TraceRange tr_("sim_ik_dls");
  if (opts)
    if (int rc = check_struct(opts, "sim_ik_opts")) return rc;
  if (!b || !target || !q || !opts) return fail(SIM_E_ARG, "null argument");
  if (opts->ndof < 1 || opts->ndof > 6 || opts->max_steps < 0) return fail(SIM_E_ARG, "bad ik options");
  if (b->cpu) return cpu_ik(b->cpu, target, target_quat, q, ok, iters, *opts);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((k_ik<6>), grid_for(b->n), dim3(64), 0, st, b->d_model, b->n, target, target_quat, q, ok,
                     iters, *opts);
  HIPCHECK(hipGetLastError());
  return SIM_OK;
}

int sim_ik_dls(sim_batch* b, const float* target, float* q, int32_t* ok, int32_t* iters,
               const sim_ik_opts* opts, void* stream) {
  return sim_ik_dls_pose(b, target, nullptr, q, ok, iters, opts, stream);
}

int sim_ik_box(sim_batch* b, int nframe, const float* target, const float* target_quat, float* q,
               float* q_traj, int32_t* ok, int32_t* iters, const sim_ik_box_opts* opts, void* stream) {
  const TraceRange tr_("sim_ik_box");
  if (opts)
    if (int rc = check_struct(opts, "sim_ik_box_opts")) return rc;
  if (!b || !target || !q || !ok || !opts) return fail(SIM_E_ARG, "null argument");
  if (nframe < 1) return fail(SIM_E_ARG, "nframe must be >= 1");
  // (negated comparisons: a NaN weight or tolerance is rejected too)
  if (!(opts->w_smooth > 0.0) || !(opts->w_pos >= 0.0) || !(opts->w_rot >= 0.0) || !(opts->tol > 0.0))
    return fail(SIM_E_ARG, "bad ik weights: need w_smooth > 0, w_pos >= 0, w_rot >= 0, tol > 0");
  if (opts->site < 0 || opts->site >= b->model->desc.nsite) return fail(SIM_E_ARG, "ik site out of range");
  if (opts->ndof < 1 || opts->ndof > 6 || opts->max_steps < 0) return fail(SIM_E_ARG, "bad ik options");
  if (b->cpu) return cpu_ik_box(b->cpu, nframe, target, target_quat, q, q_traj, ok, iters, *opts);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((k_ik_box<6>), grid_for(b->n), dim3(64), 0, st, b->d_model, b->n, nframe, target, target_quat,
                     q, q_traj, ok, iters, *opts);
  HIPCHECK(hipGetLastError());
  return SIM_OK;
}

}  // extern "C"
