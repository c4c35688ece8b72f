// sim_internal.h — what the library's translation units share: the model object behind the
// opaque `sim_model` handle (built by soarm_model.hip), the error channel of sim_last_error(),
// the topology dispatch, and the CPU backend's entry points (soarm_cpu.hip, `device = -1` in
// sim_batch_create; SURVEY.md §8(b) "Threading").
#pragma once
#include <cstdint>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/soarm_sim.h"
#include "dmodel.h"

struct DevModel;  // one device's copy of the model (soarm_sim.hip, which also defines ~sim_model)

struct sim_model {
  sim_model_desc desc;
  soarm::DModel dm;  // host copy; its hull pointers stay null: bind_tables() makes a bound copy
  std::vector<uint4> hull_rec, hull_lutrec;  // climbing records (dmodel.h)
  std::vector<uint16_t> hull_ovf;
  std::vector<float> hull_sb;  // support-bound table (dmodel.h HULL_SB_K)
  int lutadr[SIM_MAXGEOM], sbadr[SIM_MAXGEOM];
  int na = 0, nf = 0;
  mutable std::mutex mu;  // guards dev (batches may be created from several threads)
  mutable std::vector<DevModel*> dev;
  ~sim_model();
};

// sets the calling thread's sim_last_error() text; returns code (soarm_model.hip)
int soarm_set_error(int code, const std::string& msg);

// the (struct_size, abi_version) header every by-pointer struct carries (soarm_sim.h)
template <class T>
int check_struct(const T* p, const char* what) {
  if (p->struct_size != (int32_t)sizeof(T) || p->abi_version != SIM_ABI_VERSION)
    return soarm_set_error(SIM_E_ARG, std::string(what) +
                                          ": struct_size / abi_version do not match this library (built for abi " +
                                          std::to_string(SIM_ABI_VERSION) + ", sizeof " + std::to_string(sizeof(T)) + ")");
  return SIM_OK;
}

// the model's DModel bound to one copy of its hull tables (a device's or the host vectors)
inline soarm::DModel bind_tables(const sim_model& m, const uint4* rec, const uint4* lutrec, const uint16_t* ovf,
                                 const float* sb) {
  soarm::DModel dm = m.dm;
  dm.hull_rec = rec, dm.hull_lutrec = lutrec, dm.hull_ovf = ovf, dm.hull_sb = sb;
  for (int g = 0; g < SIM_MAXGEOM; g++) {
    dm.geom_lutadr[g] = g < m.desc.ngeom ? m.lutadr[g] : -1;
    dm.geom_sbadr[g] = g < m.desc.ngeom ? m.sbadr[g] : -1;
  }
  return dm;
}
// the collide's records of a bound DModel, in dispatch order (row y = pair pair_order[y])
inline std::vector<soarm::PairRec> pair_records(const soarm::DModel& dm) {
  std::vector<soarm::PairRec> prec((size_t)(dm.npair > 0 ? dm.npair : 0));
  for (int y = 0; y < dm.npair; y++) prec[y] = soarm::pair_rec_make(dm, dm.pair_order[y]);
  return prec;
}

// Supported topologies: arm chain of NA=6 hinges, NF in {0, 1} free bodies.
template <class F>
void dispatch_nf(int nf, F&& f) {
  if (nf == 0)
    f(std::integral_constant<int, 0>{});
  else
    f(std::integral_constant<int, 1>{});
}
// solver of the compiled model: PGS (the north star's) or MuJoCo's default Newton
template <class F>
void dispatch_sol(int sol, F&& f) {
  if (sol == SIM_SOL_NEWTON)
    f(std::integral_constant<int, SIM_SOL_NEWTON>{});
  else
    f(std::integral_constant<int, SIM_SOL_PGS>{});
}

// ---- CPU backend: the same per-env code as the kernels (soarm_step.h, soarm_collide.h,
// soarm_env.h) compiled for the host, envs split over threads; the constraint solve is a
// dense fp32 restatement of mj_solPGS / mj_solNewton over MuJoCo's row order, on the one
// statement of the dense rows it shares with the readout's kernel (soarm_dense.h).  All pointers
// are host memory; calls are synchronous.
struct CpuBatch;
int cpu_batch_create(const sim_model* m, int n, CpuBatch** out);
// the model's contacts at qpos0 (DModel c0_*: what a soft reset's mj_forward collides), at model creation
int cpu_qpos0_contacts(sim_model* m);
// test hook (not part of the C ABI): the kernels' hull support query (soarm_collide.h hull_support,
// compiled for the host) of mesh geom g along nd local directions dirs [nd][3] -> out [nd][3]
extern "C" int soarm_test_hull_support(const sim_model* m, int g, const float* dirs, int nd, float* out);
void cpu_batch_free(CpuBatch* c);
int cpu_reset(CpuBatch* c, const sim_state* s, const float* init_qpos, const float* init_qvel,
              const float* extra_qpos, uint64_t seed, int64_t env_offset, const uint8_t* mask, float* obs);
int cpu_step(CpuBatch* c, const sim_state* s, const sim_params& p, const float* action, int frame_skip,
             float* obs);
int cpu_bias(CpuBatch* c, const sim_state* s, const sim_params& p, float* qfrc_bias);
int cpu_observe(CpuBatch* c, const sim_state* s, float* obs);
int cpu_contacts(CpuBatch* c, const sim_state* s, float* out, int32_t* ncon);
int cpu_contact_forces(CpuBatch* c, const sim_state* s, const sim_params& p, float* contacts, float* force,
                       int32_t* ncon);
int cpu_rand_uniform(CpuBatch* c, uint64_t seed, int64_t env_offset, uint32_t counter, int k, float lo, float hi,
                     float* out);

// ---- the contact-force readout's kernel (soarm_cforce.hip: k_contact_force, its own translation
// unit): launched by sim_contact_forces after k_geom + the collide, on the collide's output
// (cbuf, pmask; it clears the mask as k_gather does).  Returns a hipError_t as int.
int launch_contact_force(int nf, int sol, const soarm::DModel* d_model, int n, const sim_state& st,
                         const sim_params& pp, const float* cbuf, uint32_t* pmask, float* contacts, float* force,
                         int32_t* ncon, void* stream);
int cpu_ik(CpuBatch* c, const float* target, const float* target_quat, float* q, int32_t* ok, int32_t* iters,
           const sim_ik_opts& o);
int cpu_ik_box(CpuBatch* c, int nframe, const float* target, const float* target_quat, float* q, float* q_traj,
               int32_t* ok, int32_t* iters, const sim_ik_box_opts& o);
