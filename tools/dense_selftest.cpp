// dense_selftest.cpp — the CPU backend's dense constraint solve (csrc/soarm_cpu.hip on
// csrc/soarm_dense.h) and the model build (csrc/soarm_model.hip) as a stand-alone program for the
// host sanitizers.  No GPU; nothing is loaded into an interpreter.  sim_step and sim_contact_forces
// live in soarm_sim.hip beside the kernels, so the program calls what they call for `device = -1`:
// cpu_batch_create, cpu_step, cpu_contact_forces (sim_internal.h).
//
// Its inputs are compiled-model files and one state file per scene, written in the same shell call
// (the states carry contacts up to the cap and joints past both sides of their range):
//
//   D=$(mktemp -d) && python - "$D" <<'EOF'
//   import sys, numpy as np
//   sys.path[:0] = [".", "tests", "oracle"]
//   import soarm_pkg, contact_forces_ref as F, contact_overflow_ref as R, joint_limits_ref as J
//   for solver in ("PGS", "Newton"):
//       pool = J.states("pool")
//       for scene, cm, sts in (("pick", R.model(solver), [R.take(R.fixture()["deep"], range(4)), J.for_model(R.model(solver), pool)]),
//                              ("arm", F.arm_model(solver), [F.arm_states(solver), J.for_model(F.arm_model(solver), pool)])):
//           cm.save(f"{sys.argv[1]}/{scene}_{solver}.mdl")
//           st = {k: np.concatenate([s[k] for s in sts]) for k in R.KEYS}
//           with open(f"{sys.argv[1]}/{scene}.state", "wb") as f:
//               np.array([len(st["qpos"])] + [st[k].shape[1] for k in R.KEYS], np.int32).tofile(f)
//               for k in R.KEYS:
//                   st[k].T.astype(np.float32).tofile(f)
//   EOF
//   hipcc -std=c++17 -O1 -g -x hip --offload-host-only -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all tools/dense_selftest.cpp lerobot-mujoco-sim2real_amd/csrc/soarm_cpu.hip \
//       lerobot-mujoco-sim2real_amd/csrc/soarm_model.hip -fsanitize=address,undefined -lpthread -o $D/dense_selftest \
//     && $D/dense_selftest $D
//
// Prints "selftest ok" and exits 0; any failed expectation exits 1 with a message.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../lerobot-mujoco-sim2real_amd/csrc/sim_internal.h"

sim_model::~sim_model() {}  // (soarm_sim.hip's frees the device copies: a host-only program has none)

#define REQUIRE(c)                                                        \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, sim_last_error()); \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

struct State {
  int n = 0, dim[4] = {};          // envs; nq, nv, nv, nu
  std::vector<float> f[4];         // qpos, qvel, qacc_warmstart, ctrl: [field][env]
};

static State read_state(const std::string& path) {
  State s;
  FILE* fp = std::fopen(path.c_str(), "rb");
  REQUIRE(fp);
  int32_t h[5];
  REQUIRE(std::fread(h, 4, 5, fp) == 5);
  s.n = h[0];
  for (int k = 0; k < 4; k++) {
    s.dim[k] = h[1 + k];
    s.f[k].resize((size_t)s.dim[k] * s.n);
    REQUIRE(std::fread(s.f[k].data(), 4, s.f[k].size(), fp) == s.f[k].size());
  }
  std::fclose(fp);
  return s;
}

// one readout and one env-step of the model's CPU batch at the states; returns contacts seen
static int run(const std::string& dir, const std::string& scene, const std::string& solver, bool with_params) {
  sim_model* m = nullptr;
  REQUIRE(sim_model_load((dir + "/" + scene + "_" + solver + ".mdl").c_str(), &m) == SIM_OK && m);
  const State s0 = read_state(dir + "/" + scene + ".state");
  const int n = s0.n, nv = m->desc.nv;
  REQUIRE(s0.dim[0] == m->desc.nq && s0.dim[1] == nv && s0.dim[3] == m->desc.nu);
  int nlimit = 0;  // joints past a side of their range: each is a limit row of the solve
  for (int j = 0; j < 6; j++)
    for (int e = 0; e < n; e++) {
      const float q = s0.f[0][(size_t)j * n + e];
      nlimit += m->desc.jnt_limited[j] && (q < m->desc.jnt_range[j][0] || q > m->desc.jnt_range[j][1]);
    }
  REQUIRE(nlimit > 0);

  CpuBatch* b = nullptr;
  REQUIRE(cpu_batch_create(m, n, &b) == SIM_OK && b);
  State s = s0;
  std::vector<int32_t> status(n, 0), nc(n, 0);
  std::vector<float> ncon(n, 0.f), applied((size_t)nv * n, 0.f), obs((size_t)n * (3 + m->desc.obs_nq));
  std::vector<float> con((size_t)n * SIM_MAXCON * 8), force((size_t)n * SIM_MAXCON * 6), scale(n), fric(n);
  for (int e = 0; e < n; e++) scale[e] = 0.8f + 0.05f * (float)(e % 8), fric[e] = 0.5f + 0.1f * (float)(e % 5);
  for (size_t i = 0; i < applied.size(); i++) applied[i] = 0.01f * (float)((int)(i % 7) - 3);
  const sim_state st{s.f[0].data(), s.f[1].data(), s.f[2].data(), s.f[3].data(), status.data(), ncon.data(),
                     with_params ? applied.data() : nullptr};
  const sim_params pp = with_params ? sim_params{scale.data(), fric.data(), scale.data()} : sim_params{};
  REQUIRE(cpu_contact_forces(b, &st, pp, con.data(), force.data(), nc.data()) == SIM_OK);
  REQUIRE(cpu_contact_forces(b, &st, pp, nullptr, force.data(), nc.data()) == SIM_OK);
  REQUIRE(s.f[0] == s0.f[0] && s.f[1] == s0.f[1] && s.f[2] == s0.f[2]);  // a pure readout
  int total = 0, full = 0;
  for (int e = 0; e < n; e++) total += nc[e], full += nc[e] == SIM_MAXCON;
  std::vector<float> action((size_t)n * m->desc.nact);
  for (int e = 0; e < n; e++)
    for (int k = 0; k < m->desc.nact; k++) action[(size_t)e * m->desc.nact + k] = s0.f[3][(size_t)k * n + e];
  REQUIRE(cpu_step(b, &st, pp, action.data(), 4, obs.data()) == SIM_OK);
  for (float v : s.f[1]) REQUIRE(v == v);
  for (float v : force) REQUIRE(v == v);
  std::printf("%s %s%s: %d envs, %d contacts (%d envs at the cap), %d joints past a limit\n", scene.c_str(),
              solver.c_str(), with_params ? " + params, qfrc_applied" : "", n, total, full, nlimit);
  cpu_batch_free(b);
  sim_model_free(m);
  return total;
}

int main(int argc, char** argv) {
  REQUIRE(argc == 2);
  for (int pass = 0; pass < 2; pass++)  // everything created and freed twice over
    for (const char* scene : {"pick", "arm"})
      for (const char* solver : {"PGS", "Newton"})
        for (int with_params = 0; with_params < 2; with_params++) REQUIRE(run(argv[1], scene, solver, with_params) > 0);
  std::puts("selftest ok");
  return 0;
}
