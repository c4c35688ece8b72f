// soarm_model.hip — the model compiler's back end: sim_model_desc (include/soarm_sim.h) -> the
// float DModel the kernels read (dmodel.h) and the hull tables the collide reads through PairRec,
// plus the compiled-model file format.  Host code only: built with --offload-host-only, it launches
// nothing and allocates no device memory (the per-device upload is soarm_sim.hip's).  It also owns
// the one error slot behind sim_last_error().
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include <sched.h>

#include "sim_internal.h"
#include "soarm_collide.h"  // CON_MAXG

using namespace soarm;

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;
int soarm_set_error(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
static int fail(int code, const std::string& msg) { return soarm_set_error(code, msg); }

// ------------------------------------------------------------------ desc -> DModel
static int host_threads() {
  int n = 1;
  cpu_set_t set;
  CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof(set), &set) == 0)
    n = CPU_COUNT(&set);
  else
    n = (int)std::thread::hardware_concurrency();
  return std::min(16, std::max(1, n));
}

static float host_impedance(const double* si, double pos, double margin) {
  double dmin = std::fmin(std::fmax(si[0], 1e-4), 0.9999), dmax = std::fmin(std::fmax(si[1], 1e-4), 0.9999);
  if (dmin == dmax || si[2] <= 1e-15) return 0.5 * (dmin + dmax);
  double x = std::fabs((pos - margin) / si[2]);
  if (x >= 1) return dmax;
  if (x <= 0) return dmin;
  double y = si[4] == 1 ? x
             : x <= si[3] ? std::pow(x, si[4]) / std::pow(si[3], si[4] - 1)
                          : 1 - std::pow(1 - x, si[4]) / std::pow(1 - si[3], si[4] - 1);
  return dmin + y * (dmax - dmin);
}
static void host_KB(const double* solref, const double* solimp, double timestep, float KB[2]) {
  double dmax = std::fmin(std::fmax(solimp[1], 1e-4), 0.9999);
  if (solref[0] > 0) {
    double tc = std::fmax(solref[0], 2 * timestep), dr = solref[1];
    KB[0] = (float)(1.0 / (dmax * dmax * tc * tc * dr * dr));
    KB[1] = (float)(2.0 / (dmax * tc));
  } else {
    KB[0] = (float)(-solref[0] / (dmax * dmax));
    KB[1] = (float)(-solref[1] / dmax);
  }
}
static void quat2mat_h(float R[9], const double* q) {
  double w = q[0], x = q[1], y = q[2], z = q[3];
  double n = std::sqrt(w * w + x * x + y * y + z * z);
  w /= n, x /= n, y /= n, z /= n;
  R[0] = 1 - 2 * (y * y + z * z), R[1] = 2 * (x * y - w * z), R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z), R[4] = 1 - 2 * (x * x + z * z), R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y), R[7] = 2 * (y * z + w * x), R[8] = 1 - 2 * (x * x + y * y);
}

// what the kernels support: topology, sizes, features.  Sets the arm's hinge count and the
// number of free bodies.
static int validate_desc(const sim_model_desc& d, int& na_out, int& nf_out) {
  // topology: world, welded base, serial hinge chain, then free bodies under the world
  if (d.nbody < 3 || d.nbody > SIM_MAXBODY) return fail(SIM_E_MODEL, "nbody out of range");
  if (d.body_parentid[1] != 0 || d.body_jntnum[1] != 0)
    return fail(SIM_E_MODEL, "body 1 must be a welded base under the world");
  int na = 0;
  int b = 2;
  for (; b < d.nbody; b++) {
    if (d.body_parentid[b] != b - 1) break;
    if (d.body_jntnum[b] != 1 || d.jnt_type[d.body_jntadr[b]] != SIM_JNT_HINGE)
      return fail(SIM_E_MODEL, "chain bodies must carry exactly one hinge");
    int j = d.body_jntadr[b];
    if (j != na || d.jnt_dofadr[j] != na || d.jnt_qposadr[j] != na)
      return fail(SIM_E_MODEL, "chain hinge addresses must equal their chain index");
    na++;
  }
  int nf = 0;
  for (; b < d.nbody; b++) {
    if (d.body_parentid[b] != 0 || d.body_jntnum[b] != 1 ||
        d.jnt_type[d.body_jntadr[b]] != SIM_JNT_FREE)
      return fail(SIM_E_MODEL, "bodies after the chain must be free bodies under the world");
    int j = d.body_jntadr[b];
    if (d.jnt_dofadr[j] != na + 6 * nf || d.jnt_qposadr[j] != na + 7 * nf)
      return fail(SIM_E_MODEL, "free joint addresses out of order");
    nf++;
  }
  if (na != 6 || nf > 1) return fail(SIM_E_MODEL, "kernels are compiled for a 6-hinge arm + <=1 free body");
  if (d.solver != SIM_SOL_PGS && d.solver != SIM_SOL_NEWTON)
    return fail(SIM_E_MODEL, "solver must be PGS or Newton");
  if (d.ccd != SIM_CCD_MPR && d.ccd != SIM_CCD_NATIVE) return fail(SIM_E_MODEL, "ccd must be MPR or native");
  if (d.nv != na + 6 * nf || d.nq != na + 7 * nf) return fail(SIM_E_MODEL, "nq/nv mismatch");
  if (d.nu > na) return fail(SIM_E_MODEL, "more actuators than arm hinges");
  for (int a = 0; a < d.nu; a++)
    if (d.actuator_trnid[a] != a) return fail(SIM_E_MODEL, "actuator a must drive joint a");
  for (int i = na; i < d.nv; i++)
    if (d.dof_frictionloss[i] > 0) return fail(SIM_E_MODEL, "frictionloss on free dofs unsupported");
  // one limit row per joint at a time (the kernels' LDS holds NA): both sides active at once needs
  // range width < 2 margin
  for (int j = 0; j < na; j++)
    if (d.jnt_limited[j] && d.jnt_range[j][1] - d.jnt_range[j][0] < 2.0 * d.jnt_margin[j])
      return fail(SIM_E_MODEL, "joint margin wider than half its range (both limit rows active) unsupported");
  if (d.nact > na || d.obs_nq > na) return fail(SIM_E_MODEL, "obs/act larger than the arm");
  for (int k = 0; k < d.obs_nq; k++)
    if (d.obs_qadr[k] >= na) return fail(SIM_E_MODEL, "observed joints must be arm hinges");
  for (int g = 0; g < d.ngeom; g++) {
    int t = d.geom_type[g];
    if (t != SIM_GEOM_PLANE && t != SIM_GEOM_BOX && t != SIM_GEOM_MESH)
      return fail(SIM_E_MODEL, "geom type unsupported by the kernels");
    if (d.geom_condim[g] != 3) return fail(SIM_E_MODEL, "only condim 3 contacts supported");
  }
  if (!d.disable_contact && d.ngeom > CON_MAXG) return fail(SIM_E_MODEL, "too many collidable geoms");
  na_out = na, nf_out = nf;
  return SIM_OK;
}

// the DModel's constants from a validated desc (na: the arm's hinges); the hull pointers and
// geom_lutadr / geom_sbadr stay zero here (bind_tables, sim_internal.h)
static int fill_dmodel(const sim_model_desc& d, int na, DModel& m) {
  std::memset(&m, 0, sizeof(m));
  m.nq = d.nq, m.nv = d.nv, m.nu = d.nu, m.ngeom = d.ngeom, m.npair = d.npair, m.nact = d.nact;
  m.obs_site = d.obs_site, m.obs_nq = d.obs_nq;
  for (int k = 0; k < SIM_MAXOBSQ; k++) m.obs_qadr[k] = d.obs_qadr[k];
  m.iterations = d.iterations, m.disable_contact = d.disable_contact;
  m.ccd = d.ccd;
  bool anyd = false;
  for (int i = 0; i < d.nv; i++) anyd |= d.dof_damping[i] > 0;
  m.eulerdamp = (!d.disable_eulerdamp && anyd) ? 1 : 0;
  m.nhullvert = d.nhullvert;
  m.timestep = (float)d.timestep, m.impratio = (float)d.impratio;
  m.tolerance = (float)d.tolerance;
  m.pgs_scale = (float)(1.0 / ((d.meaninertia > 1e-15 ? d.meaninertia : 1.0) * std::max(1, d.nv)));
  for (int k = 0; k < 3; k++) m.gravity[k] = (float)d.gravity[k];
  for (int b2 = 0; b2 < d.nbody; b2++) {
    for (int k = 0; k < 3; k++) {
      m.body_pos[b2][k] = (float)d.body_pos[b2][k];
      m.body_ipos[b2][k] = (float)d.body_ipos[b2][k];
      m.body_inertia[b2][k] = (float)d.body_inertia[b2][k];
    }
    double qn = 0;
    for (int k = 0; k < 4; k++) qn += d.body_quat[b2][k] * d.body_quat[b2][k];
    for (int k = 0; k < 4; k++) m.body_quat[b2][k] = (float)(d.body_quat[b2][k] / std::sqrt(qn));
    quat2mat_h(m.body_imat[b2], d.body_iquat[b2]);
    m.body_mass[b2] = (float)d.body_mass[b2];
    m.body_invweight0[b2][0] = (float)d.body_invweight0[b2][0];
    m.body_invweight0[b2][1] = (float)d.body_invweight0[b2][1];
  }
  for (int j = 0; j < d.njnt; j++) {
    for (int k = 0; k < 3; k++) {
      m.jnt_pos[j][k] = (float)d.jnt_pos[j][k];
      m.jnt_axis[j][k] = (float)d.jnt_axis[j][k];
    }
    m.jnt_range[j][0] = (float)d.jnt_range[j][0], m.jnt_range[j][1] = (float)d.jnt_range[j][1];
    for (int k = 0; k < 5; k++) m.jnt_solimp[j][k] = (float)d.jnt_solimp[j][k];
    host_KB(d.jnt_solref[j], d.jnt_solimp[j], d.timestep, m.jnt_KB[j]);
    m.jnt_margin[j] = (float)d.jnt_margin[j];
    m.jnt_limited[j] = d.jnt_limited[j] && d.jnt_type[j] == SIM_JNT_HINGE;
  }
  for (int i = 0; i < d.nq; i++) m.qpos0[i] = (float)d.qpos0[i];
  for (int i = 0; i < d.nv; i++) {
    m.dof_armature[i] = (float)d.dof_armature[i];
    m.dof_damping[i] = (float)d.dof_damping[i];
    m.dof_frictionloss[i] = (float)d.dof_frictionloss[i];
    m.dof_invweight0[i] = (float)d.dof_invweight0[i];
    double imp = host_impedance(d.dof_solimp[i], 0.0, 0.0);
    m.dof_fricR[i] = (float)std::fmax(1e-15, (1 - imp) * d.dof_invweight0[i] / imp);
    float KB[2];
    host_KB(d.dof_solref[i], d.dof_solimp[i], d.timestep, KB);
    m.dof_fricB[i] = KB[1];
  }
  for (int g = 0; g < d.ngeom; g++) {
    m.geom_type[g] = d.geom_type[g], m.geom_bodyid[g] = d.geom_bodyid[g];
    m.geom_hulladr[g] = d.geom_hulladr[g], m.geom_hullnum[g] = d.geom_hullnum[g];
    for (int k = 0; k < 3; k++) {
      m.geom_pos[g][k] = (float)d.geom_pos[g][k];
      m.geom_size[g][k] = (float)d.geom_size[g][k];
      m.geom_center[g][k] = (float)d.geom_aabb[g][k];
      m.geom_half[g][k] = (float)d.geom_aabb[g][3 + k];
    }
    quat2mat_h(m.geom_mat[g], d.geom_quat[g]);
    for (int k = 0; k < 3; k++) {
      double c = d.geom_pos[g][k];
      for (int j = 0; j < 3; j++) c += (double)m.geom_mat[g][3 * k + j] * d.geom_aabb[g][j];
      m.geom_cbody[g][k] = (float)c;
    }
    m.geom_rbound[g] = (float)d.geom_rbound[g];
    m.geom_friction[g] = (float)d.geom_friction[g][0];
  }
  for (int p = 0; p < d.npair; p++) {
    int g1 = d.pair_geom1[p], g2 = d.pair_geom2[p];
    m.pair_geom1[p] = g1, m.pair_geom2[p] = g2;
    double sr[2], si[5];
    for (int k = 0; k < 2; k++) sr[k] = 0.5 * (d.geom_solref[g1][k] + d.geom_solref[g2][k]);
    for (int k = 0; k < 5; k++) {
      si[k] = 0.5 * (d.geom_solimp[g1][k] + d.geom_solimp[g2][k]);
      m.pair_solimp[p][k] = (float)si[k];
    }
    host_KB(sr, si, d.timestep, m.pair_KB[p]);
    m.pair_margin[p] = (float)std::fmax(d.geom_margin[g1], d.geom_margin[g2]);
    m.pair_tran[p] = (float)(d.body_invweight0[d.geom_bodyid[g1]][0] + d.body_invweight0[d.geom_bodyid[g2]][0]);
    m.pair_friction[p] = (float)std::fmax(d.geom_friction[g1][0], d.geom_friction[g2][0]);
    // slot capacity: box-box and plane-box can return up to 4 contacts, the rest 1
    const int t1 = d.geom_type[g1], t2 = d.geom_type[g2];
    const int cap = (t2 == SIM_GEOM_BOX && (t1 == SIM_GEOM_BOX || t1 == SIM_GEOM_PLANE)) ? 4 : 1;
    m.pair_slot[p] = m.nslot;
    m.pair_cap[p] = cap;
    m.pair_cq[p] = cap > 1 ? m.ncq++ : -1;
    m.pair_body1[p] = d.geom_bodyid[g1], m.pair_body2[p] = d.geom_bodyid[g2];
    m.nslot += cap;
  }
  if (m.ncq > 16) return fail(SIM_E_MODEL, "more than 16 box-box / plane-box pairs");
  for (int w = 0; w < (MAXP + 31) / 32; w++)
    m.pair_mw_multi[w] = m.pair_mw_arm[w] = m.pair_mw_free[w] = 0u, m.pair_cqbase[w] = 0;
  for (int p = 0, q = 0; p < d.npair; p++) {
    const int w = p >> 5;
    const uint32_t bit = 1u << (p & 31);
    if ((p & 31) == 0) m.pair_cqbase[w] = q;
    if (m.pair_cq[p] >= 0) m.pair_mw_multi[w] |= bit, q++;
    const int b1 = m.pair_body1[p], b2 = m.pair_body2[p];
    if ((b1 >= 2 && b1 < 2 + na) || (b2 >= 2 && b2 < 2 + na)) m.pair_mw_arm[w] |= bit;
    if (b1 >= 2 + na || b2 >= 2 + na) m.pair_mw_free[w] |= bit;
  }
  {  // collide dispatch order: by class (convex-convex and box-box with the free body or the world's
     // boxes, then the arm's own mesh pairs, then plane pairs), later pairs first within a class
     // (round 4's order): a class-0 pair dispatched among the last workgroups started after the
     // grid had filled and set the launch's tail
    auto cls = [&](int p) {
      const int t1 = d.geom_type[d.pair_geom1[p]], t2 = d.geom_type[d.pair_geom2[p]];
      if (t1 == SIM_GEOM_PLANE || t2 == SIM_GEOM_PLANE) return 2;
      const int b1 = d.geom_bodyid[d.pair_geom1[p]], b2 = d.geom_bodyid[d.pair_geom2[p]];
      return (b1 == 0 || b2 == 0 || b1 >= 2 + na || b2 >= 2 + na) ? 0 : 1;
    };
    int k = 0;
    for (int c = 0; c < 3; c++)
      for (int p = d.npair - 1; p >= 0; p--)
        if (cls(p) == c) m.pair_order[k++] = p;
    for (int y = 0; y < d.npair; y++) m.pair_rec[m.pair_order[y]] = y;
  }
  // free bodies: the kernels use a diagonal 6x6 mass block, which needs the inertia frame at
  // the body frame (ipos = 0, iquat = identity) — true for the build-defined cube
  m.free_diag = 1;
  for (int b2 = 2 + na; b2 < d.nbody; b2++) {
    const double* ip = d.body_ipos[b2];
    const double* iq = d.body_iquat[b2];
    if (ip[0] != 0 || ip[1] != 0 || ip[2] != 0 || iq[0] != 1 || iq[1] != 0 || iq[2] != 0 || iq[3] != 0)
      return fail(SIM_E_MODEL, "free bodies need ipos = 0 and an inertia frame equal to the body frame");
  }
  for (int s = 0; s < d.nsite; s++) {
    m.site_bodyid[s] = d.site_bodyid[s];
    for (int k = 0; k < 3; k++) m.site_pos[s][k] = (float)d.site_pos[s][k];
    double qn = 0;
    for (int k = 0; k < 4; k++) qn += d.site_quat[s][k] * d.site_quat[s][k];
    for (int k = 0; k < 4; k++) m.site_quat[s][k] = (float)(qn > 0 ? d.site_quat[s][k] / std::sqrt(qn) : k == 0);
  }
  for (int a = 0; a < d.nu; a++) {
    m.act_ctrllimited[a] = d.actuator_ctrllimited[a];
    m.act_forcelimited[a] = d.actuator_forcelimited[a];
    m.act_gear[a] = (float)d.actuator_gear[a];
    m.act_gain[a] = (float)d.actuator_gainprm[a];
    for (int k = 0; k < 3; k++) m.act_bias[a][k] = (float)d.actuator_biasprm[a][k];
    for (int k = 0; k < 2; k++) {
      m.act_ctrlrange[a][k] = (float)d.actuator_ctrlrange[a][k];
      m.act_forcerange[a][k] = (float)d.actuator_forcerange[a][k];
    }
  }
  return SIM_OK;
}

// ------------------------------------------------------------------ hull tables
// Called in this order by sim_model_create; each reads the caller's hull arrays (hull_vert
// [nhullvert][3], hull_adr CSR, hull_adj local ids) and the earlier tables it names.

static int count_meshes(const sim_model_desc& d) {
  int nmesh = 0;
  for (int g = 0; g < d.ngeom; g++) nmesh += d.geom_type[g] == SIM_GEOM_MESH;
  return nmesh;
}

// support start table: per mesh geom, the argmax vertex of each cube-map cell's centre direction.
// Reads hull_vert only; fills M->lutadr.  The table itself only feeds hull_cell_records.
static int hull_start_table(sim_model* M, const float* hull_vert, std::vector<uint16_t>& lut) {
  const sim_model_desc& d = M->desc;
  lut.assign((size_t)std::max(count_meshes(d), 1) * HULL_LUT_CELLS, 0);
  for (int g = 0, k = 0; g < d.ngeom; g++) {
    M->lutadr[g] = -1;
    if (d.geom_type[g] != SIM_GEOM_MESH) continue;
    if (d.geom_hullnum[g] > 65535) return fail(SIM_E_MODEL, "hull with more than 65535 vertices");
    M->lutadr[g] = k * HULL_LUT_CELLS;
    const float* hv = hull_vert + 3 * (size_t)d.geom_hulladr[g];
    const int nv = d.geom_hullnum[g];
    uint16_t* out = &lut[(size_t)k * HULL_LUT_CELLS];
    // exact argmax per cell (brute force), cells split over host threads
    auto cells = [hv, nv, out](int c0, int c1) {
      for (int c = c0; c < c1; c++) {
        double d[3];
        lut_dir(c, d);
        int best = 0;
        double bd = -1e300;
        for (int i = 0; i < nv; i++) {
          const double s = d[0] * hv[3 * i] + d[1] * hv[3 * i + 1] + d[2] * hv[3 * i + 2];
          if (s > bd) bd = s, best = i;
        }
        out[c] = (uint16_t)best;
      }
    };
    // pool sized to the CPUs this process may run on (the GPU box gives each job a share of
    // the machine), at most 16; if a thread cannot be started its cells run on this one
    const int nt = host_threads();
    std::vector<std::thread> pool;
    int started = 0;
    for (int t = 0; t < nt; t++) {
      const int c0 = (int)((long)HULL_LUT_CELLS * t / nt), c1 = (int)((long)HULL_LUT_CELLS * (t + 1) / nt);
      if (t + 1 < nt && started == t) {
        try {
          pool.emplace_back(cells, c0, c1);
          started++;
          continue;
        } catch (...) {
        }
      }
      cells(c0, c1);
    }
    for (auto& th : pool) th.join();
    k++;
  }
  return SIM_OK;
}

// climbing records M->hull_rec (HULL_LUTREC uint4 per vertex): coordinates and degree, the first 8
// neighbour ids, then those neighbours' coordinates and ids; neighbours past 8 go to M->hull_ovf.
// Reads the three hull arrays, no earlier table.
static int hull_climb_records(sim_model* M, const float* hull_vert, const int32_t* hull_adr,
                              const int32_t* hull_adj) {
  const sim_model_desc& d = M->desc;
  M->hull_rec.assign((size_t)HULL_LUTREC * std::max(d.nhullvert, 1), make_uint4(0, 0, 0, 0));
  M->hull_ovf.assign(1, 0);
  for (int g = 0; g < d.ngeom; g++) {
    if (d.geom_type[g] != SIM_GEOM_MESH) continue;
    const int base = d.geom_hulladr[g];
    for (int li = 0; li < d.geom_hullnum[g]; li++) {
      const int i = base + li;
      const int32_t a0 = hull_adr[i], deg = hull_adr[i + 1] - a0;
      const size_t ovf = M->hull_ovf.size();
      for (int a = 8; a < deg; a++) M->hull_ovf.push_back((uint16_t)hull_adj[a0 + a]);
      if (ovf >= (1u << 24)) return fail(SIM_E_MODEL, "hull adjacency overflow table too large");
      uint32_t xb, yb, zb;
      memcpy(&xb, &hull_vert[3 * i], 4), memcpy(&yb, &hull_vert[3 * i + 1], 4), memcpy(&zb, &hull_vert[3 * i + 2], 4);
      M->hull_rec[HULL_LUTREC * i] = make_uint4(xb, yb, zb, (uint32_t)deg | (deg > 8 ? (uint32_t)ovf << 8 : 0u));
      uint32_t id[8];
      for (int a = 0; a < 8; a++) id[a] = a < deg ? (uint32_t)hull_adj[a0 + a] : (uint32_t)li;
      M->hull_rec[HULL_LUTREC * i + 1] =
          make_uint4(id[0] | id[1] << 16, id[2] | id[3] << 16, id[4] | id[5] << 16, id[6] | id[7] << 16);
    }
    for (int li = 0; li < d.geom_hullnum[g]; li++)  // neighbour k in record order (padding = the vertex itself)
      for (int k = 0; k < 8; k++) {
        const uint4 ids = M->hull_rec[HULL_LUTREC * (base + li) + 1];
        const uint32_t w[4] = {ids.x, ids.y, ids.z, ids.w};
        const uint32_t u = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
        const uint4 r = M->hull_rec[HULL_LUTREC * (base + u)];
        M->hull_rec[HULL_LUTREC * (base + li) + 2 + k] = make_uint4(r.x, r.y, r.z, u);
      }
  }
  return SIM_OK;
}

// support-bound table M->hull_sb: exact support at every grid point, rounded up to the next float.
// Reads hull_vert only; fills M->sbadr.
static void hull_support_bounds(sim_model* M, const float* hull_vert) {
  const sim_model_desc& d = M->desc;
  M->hull_sb.assign((size_t)std::max(count_meshes(d), 1) * 6 * HULL_SB_FACE, 0.f);
  for (int g = 0, k = 0; g < d.ngeom; g++) {
    M->sbadr[g] = -1;
    if (d.geom_type[g] != SIM_GEOM_MESH) continue;
    M->sbadr[g] = k * 6 * HULL_SB_FACE;
    const float* hv = hull_vert + 3 * (size_t)d.geom_hulladr[g];
    const int nv = d.geom_hullnum[g];
    for (int f = 0; f < 6; f++)
      for (int i = 0; i <= HULL_SB_K; i++)
        for (int j = 0; j <= HULL_SB_K; j++) {
          const double u = -1.0 + 2.0 * i / HULL_SB_K, v = -1.0 + 2.0 * j / HULL_SB_K, sg = (f & 1) ? -1.0 : 1.0;
          double dir[3];
          switch (f >> 1) {
            case 0: dir[0] = sg, dir[1] = u, dir[2] = v; break;
            case 1: dir[0] = u, dir[1] = sg, dir[2] = v; break;
            default: dir[0] = u, dir[1] = v, dir[2] = sg; break;
          }
          double bd = -1e300;
          for (int a = 0; a < nv; a++)
            bd = std::fmax(bd, dir[0] * hv[3 * a] + dir[1] * hv[3 * a + 1] + dir[2] * hv[3 * a + 2]);
          M->hull_sb[(size_t)M->sbadr[g] + f * HULL_SB_FACE + i * (HULL_SB_K + 1) + j] =
              std::nextafter((float)bd, 3.0e38f);
        }
    k++;
  }
}

// start-cell records M->hull_lutrec: per cube-map cell, a copy of its start vertex's climbing
// record.  Reads the start table (lut, M->lutadr) and M->hull_rec.
static void hull_cell_records(sim_model* M, const std::vector<uint16_t>& lut) {
  const sim_model_desc& d = M->desc;
  M->hull_lutrec.assign((size_t)HULL_LUTREC * lut.size(), make_uint4(0, 0, 0, 0));
  for (int g = 0; g < d.ngeom; g++) {
    if (M->lutadr[g] < 0) continue;
    const size_t base = (size_t)d.geom_hulladr[g];
    for (int c = 0; c < HULL_LUT_CELLS; c++) {
      const size_t cell = (size_t)M->lutadr[g] + c;
      const size_t v = base + lut[cell];
      for (int k = 0; k < HULL_LUTREC; k++)  // (a copy of its start vertex's record)
        M->hull_lutrec[HULL_LUTREC * cell + k] = M->hull_rec[HULL_LUTREC * v + k];
    }
  }
}

// ============================================================== C ABI
extern "C" {

const char* sim_last_error(void) { return g_err.c_str(); }

int sim_model_create(const sim_model_desc* desc, const float* hull_vert, const int32_t* hull_adr,
                     const int32_t* hull_adj, sim_model** out) {
  if (!desc || !out) return fail(SIM_E_ARG, "null argument");
  *out = nullptr;
  if (int rc = check_struct(desc, "sim_model_desc")) return rc;
  std::unique_ptr<sim_model> M(new sim_model());
  M->desc = *desc;
  if (int rc = validate_desc(*desc, M->na, M->nf)) return rc;
  if (int rc = fill_dmodel(*desc, M->na, M->dm)) return rc;
  if (desc->nhullvert > 0 && (!hull_vert || !hull_adr || !hull_adj)) return fail(SIM_E_ARG, "hull arrays missing");
  // the climbing records pack a vertex's degree into 8 bits beside a 24-bit offset
  for (int i = 0; i < desc->nhullvert; i++) {
    const int32_t a0 = hull_adr[i], deg = hull_adr[i + 1] - a0;
    if (a0 < 0 || a0 >= (1 << 24) || deg < 0 || deg > 255)
      return fail(SIM_E_MODEL, "hull graph too large for packed vertex records");
  }
  std::vector<uint16_t> lut;
  if (int rc = hull_start_table(M.get(), hull_vert, lut)) return rc;
  if (int rc = hull_climb_records(M.get(), hull_vert, hull_adr, hull_adj)) return rc;
  hull_support_bounds(M.get(), hull_vert);
  hull_cell_records(M.get(), lut);
  if (int rc = cpu_qpos0_contacts(M.get())) return rc;  // (the hull tables above are its input)
  *out = M.release();
  return SIM_OK;
}

// compiled-model files (soarm_sim.h): the desc and hull arrays as sim_model_create takes them
static const char kModelMagic[8] = {'S', 'O', 'A', 'R', 'M', 'M', 'D', 'L'};
static const uint32_t kModelVersion = 2;  // 2: desc carries (struct_size, abi_version)

int sim_model_save(const sim_model_desc* desc, const float* hull_vert, const int32_t* hull_adr,
                   const int32_t* hull_adj, const char* path) {
  if (!desc || !path) return fail(SIM_E_ARG, "null argument");
  if (int rc = check_struct(desc, "sim_model_desc")) return rc;
  if (desc->nhullvert < 0 || desc->nhulladj < 0) return fail(SIM_E_ARG, "bad hull sizes");
  if (desc->nhullvert > 0 && (!hull_vert || !hull_adr || !hull_adj)) return fail(SIM_E_ARG, "hull arrays missing");
  FILE* f = fopen(path, "wb");
  if (!f) return fail(SIM_E_ARG, "cannot open model file for writing");
  const uint32_t hdr[2] = {kModelVersion, (uint32_t)sizeof(sim_model_desc)};
  bool ok = fwrite(kModelMagic, 1, 8, f) == 8 && fwrite(hdr, sizeof(uint32_t), 2, f) == 2 &&
            fwrite(desc, sizeof(sim_model_desc), 1, f) == 1;
  if (ok && desc->nhullvert > 0)
    ok = fwrite(hull_vert, sizeof(float), 3 * (size_t)desc->nhullvert, f) == 3 * (size_t)desc->nhullvert &&
         fwrite(hull_adr, sizeof(int32_t), (size_t)desc->nhullvert + 1, f) == (size_t)desc->nhullvert + 1 &&
         fwrite(hull_adj, sizeof(int32_t), (size_t)desc->nhulladj, f) == (size_t)desc->nhulladj;
  ok = (fclose(f) == 0) && ok;
  return ok ? SIM_OK : fail(SIM_E_ARG, "model file write failed");
}

int sim_model_load(const char* path, sim_model** out) {
  if (!path || !out) return fail(SIM_E_ARG, "null argument");
  *out = nullptr;
  FILE* f = fopen(path, "rb");
  if (!f) return fail(SIM_E_ARG, "cannot open model file");
  char magic[8];
  uint32_t hdr[2];
  sim_model_desc d;
  if (fread(magic, 1, 8, f) != 8 || memcmp(magic, kModelMagic, 8) != 0 || fread(hdr, sizeof(uint32_t), 2, f) != 2) {
    fclose(f);
    return fail(SIM_E_ARG, "not a compiled SO-ARM101 model file");
  }
  if (hdr[0] != kModelVersion || hdr[1] != sizeof(sim_model_desc)) {
    fclose(f);
    return fail(SIM_E_ARG, "model file version / layout does not match this library");
  }
  if (fread(&d, sizeof(d), 1, f) != 1 || d.nhullvert < 0 || d.nhulladj < 0 || d.nhullvert > (1 << 24) ||
      d.nhulladj > (1 << 26)) {
    fclose(f);
    return fail(SIM_E_ARG, "model file truncated or corrupt");
  }
  std::vector<float> hv(3 * (size_t)d.nhullvert);
  std::vector<int32_t> ha(d.nhullvert > 0 ? (size_t)d.nhullvert + 1 : 0), hj((size_t)d.nhulladj);
  bool ok = true;
  if (d.nhullvert > 0)
    ok = fread(hv.data(), sizeof(float), hv.size(), f) == hv.size() &&
         fread(ha.data(), sizeof(int32_t), ha.size(), f) == ha.size() &&
         fread(hj.data(), sizeof(int32_t), hj.size(), f) == hj.size();
  char extra;
  ok = ok && fread(&extra, 1, 1, f) == 0;  // nothing after the arrays
  fclose(f);
  if (!ok) return fail(SIM_E_ARG, "model file truncated or corrupt");
  return sim_model_create(&d, d.nhullvert ? hv.data() : nullptr, d.nhullvert ? ha.data() : nullptr,
                          d.nhullvert ? hj.data() : nullptr, out);
}

void sim_model_free(sim_model* m) { delete m; }

}  // extern "C"
