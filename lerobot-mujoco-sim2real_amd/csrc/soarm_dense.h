// soarm_dense.h — the dense statement of MuJoCo's constraint problem (mj_makeConstraint's rows in
// MuJoCo's order: dof frictionloss, joint limits lower/upper, 4 pyramid edges per contact), once,
// for the two units that solve it densely: the CPU backend (soarm_cpu.hip) and the contact-force
// readout's kernel (soarm_cforce.hip).  What a row is (its constants, its force and cost as
// functions of J a - aref, the PGS warm start and projection), the contact frame and Jacobian, M's
// packed blocks, the packed Cholesky solve and the pyramid decode live here; how the rows are
// enumerated and swept stays with each unit (a serial walk there, 16 lanes per env here).
//
// Every function is HDI, holds no state, no LDS and no lane operation.  The step's kernels
// (soarm_pgs.h / soarm_newton.h / soarm_rs.h) state the same rows in their lane-cooperative form
// and do not include this header.
#pragma once
#include "soarm_step.h"

namespace soarm {

enum { ROW_NONE = 0, ROW_FRICTION = 1, ROW_LIMIT = 2, ROW_CONTACT = 3 };

// a row's constants: reference acceleration, regulariser, frictionloss (0 but for ROW_FRICTION)
struct RowConst {
  float aref, R, fl;
};

// ------------------------------------------------------------------ M (Sim's packed blocks)
// index of (i, k) in a packed lower triangle, either order
HDI constexpr int tri(int i, int k) { return i >= k ? i * (i + 1) / 2 + k : k * (k + 1) / 2 + i; }

// y = M x with the block-diagonal packed M of Sim (arm NA x NA | one 6x6 per free body)
template <int NA, int NF>
HDI void mul_m(const Sim<NA, NF>& S, const float* x, float* y) {
#pragma unroll
  for (int i = 0; i < NA; i++) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NA; k++) s += S.MA[tri(i, k)] * x[k];
    y[i] = s;
  }
#pragma unroll
  for (int f = 0; f < NF; f++) {
    const int d0 = NA + 6 * f;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 6; k++) s += S.MF[f][tri(i, k)] * x[d0 + k];
      y[d0 + i] = s;
    }
  }
}
// element (i, k) of M, i >= k
template <int NA, int NF>
HDI float m_at(const Sim<NA, NF>& S, int i, int k) {
  if (i < NA) return S.MA[tri(i, k)];
  const int f = (i - NA) / 6, d0 = NA + 6 * f;
  return k >= d0 ? S.MF[f][tri(i - d0, k - d0)] : 0.f;
}

// dense Cholesky solve of the SPD H, packed lower triangle; false on a non-positive pivot (x is
// then unusable: no early exit, so the device code stays straight-line)
template <int N>
HDI bool chol_solve(const float (&A)[N * (N + 1) / 2], float (&x)[N], const float (&b)[N]) {
  float L[N * (N + 1) / 2];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) {
      float s = A[tri(i, j)];
#pragma unroll
      for (int k = 0; k < j; k++) s -= L[tri(i, k)] * L[tri(j, k)];
      if (i == j) {
        ok = ok && s > 0.f;
        L[tri(i, i)] = sqrtf(s);
      } else {
        L[tri(i, j)] = s / L[tri(j, j)];
      }
    }
  float y[N];
#pragma unroll
  for (int i = 0; i < N; i++) {
    float s = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= L[tri(i, k)] * y[k];
    y[i] = s / L[tri(i, i)];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    float s = y[i];
#pragma unroll
    for (int k = i + 1; k < N; k++) s -= L[tri(k, i)] * x[k];
    x[i] = s / L[tri(i, i)];
  }
  return ok;
}

// ------------------------------------------------------------------ contact geometry
// contact frame (mju_makeFrame): rows normal, tangent 1, tangent 2
HDI void contact_frame(const float nrm[3], float fr[9]) {
  fr[0] = nrm[0], fr[1] = nrm[1], fr[2] = nrm[2];
  float y[3];
  if (fabsf(fr[1]) < 0.5f)
    y[0] = 0, y[1] = 1, y[2] = 0;
  else
    y[0] = 0, y[1] = 0, y[2] = 1;
  const float dd = dot3(fr, y);
  y[0] -= dd * fr[0], y[1] -= dd * fr[1], y[2] -= dd * fr[2];
  const float inv = 1.f / sqrtf(dot3(y, y));
  fr[3] = y[0] * inv, fr[4] = y[1] * inv, fr[5] = y[2] * inv;
  cross(fr + 6, fr, fr + 3);
}

// relative translational Jacobian (body2 - body1) at the contact point cpos, in the contact frame fr
template <int NA, int NF>
HDI void contact_jac(const Sim<NA, NF>& S, int b1, int b2, const float cpos[3], const float fr[9],
                     float (&jd)[3][NA + 6 * NF]) {
#pragma unroll
  for (int q = 0; q < 3; q++)
#pragma unroll
    for (int i = 0; i < NA + 6 * NF; i++) jd[q][i] = 0.f;
#pragma unroll
  for (int side = 0; side < 2; side++) {
    const int b = side ? b2 : b1;
    const float sg = side ? 1.f : -1.f;
#pragma unroll
    for (int i = 0; i < NA; i++)
      if (b >= i + 2 && b < 2 + NA) {  // hinge i moves chain bodies i+2.. (reference point: origin)
        float l[3];
        cross(l, S.cdof[i], cpos);
        const float jp[3] = {S.cdof[i][3] + l[0], S.cdof[i][4] + l[1], S.cdof[i][5] + l[2]};
#pragma unroll
        for (int q = 0; q < 3; q++) jd[q][i] += sg * dot3(fr + 3 * q, jp);
      }
#pragma unroll
    for (int f = 0; f < NF; f++) {
      const int fb = 2 + NA + f, d0 = NA + 6 * f;
      if (b != fb) continue;
      const float off[3] = {cpos[0] - S.xpos[fb][0], cpos[1] - S.xpos[fb][1], cpos[2] - S.xpos[fb][2]};
#pragma unroll
      for (int i = 0; i < 6; i++) {
        float l[3];
        cross(l, S.cdof[d0 + i], off);
        const float jp[3] = {S.cdof[d0 + i][3] + l[0], S.cdof[d0 + i][4] + l[1], S.cdof[d0 + i][5] + l[2]};
#pragma unroll
        for (int q = 0; q < 3; q++) jd[q][d0 + i] += sg * dot3(fr + 3 * q, jp);
      }
    }
  }
}

// ------------------------------------------------------------------ row constants (mj_makeConstraint)
// from the same model constants as the step's kernels: dof_fricR/B, jnt_KB, pair_KB / tran / solimp / margin
// frictionloss row of dof i (J = e_i)
HDI RowConst friction_row(const DModel& m, int i, float qvel) {
  return {-m.dof_fricB[i] * qvel, m.dof_fricR[i], m.dof_frictionloss[i]};
}
// limit row of joint i (J = sg e_i, sg = +1 lower / -1 upper), active while dist < jnt_margin
HDI RowConst limit_row(const DModel& m, int i, int side, float dist, float qvel) {
  const float sg = side == 0 ? 1.f : -1.f;
  const float imp = impedance(m.jnt_solimp[i], dist, m.jnt_margin[i]);
  return {-m.jnt_KB[i][1] * (sg * qvel) - m.jnt_KB[i][0] * imp * (dist - m.jnt_margin[i]),
          fmaxf(MINVALF, (1.f - imp) * m.dof_invweight0[i] / imp), 0.f};
}
// a contact of pair p: its impedance, the normal's regulariser R0 and the pyramid edges' Rpy
HDI void contact_consts(const DModel& m, int p, float mu, float cdist, float& imp, float& R0, float& Rpy) {
  imp = impedance(m.pair_solimp[p], cdist, m.pair_margin[p]);
  const float tran = m.pair_tran[p];
  R0 = fmaxf(MINVALF, (1.f - imp) * (tran + mu * mu * tran) / imp);
  Rpy = 2.f * mu * mu * R0 / m.impratio;
}
// pyramid edge ed of a contact (condim 3): J = jd[normal] +- mu jd[tangent 1 + ed / 2]; returns aref
template <int NV>
HDI float edge_row(const DModel& m, const float (&jd)[3][NV], int ed, float mu, const float* qvel, int p, float imp,
                   float cdist, float* J) {
  const float s = (ed & 1) ? -mu : mu;
  float vel = 0.f;
#pragma unroll
  for (int i = 0; i < NV; i++) {
    J[i] = jd[0][i] + s * ((ed >> 1) ? jd[2][i] : jd[1][i]);
    vel += J[i] * qvel[i];
  }
  return -m.pair_KB[p][1] * vel - m.pair_KB[p][0] * imp * (cdist - m.pair_margin[p]);
}

// ------------------------------------------------------------------ a row as a function of x = J a - aref
// force -s'(x) and whether the row is in its quadratic zone; its cost s(x)
HDI float row_force(int type, float R, float fl, float x, bool& quad) {
  if (type == ROW_FRICTION) {
    quad = x > -R * fl && x < R * fl;
    return x <= -R * fl ? fl : x >= R * fl ? -fl : -x / R;
  }
  quad = x < 0.f;
  return quad ? -x / R : 0.f;
}
HDI float row_cost(int type, float R, float fl, float x) {
  if (type == ROW_FRICTION) {
    if (x <= -R * fl) return -fl * x - 0.5f * R * fl * fl;
    if (x >= R * fl) return fl * x - 0.5f * R * fl * fl;
    return 0.5f * x * x / R;
  }
  return x < 0.f ? 0.5f * x * x / R : 0.f;
}
// PGS's warm start: the force implied by jar = J qacc_warmstart - aref (an absent row: 0)
HDI float warm_force(int type, float R, float fl, float jar) {
  if (type == ROW_FRICTION) return jar <= -fl * R ? fl : jar >= fl * R ? -fl : -jar / R;
  return type != ROW_NONE && jar < 0.f ? -jar / R : 0.f;
}
// PGS's projection of a row's updated force onto its bounds
HDI float pgs_project(int type, float fl, float fn) {
  return type == ROW_FRICTION ? fminf(fmaxf(fn, -fl), fl) : fmaxf(fn, 0.f);
}

// mju_decodePyramid of a condim-3 contact's 4 edge forces g: fo = normal, tangent 1, tangent 2 in
// the contact frame fr, then the same force as a world vector
HDI void decode_pyramid(const float g[4], float mu, const float fr[9], float fo[6]) {
  fo[0] = (g[0] + g[1]) + (g[2] + g[3]);
  fo[1] = mu * (g[0] - g[1]);
  fo[2] = mu * (g[2] - g[3]);
#pragma unroll
  for (int q = 0; q < 3; q++) fo[3 + q] = fo[0] * fr[q] + fo[1] * fr[3 + q] + fo[2] * fr[6 + q];
}

}  // namespace soarm
