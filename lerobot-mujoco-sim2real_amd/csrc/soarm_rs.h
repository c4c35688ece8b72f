// soarm_rs.h -- the row-space PGS of the RS kernel (k_substep<..., RS = true>: 16 lanes per env,
// 4 envs per wave): the row layout (RsLayout), one sweep (rs_sweep) and the solve (rs_solve), which
// also makes its own warm start.  Included by soarm_pgs.h; solve_constraints calls rs_solve when the
// wave's vote (rs_fast, soarm_pgs.h) says every env's rows fit a layout.
// Reads: the contact records of RowLds (J rows, aref, mu, R), the frictionloss rows' aref / R (fa, fR),
// M^-1 (MInv), S.qacc_s, S.warm, the per-category contact counts of the vote.  Writes: v (qacc on
// return) and the W rows in RowLds::rsw; no force goes back to the records (the RS kernel's Euler step
// needs qacc alone).
#pragma once

namespace soarm {

// ---- Row-space PGS (the RS kernel: k_substep<..., RS>, 16 lanes per env, 4 envs per wave).
// MuJoCo's mj_solPGS sweeps the dual on the dense matrix AR = J M^-1 J' + R (efc_AR): row i's
// residual is AR_i f + b_i, its force steps by -res / AR_ii and is projected (frictionloss
// rows into [-fl, fl], limit rows and pyramid edges to f >= 0), rows in order.  The RS kernel
// holds that system directly: lane r of an env's 16-lane DPP row owns constraint rows r
// (slot A) and 16 + r (slot B) -- every frictionloss, limit and pyramid-edge row, from the
// first sweep to the last -- with the row's scaled residual s_r = -res_r / AR_rr and its row of
// the scaled matrix C[r][q] = -AR_rq / AR_rr (C[r][r] = -1) in registers.  Step q of a sweep:
// the projected step d = clamp(s_q, lo_q - f_q, hi_q - f_q) is formed from lane q's residual by
// a DPP row broadcast fused into the max (v_max_f32_dpp row_newbcast), every lane moves its
// residuals by C[r][q] d (one packed FMA per slot), and the step's bound registers (-f_q,
// kept broadcast in every lane of the env) take it: two dependent instructions per row.
// The improvement of mj_solPGS's stopping test is the sweep's exact cost change: with
// res = AR f + b, cost(f0) - cost(f1) = sum_r AR_rr / 2 (f1 - f0)_r (s0 + s1)_r, and each
// row's force change over the sweep is its own step, which a second accumulator beside s takes
// exactly (its coefficient is 1 at the row's own step, 0 elsewhere).
#ifndef SOARM_RS_SEQ
#define SOARM_RS_SEQ 0  // 1: the decoupled layouts' steps one at a time (A/B of the paired sweep)
#endif
constexpr int RS_MAXROW = 32;               // rows of one env (2 slots x 16 lanes)
constexpr int RS_WROW = 12;                 // floats per row of W = M^-1 J' in LDS (NV <= 12)
constexpr int RS_WENV = RS_MAXROW * RS_WROW + 4;  // per env (+4: the 4 envs of a wave on distinct banks)
constexpr int RS_EPW = 4;                   // envs per wave (workgroup)
template <int Q>
DEVI float rowbcast(float x) {  // lane Q of each 16-lane row
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x150 + Q, 0xF, 0xF, true));
}
// sum over the 16-lane row, bit-identical in all 16 lanes (the stop test must agree)
// (the permutes fused into the adds, v_add_f32_dpp; every stage adds two values that are equal
// bit for bit within each pair of partners -- quad xor 1, quad xor 2, the 8-lane mirror, the
// 16-lane mirror -- and fp addition is commutative, so all 16 lanes end with the same bits)
DEVI float rowsum16(float x) {
  asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "+v"(x));
  asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "+v"(x));
  asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf" : "+v"(x));
  asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf" : "+v"(x));
  return x;
}
// max(lane Q's x, b): the row broadcast fused into the max (VOP2 DPP).  A DPP read of a VGPR needs
// 2 wait states after the VALU write of it, and the compiler's hazard recognizer does not look into
// inline asm: the caller states how many instructions (NOPS = 2 - that count) must be padded.
template <int Q, int NOPS = 2>
DEVI float max_bcast(float x, float b) {
  float r;
  if constexpr (NOPS >= 2)
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x), "v"(b), "i"(Q));
  else if constexpr (NOPS == 1)
    asm volatile("s_nop 0\n\tv_max_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x), "v"(b), "i"(Q));
  else
    asm volatile("v_max_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x), "v"(b), "i"(Q));
  return r;
}
DEVI float vmin(float a, float b) {  // v_min without the IEEE-mode canonicalising of fminf
  float r;
  asm("v_min_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// f(std::integral_constant<int, i>) for i = 0 .. N-1 (compile-time lane / register indices)
template <class F, int... Is>
DEVI void sfor_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
DEVI void sfor(F&& f) {
  sfor_impl(f, std::make_integer_sequence<int, N>{});
}
// Row layout of one wave's RS solve (compile time).  Steps in mj_solPGS order: the NA dof
// frictionloss rows (F), then the edges of up to KAT arm-only contacts (AT: arm on the table /
// floor, arm self-contacts), of up to 4 contacts on the free body alone (CT: the cube on the
// table), of up to KAC contacts between the arm and the free body (AC) -- the order the pair
// list produces (arm-only pairs precede the free body's, its world pairs precede its arm pairs).
// Rows touching arm dofs (F, AT, AC) live in slot B, the CT edges in slot A: M is block diagonal,
// so an F / AT step moves slot B alone and a CT step slot A alone (and slot B's AC rows when the
// wave has an AC contact); a step therefore costs one residual update where the systems decouple.
// Steps an env has no row for are zero rows (exact no-ops).
template <int NA, int KAT, int KAC>
struct RsLayout {
  static_assert(NA + 4 * (KAT + KAC) <= 16, "slot B holds the F, AT and AC rows");
  static constexpr int CT0 = NA + 4 * KAT, AC0 = CT0 + 16, NS = AC0 + 4 * KAC;
  static constexpr bool decoupled = KAC == 0;  // no AC rows: the slot-B (arm) and slot-A (cube) steps never meet
  static constexpr int slot(int q) { return (q >= CT0 && q < AC0) ? 0 : 1; }
  static constexpr int lane(int q) { return q < CT0 ? q : q < AC0 ? q - CT0 : q - 16; }
  static constexpr bool upd_a(int q) { return q >= CT0; }                 // CT, AC
  static constexpr bool upd_b(int q) { return q < CT0 || q >= AC0 || KAC > 0; }
  // instructions after step q's write of slot sl before step q+1 (see rs_sweep's order)
  static constexpr int after_write(int q, int sl) {
    return (sl == 0 ? upd_a(q) : upd_b(q)) ? ((upd_a(q) && upd_b(q)) ? 1 : 0) + 1 + (q < NA ? 1 : 0) : 2;
  }
};
// one sweep of the row-space PGS (see above): s = (residual, own-step accumulator) per slot,
// C = (C, G) pairs per step, NF = lo - f of every row, NH = hi - f of the NA frictionloss rows (the
// others have hi = +inf).  Instruction order is pinned (sched_barrier): a DPP op waits for every
// VALU op in flight, so a step is its broadcast-max, the residual update of the slot the NEXT step
// broadcasts from, then the other slot's update and the bound updates -- which are also the 2 wait
// states the next broadcast needs after that write (padded with s_nop where a step has fewer)
//
// Layouts without AC rows (KAC = 0: no arm-cube contact in the wave, ~99.6% of the headline's waves)
// are two systems that never meet: the F / AT steps read and move slot B alone, the CT steps slot A
// alone (M is block diagonal).  Their steps then run paired -- B step i beside A step i, two
// independent chains in one instruction stream, each hiding the other's latency and DPP drain --
// and each slot still takes its own steps in mj_solPGS order, so every residual, force and
// accumulator is bit-identical to the sequential sweep.
template <int NA, class LY>
DEVI void rs_sweep(f2& sA, f2& sB, const f2 (&CA)[LY::NS], const f2 (&CB)[LY::NS], float (&NF)[LY::NS],
                   float (&NH)[NA]) {
  if constexpr (LY::decoupled && !SOARM_RS_SEQ) {
    constexpr int NB = LY::CT0, NAS = LY::NS - LY::CT0;  // slot-B steps (F, AT), slot-A steps (CT)
    static_assert(NB <= NAS, "slot A has at least as many steps as slot B");
    sfor<NAS>([&](auto ic) {
      constexpr int I = decltype(ic)::value;
      constexpr bool HB = I < NB;
      constexpr int QA = LY::CT0 + I;
      // wait states before this step's broadcasts (2 needed after the VALU write of the source):
      // B reads sB, written by step I-1's first update, with the sA update and >= 2 bound updates
      // after it; A reads sA, written by step I-1's second update, with step I-1's bound updates
      // (2 when it had a B step, else 1) and this step's B broadcast after it
      constexpr int waitA = I == 0 ? 0 : ((I - 1) < NB ? 2 + (HB ? 1 : 0) : 1 + (HB ? 1 : 0));
      float dB = 0.f, dA;
      if constexpr (HB) dB = max_bcast<LY::lane(I), (I == 0 ? 2 : 0)>(sB.x, NF[I]);
      dA = max_bcast<LY::lane(QA), (waitA >= 2 ? 0 : 2 - waitA)>(sA.x, NF[QA]);
      if constexpr (HB && I < NA) dB = vmin(dB, NH[I]);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (HB) sB = __builtin_elementwise_fma(CB[I], f2{dB, dB}, sB);
      __builtin_amdgcn_sched_barrier(0);
      sA = __builtin_elementwise_fma(CA[QA], f2{dA, dA}, sA);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (HB) {
        NF[I] -= dB;
        if constexpr (I < NA) NH[I] -= dB;
      }
      NF[QA] -= dA;
      __builtin_amdgcn_sched_barrier(0);
    });
    return;
  }
  sfor<LY::NS>([&](auto qc) {
    constexpr int Q = decltype(qc)::value;
    constexpr int SL = LY::slot(Q), LN = LY::lane(Q);
    constexpr int after = Q == 0 ? 0 : LY::after_write(Q - 1, SL);
    float d = max_bcast<LN, (after >= 2 ? 0 : 2 - after)>(SL == 0 ? sA.x : sB.x, NF[Q]);
    if constexpr (Q < NA) d = vmin(d, NH[Q]);
    __builtin_amdgcn_sched_barrier(0);
    constexpr int NSL = Q + 1 < LY::NS ? LY::slot(Q + 1) : SL;  // the next step's source slot
    auto upd = [&](auto slc) {
      if constexpr (decltype(slc)::value == 0) {
        if constexpr (LY::upd_a(Q)) sA = __builtin_elementwise_fma(CA[Q], f2{d, d}, sA);
      } else {
        if constexpr (LY::upd_b(Q)) sB = __builtin_elementwise_fma(CB[Q], f2{d, d}, sB);
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    upd(std::integral_constant<int, NSL>{});
    upd(std::integral_constant<int, 1 - NSL>{});
    NF[Q] -= d;
    if constexpr (Q < NA) NH[Q] -= d;
    __builtin_amdgcn_sched_barrier(0);
  });
}

// ---- row-space PGS (RS kernel; see RS_MAXROW above).  Rows in mj_solPGS order: the NA dof
// frictionloss rows, the active limits, 4 pyramid edges per contact; NRB (compile time) bounds
// the rows of every env of the wave (rows past an env's own are zero rows: J = 0, so C's row and
// column are 0 and their steps are exact no-ops).  Lane r16 holds rows r16 (slot A) and 16 + r16
// (slot B, when NRB > 16).  v: the velocity after the warm start; on return, qacc.
template <int KAT, int KAC, int NA, int NF>
DEVI void rs_solve(Sim<NA, NF>& S, const RowLds& L, const MInv<NA, NF>& Mi, const float (&fa)[NA],
                   const float (&fR)[NA], float (&v)[NA + 6 * NF], int rs_nat, int rs_nct,
                   int rs_nac PROF_DECL(, int e, int& nsweep)) {
  constexpr int NV = NA + 6 * NF;
  const DModel& m = *S.mp;
  using LY = RsLayout<NA, KAT, KAC>;
  constexpr int NS = LY::NS;
    const int r16 = L.lane & 15;
    float* const Wl = L.rsw + L.col * RS_WENV;
    // this lane's rows: slot A = CT edge r16, slot B = frictionloss row / AT edge / AC edge r16;
    // kind 0 frictionloss, 1 pyramid edge, -1 none; c, ed: the edge's contact and edge index;
    // qA / qB: the rows' step indices (their W rows in LDS)
    const int cA = rs_nat + (r16 >> 2), qA = LY::CT0 + r16;
    const int kindA = (r16 >> 2) < rs_nct ? 1 : -1;
    int kindB = -1, cB = 0;
    if (r16 < NA) {
      kindB = 0;
    } else if (r16 < LY::CT0) {
      cB = (r16 - NA) >> 2, kindB = cB < rs_nat ? 1 : -1;
    } else if (r16 < LY::CT0 + 4 * KAC) {
      const int k = (r16 - LY::CT0) >> 2;
      cB = rs_nat + rs_nct + k, kindB = k < rs_nac ? 1 : -1;
    }
    const int qB = r16 < LY::CT0 ? r16 : r16 + 16;
    // row data: J (NV), aref, R, the warm-start force (the warm start above)
    auto row_of = [&](int kind, int c, int ed, float (&J)[NV], float& ar, float& R, float& f) {
#pragma unroll
      for (int i = 0; i < NV; i++) J[i] = 0.f;
      ar = 0.f, R = 1.f, f = 0.f;
      if (kind == 0) {  // dof frictionloss row ed: J = e_ed
#pragma unroll
        for (int i = 0; i < NA; i++)
          if (ed == i) {
            J[i] = 1.f, ar = fa[i], R = fR[i];
            // warm-start force (the Gram-form warm start's frictionloss branch)
            const float fl = m.dof_frictionloss[i], jar = S.warm[i] - fa[i];
            const float fs = (jar <= -fl * R) ? fl : (jar >= fl * R) ? -fl : -jar / R;
            f = fl > 0.f ? fs : 0.f;
          }
      } else if (kind == 1) {  // pyramid edge J_n +- mu J_t of contact c
        const float mu = L.at(c, F_MU), s = (ed & 1) ? -mu : mu;
        const int t = 12 * (1 + (ed >> 1));
#pragma unroll
        for (int i = 0; i < NV; i++) J[i] = fmaf(s, L.at(c, t + i), L.at(c, i));
        ar = L.at(c, F_AREF + ed), R = L.at(c, F_R);
        float jar = -ar;  // warm-start force: the edge's J qacc_warmstart - aref, if negative
#pragma unroll
        for (int i = 0; i < NV; i++) jar = fmaf(J[i], S.warm[i], jar);
        f = jar < 0.f ? -jar / R : 0.f;
      }
    };
    float JA[NV], JB[NV], WA[NV], WB[NV], arA, arB, RA, RB, fA, fB;
    row_of(kindA, cA, r16 & 3, JA, arA, RA, fA);
    row_of(kindB, cB, kindB == 0 ? r16 : (r16 - NA) & 3, JB, arB, RB, fB);
    Mi.mul(JA, WA, false, true);  // (CT rows touch the free body alone)
    Mi.mul(JB, WB, true, KAC > 0);
    // W rows to LDS, by step (the 4 copies of a quad write identical values)
#pragma unroll
    for (int i = 0; i < NV; i++) Wl[qA * RS_WROW + i] = WA[i];
    if (qB < NS)
#pragma unroll
      for (int i = 0; i < NV; i++) Wl[qB * RS_WROW + i] = WB[i];
    // AR_rr = J_r W_r + R_r
    float ardA = RA, ardB = RB;
#pragma unroll
    for (int i = 0; i < NV; i++) ardA = fmaf(JA[i], WA[i], ardA), ardB = fmaf(JB[i], WB[i], ardB);
    const float iA = 1.f / ardA, iB = 1.f / ardB;
    const float hdA = 0.5f * ardA, hdB = 0.5f * ardB;
    wave_sync();
    // the bound registers, broadcast over the env's row: -f_q (edges) and the frictionloss
    // rows' lo - f, hi - f
    float NF_[NS], NH_[NA];
    auto bounds = [&]() {
      sfor<NS>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const float fq = -rowbcast<LY::lane(q)>(LY::slot(q) == 0 ? fA : fB);
        if constexpr (q < NA) {
          const float fl = m.dof_frictionloss[q];
          NF_[q] = fq - fl, NH_[q] = fq + fl;
        } else {
          NF_[q] = fq;
        }
      });
    };
    // v = qacc_smooth + sum_q W_q f_q (lane i < NV sums dof i, the row broadcasts it); f_q from the
    // bound registers (NH_ = fl - f on the frictionloss rows, NF_ = -f on the others)
    auto vel = [&]() {
      float acc = 0.f;
      const int di = r16 < NV ? r16 : 0;
#pragma unroll
      for (int q = 0; q < NS; q++)
        acc = fmaf(Wl[q * RS_WROW + di], q < NA ? m.dof_frictionloss[q] - NH_[q] : -NF_[q], acc);
      sfor<NV>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        v[i] = S.qacc_s[i] + rowbcast<i>(acc);
      });
    };
    // the warm start in row space (the Gram-form block above is skipped on these waves): every
    // row's warm force (row_of), v, and the dual cost against f = 0, summed over the env's rows
    bounds();
    vel();
    float jvA = -arA, jvB = -arB, jqA = -arA, jqB = -arB;
#pragma unroll
    for (int i = 0; i < NV; i++) {
      jvA = fmaf(JA[i], v[i], jvA), jvB = fmaf(JB[i], v[i], jvB);
      jqA = fmaf(JA[i], S.qacc_s[i], jqA), jqB = fmaf(JB[i], S.qacc_s[i], jqB);
    }
    // dual cost: sum_r 0.5 f_r (J_r v - aref_r + R_r f_r) + 0.5 f_r (J_r qacc_smooth - aref_r)
    const float wcost = rowsum16(0.5f * fA * (jvA + RA * fA) + 0.5f * fA * jqA +
                                 (0.5f * fB * (jvB + RB * fB) + 0.5f * fB * jqB));
    const bool rej = wcost > 0.f;  // worse than no warm start: f = 0, v = qacc_smooth
    if (__any(rej)) {              // (wave-uniform: the broadcasts run on every row)
      fA = rej ? 0.f : fA, fB = rej ? 0.f : fB;
      bounds();
#pragma unroll
      for (int i = 0; i < NV; i++) v[i] = rej ? S.qacc_s[i] : v[i];
      jvA = rej ? jqA : jvA, jvB = rej ? jqB : jvB;
    }
    f2 sA = f2{-fmaf(RA, fA, jvA) * iA, 0.f}, sB = f2{-fmaf(RB, fB, jvB) * iB, 0.f};
    // the scaled matrix: C[r][q] = -J_r W_q / AR_rr, C[r][r] = -1, as (C, G) pairs: G is the row's
    // own-step indicator, so the second accumulator takes the row's force step exactly (the stop
    // test's Delta f_r; it was u_r - Delta s_r from an off-diagonal accumulator, whose fp32
    // cancellation stopped an ill-conditioned env 22 sweeps early, 3.3e-3 m/s off -- r05); only
    // the blocks a step updates
    f2 CA[NS], CB[NS];
    sfor<NS>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      constexpr bool UA = LY::upd_a(q), UB = LY::upd_b(q);
      f2 a = f2{0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NV; i++)
        a = fma2(f2{UA ? JA[i] : 0.f, UB ? JB[i] : 0.f}, splat2(Wl[q * RS_WROW + i]), a);
      const float ca = -a.x * iA, cb = -a.y * iB;
      CA[q] = qA == q ? f2{-1.f, 1.f} : f2{ca, 0.f};
      CB[q] = qB == q ? f2{-1.f, 1.f} : f2{cb, 0.f};
      // (the W rows of two steps in flight at a time: hoisting every step's 12 LDS loads to
      // the top would hold hundreds of values)
      if constexpr (q & 1) __builtin_amdgcn_sched_barrier(0);
    });
    float scale = m.pgs_scale, tol = m.tolerance;
    int iters = m.iterations;
    // (loaded once: the sweeps' asm statements keep LICM from hoisting the model loads, which would
    // otherwise be re-issued and waited for in every sweep)
    asm volatile("" : "+s"(iters), "+s"(scale), "+s"(tol));
    PHASE_T(rp0);  // (the RS solve's split: prof_rs_split)
    // The sweep loop.  An env's lanes leave it at the sweep whose improvement passes the stop test
    // (they drop out of the active mask once, there), and the loop ends when no env is left or at the
    // cap: the count is wave-uniform and stays on the scalar unit, so the back edge is the verdict's
    // compare, the mask update and one branch.  (It was `if (!done) {...} if (__all(done)) break`: the
    // mask re-derived from `done` every sweep, a per-lane count, two taken branches -- 712 against
    // 647 cycles per sweep iteration in tools/mb_rs_tail.hip)
    int it = 0;
    PROF_DECL(int pis = 0);  // (profiling build: the env's sweeps, counted per lane beside the scalar count)
    if (iters > 0) do {
      const float s0A = sA.x, s0B = sB.x;
      sA.y = 0.f, sB.y = 0.f;
      rs_sweep<NA, LY>(sA, sB, CA, CB, NF_, NH_);
      // improvement = sum_r AR_rr / 2 Delta f_r (s0 + s1)_r, Delta f_r = the row's own step (y)
      float P = hdA * sA.y * (s0A + sA.x);
      P = fmaf(hdB * sB.y, s0B + sB.x, P);
      it++;
      asm volatile("" : "+s"(it));
      PROF_DO(pis++);
      if (rowsum16(P) * scale < tol) break;  // (per env: all 16 lanes hold the same bits)
    } while (it < iters);
    PROF_DO(nsweep = pis);
    PROF_DECL(const int wsw = wave_max_i(pis));  // the wave's sweeps: its slowest env's
    PHASE_T(rp1);
    // qacc = qacc_smooth + sum_q W_q f_q (NH_ = fl - f on the frictionloss rows, NF_ = -f on the
    // others): lane i < NV sums dof i, then the row broadcasts it
    vel();
    PROF_DO(prof_rs_split(e, rp0, rp1, wsw));
}

}  // namespace soarm
