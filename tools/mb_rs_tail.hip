// Diagnostic microbenchmark: cycles per whole sweep iteration of the RS solve's (0,0) layout
// (soarm_rs.h: 6 paired + 10 slot-A-only steps) under the loop forms of rs_solve, one wave per
// SIMD (1024 blocks of 64 lanes, as the RS kernel at 4096 envs).  The loop forms are written as
// rs_solve writes (or wrote) them, so the compiler builds the same control around the same steps;
// check the loops in the ISA (tools/isa_loops.py) against the kernel's before trusting a row.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -o tools/_mb/mb_rs_tail tools/mb_rs_tail.hip
// Variants: 0 the steps alone (counted loop, no stop test); 1 the loop before the scalar loop
// control (`if (!done) {...} if (__all(done)) break`, the test's 16-lane sum after the steps);
// 2 rs_solve's loop (an env's lanes leave at their verdict; scalar count); 3 the stop test pipelined
// one sweep deep (the sum's DPP stages and the verdict inside the next sweep, two register sets so
// that the speculative sweep is harmless) -- tried in the kernel, exact, and not kept: slower here
// and in the bench ("Stop test"); 4 as 3 with ds_swizzle_b32 + v_add stages
// (xor 1, 2, 7, 15: the same partners).  The tolerance is negative, so no env ever stops and every
// variant runs R sweeps.  MI355X, 1024 waves, cycles per sweep iteration: 495 / 712 / 647 / 851 / 918.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <utility>
typedef float f2 __attribute__((ext_vector_type(2)));
#define DEVI __device__ __forceinline__
#define R 200
constexpr int NA = 6, NB = 6, NAS = 16, NS = 22;
template <int Q, int NOPS>
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
DEVI float vmin(float a, float b) {
  float r;
  asm("v_min_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
DEVI void vpin(float& x) { asm volatile("" : "+v"(x)); }
DEVI void vpin(f2& x) { asm volatile("" : "+v"(x)); }
DEVI float rowsum16(float x) {
  asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "+v"(x));
  asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "+v"(x));
  asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf" : "+v"(x));
  asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf" : "+v"(x));
  return x;
}
template <int ST>
DEVI void stage_dpp(float& x) {
  if constexpr (ST == 0)
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "+v"(x));
  else if constexpr (ST == 1)
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "+v"(x));
  else if constexpr (ST == 2)
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf" : "+v"(x));
  else
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf" : "+v"(x));
}
template <int ST>
DEVI float swz(float x) {  // ds_swizzle_b32, bit mode: and 0x1f, xor 1 / 2 / 7 / 15
  constexpr int pat = 0x1f | ((ST == 0 ? 1 : ST == 1 ? 2 : ST == 2 ? 7 : 15) << 10);
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(x), pat));
}
template <class F, int... Is>
DEVI void sfor_impl(F&& f, std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }
template <int N, class F>
DEVI void sfor(F&& f) { sfor_impl(f, std::make_integer_sequence<int, N>{}); }

// the paired sweep from set 0 into set 1 (the same set when they alias: the in-place sweep);
// RED: 0 none, 1 DPP stages of `pend`, 2 swizzle stages; returns the verdict
template <int RED, bool INPLACE>
DEVI bool sweep(const f2& sA0, const f2& sB0, f2& sA1, f2& sB1, const f2 (&CA)[NS], const f2 (&CB)[NS],
                const float (&NF0)[NS], float (&NF1)[NS], const float (&NH0)[NA], float (&NH1)[NA], float hdA,
                float hdB, float scale, float tol, float& pend) {
  bool verdict = false;
  float pB1 = 0.f, pB2 = 0.f, sw = 0.f;
  sfor<NAS>([&](auto ic) __attribute__((always_inline)) {
    constexpr int I = decltype(ic)::value;
    constexpr bool HB = I < NB;
    constexpr int QA = NB + I;
    constexpr int waitA = I == 0 ? 0 : ((I - 1) < NB ? 2 + (HB ? 1 : 0) : 1 + (HB ? 1 : 0));
    const f2 srcA = I == 0 ? f2{sA0.x, 0.f} : sA1, srcB = I == 0 ? f2{sB0.x, 0.f} : sB1;
    float dB = 0.f, dA;
    if constexpr (HB) dB = max_bcast<I, (I == 0 ? 2 : 0)>(srcB.x, NF0[I]);
    dA = max_bcast<I, (waitA >= 2 ? 0 : 2 - waitA)>(srcA.x, NF0[QA]);
    if constexpr (HB && I < NA) dB = vmin(dB, NH0[I]);
    if constexpr (RED == 1 && I >= NB && I < NB + 8 && (I - NB) % 2 == 0) stage_dpp<(I - NB) / 2>(pend);
    if constexpr (RED == 2 && I >= NB && I < NB + 8) {
      if constexpr ((I - NB) % 2 == 0)
        sw = swz<(I - NB) / 2>(pend);
      else
        pend += sw;
    }
    if constexpr (RED != 0 && I == NB + 8) {
      float t = pend * scale;
      asm volatile("" : "+v"(t));
      verdict = t < tol;
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (HB) sB1 = __builtin_elementwise_fma(CB[I], f2{dB, dB}, srcB);
    __builtin_amdgcn_sched_barrier(0);
    sA1 = __builtin_elementwise_fma(CA[QA], f2{dA, dA}, srcA);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (HB) {
      NF1[I] = NF0[I] - dB;
      if constexpr (I < NA) NH1[I] = NH0[I] - dB;
    }
    NF1[QA] = NF0[QA] - dA;
    if constexpr (!INPLACE && I == NB) {
      pB1 = hdB * sB1.y, pB2 = sB0.x + sB1.x;
      asm volatile("" : "+v"(pB1), "+v"(pB2));
    }
    __builtin_amdgcn_sched_barrier(0);
  });
  if constexpr (!INPLACE) {
    vpin(sA1), vpin(sB1);
    sfor<NS>([&](auto qc) __attribute__((always_inline)) { vpin(NF1[decltype(qc)::value]); });
    sfor<NA>([&](auto qc) __attribute__((always_inline)) { vpin(NH1[decltype(qc)::value]); });
    pend = fmaf(pB1, pB2, hdA * sA1.y * (sA0.x + sA1.x));
    vpin(pend);
  }
  return verdict;
}

template <int K>
__global__ __launch_bounds__(64) void k(float* out, long long* cyc, float a, int iters_, float scale_, float tol_) {
  const float l = (threadIdx.x & 15) * 1e-3f + 1e-3f;
  f2 CA[NS], CB[NS];
  float NF[NS], NH[NA], NF1[NS], NH1[NA];
#pragma unroll
  for (int q = 0; q < NS; q++) CA[q] = f2{-l * 0.01f * q, 0.f}, CB[q] = f2{l * 0.01f * q, 0.f}, NF[q] = -a * (q + 1), NF1[q] = 0.f;
#pragma unroll
  for (int q = 0; q < NA; q++) NH[q] = a * (q + 1), NH1[q] = 0.f;
  f2 sA = {l, 0}, sB = {-l, 0}, sA1 = sA, sB1 = sB;
  const float hdA = 0.5f + l, hdB = 0.25f + l;
  int iters = iters_;
  float scale = scale_, tol = tol_;
  asm volatile("" : "+s"(iters), "+s"(scale), "+s"(tol));
  float pend = 0.f;
  bool in1 = false;
  const long long t0 = clock64();
  if constexpr (K == 0) {
    for (int it = 0; it < iters; it++) sweep<0, true>(sA, sB, sA, sB, CA, CB, NF, NF, NH, NH, hdA, hdB, scale, tol, pend);
  } else if constexpr (K == 1) {
    bool done = false;
    for (int it = 0; it < iters; it++) {
      if (!done) {
        const float s0A = sA.x, s0B = sB.x;
        sweep<0, true>(sA, sB, sA, sB, CA, CB, NF, NF, NH, NH, hdA, hdB, scale, tol, pend);
        float P = hdA * sA.y * (s0A + sA.x);
        P = fmaf(hdB * sB.y, s0B + sB.x, P);
        done = rowsum16(P) * scale < tol;
      }
      if (__all(done)) break;
    }
  } else if constexpr (K == 2) {
    int it = 0;
    if (iters > 0) do {
      const float s0A = sA.x, s0B = sB.x;
      sweep<0, true>(sA, sB, sA, sB, CA, CB, NF, NF, NH, NH, hdA, hdB, scale, tol, pend);
      float P = hdA * sA.y * (s0A + sA.x);
      P = fmaf(hdB * sB.y, s0B + sB.x, P);
      it++;
      asm volatile("" : "+s"(it));
      if (rowsum16(P) * scale < tol) break;
    } while (it < iters);
  } else {
    constexpr int RED = K == 3 ? 1 : 2;
    if (iters > 0) {
      int it = 1;
      sweep<0, false>(sA, sB, sA1, sB1, CA, CB, NF, NF1, NH, NH1, hdA, hdB, scale, tol, pend);
      in1 = true;
      for (;;) {
        asm volatile("" : "+s"(it));
        if (it >= iters) break;
        if (sweep<RED, false>(sA1, sB1, sA, sB, CA, CB, NF1, NF, NH1, NH, hdA, hdB, scale, tol, pend)) break;
        it++, in1 = false;
        asm volatile("" : "+s"(it));
        if (it >= iters) break;
        if (sweep<RED, false>(sA, sB, sA1, sB1, CA, CB, NF, NF1, NH, NH1, hdA, hdB, scale, tol, pend)) break;
        it++, in1 = true;
      }
    }
  }
  const long long t1 = clock64();
  float acc = in1 ? sA1.x + sB1.x : sA.x + sB.x;
#pragma unroll
  for (int q = 0; q < NS; q++) {
    const float f0 = NF[q], f1 = NF1[q];
    acc += in1 ? f1 : f0;
  }
#pragma unroll
  for (int q = 0; q < NA; q++) {
    const float h0 = NH[q], h1 = NH1[q];
    acc += in1 ? h1 : h0;
  }
  out[blockIdx.x * 64 + threadIdx.x] = acc + pend;
  if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}

template <int K>
void run(const char* name, int nblk) {
  float* o;
  long long* c;
  hipMalloc(&o, nblk * 64 * 4);
  hipMalloc(&c, nblk * 8);
  for (int rep = 0; rep < 2; rep++) hipLaunchKernelGGL(k<K>, dim3(nblk), dim3(64), 0, 0, o, c, 0.5f, R, 1.f, -1.f);
  hipDeviceSynchronize();
  long long* h = new long long[nblk];
  hipMemcpy(h, c, nblk * 8, hipMemcpyDeviceToHost);
  double s = 0, mx = 0;
  for (int i = 0; i < nblk; i++) s += h[i], mx = h[i] > mx ? h[i] : mx;
  printf("%-52s waves %5d  cycles/sweep mean %7.1f max %7.1f\n", name, nblk, s / nblk / R, mx / R);
  hipFree(o), hipFree(c);
  delete[] h;
}
int main() {
  for (int nb : {1, 1024}) {
    run<0>("0 steps alone (6 paired + 10 single)", nb);
    run<1>("1 loop before: if(!done) + __all, sum after steps", nb);
    run<2>("2 rs_solve's loop: lanes leave, scalar count", nb);
    run<3>("3 pipelined, DPP stages in the next sweep", nb);
    run<4>("4 pipelined, ds_swizzle + v_add stages", nb);
  }
  return 0;
}
