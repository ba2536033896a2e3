// What stands around an optimiser rule (optim_rules.h) in a kernel, ONE copy for the flat streaming kernels (optim.hip) and the
// layer-wise trust kernels (trust.hip): the gate, the element body (loads, the regulariser's w^2, the EMA from the weight before
// the step, frozen ranges, stores, the bf16 refresh; 4-wide and scalar), the regulariser's finish and the workgroup sum of
// doubles.  The kernels keep their loop shape, how they scale g' and which rule call they make.
#pragma once
#include "optim_rules.h"

namespace {

// step control block (two floats, summed over ranks with the beta gradients): [0] grid-barrier timeouts of this
// step's one-launch BN backward (its gradients are poisoned), [1] ranks that asked to stop (input exhausted).
// Either non-zero: the step is NOT applied -- no update, no EMA, nothing written (uniform branch).  The clip block of
// clip_finalize_kernel starts with the same two words.
__device__ __forceinline__ bool gated(const float* ctl) { return ctl && (ctl[0] != 0.f || ctl[1] != 0.f); }

// The streams of one range and the per-element surroundings of its rule.  s0 / s1: the rule's slots (those beyond Rule::kSlots
// are never touched and may be NULL).  kG: g is read; kWr: the slots are written back (the trusted adam apply pass does
// neither: Rule::kTrustReadsG / kTrustWritesSlots).  A frozen range (trainable = 0) keeps its EMA, the regulariser sum and the
// bf16 refresh, and touches neither g nor the slots.  new_w(path, w, g, slot a, slot b) returns the weight after the step;
// path: std::true_type from four(), std::false_type from one().
template <class Rule, bool kG, bool kWr>
struct OptBody {
  static constexpr bool kA = Rule::kSlots >= 1, kB = Rule::kSlots >= 2;
  float* w;
  const float* g;
  float* s0;
  float* s1;
  float* ema;
  unsigned short* wb;
  float ema_decay;
  int trainable;
  float sq;                                                  // this thread's sum of w^2 (before the step), for reg_finish

  // 16-byte accesses where every stream in use is 16-byte aligned (the flat parameter buffers are; round 6: the 4-byte form
  // streamed 1.8 GB per step at 5.5 TB/s; wb 8-byte), element by element otherwise
  __device__ __forceinline__ bool aligned() const {
    return ((reinterpret_cast<uintptr_t>(w) | (kG ? reinterpret_cast<uintptr_t>(g) : 0) | (kA ? reinterpret_cast<uintptr_t>(s0) : 0) |
             (kB ? reinterpret_cast<uintptr_t>(s1) : 0) | reinterpret_cast<uintptr_t>(ema)) & 15) == 0 &&
           (reinterpret_cast<uintptr_t>(wb) & 7) == 0;
  }

  template <class Path, class F>
  __device__ __forceinline__ float elem(Path path, float wi, float gi, float& ai, float& bi, float& emai, const F& new_w) {
    sq = fmaf(wi, wi, sq);
    if (ema) emai = fmaf(-(1.0f - ema_decay), emai - wi, emai);       // emai - (1 - ema_decay) * (emai - wi)
    if (trainable) wi = new_w(path, wi, gi, ai, bi);
    return wi;
  }

  // element e
  template <class F>
  __device__ __forceinline__ void one(long long e, const F& new_w) {
    float ai = 0.f, bi = 0.f, gi = 0.f, emai = ema ? ema[e] : 0.f;
    if (trainable) {
      if constexpr (kG) gi = g[e];
      if constexpr (kA) ai = s0[e];
      if constexpr (kB) bi = s1[e];
    }
    const float wi = elem(std::false_type{}, w[e], gi, ai, bi, emai, new_w);
    if (ema) ema[e] = emai;
    if (trainable) {
      if constexpr (kA && kWr) s0[e] = ai;
      if constexpr (kB && kWr) s1[e] = bi;
      w[e] = wi;
    }
    if (wb) wb[e] = (unsigned short)f2bf(wi);
  }

  // elements e .. e + 3; aligned() holds and e is a multiple of 4
  template <class F>
  __device__ __forceinline__ void four(long long e, const F& new_w) {
    const std::true_type vec{};
    float4 wv = *reinterpret_cast<const float4*>(w + e);
    float4 ev = ema ? *reinterpret_cast<const float4*>(ema + e) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 gv = make_float4(0.f, 0.f, 0.f, 0.f), av = gv, bv = gv;
    if (trainable) {
      if constexpr (kG) gv = *reinterpret_cast<const float4*>(g + e);
      if constexpr (kA) av = *reinterpret_cast<const float4*>(s0 + e);
      if constexpr (kB) bv = *reinterpret_cast<const float4*>(s1 + e);
    }
    wv.x = elem(vec, wv.x, gv.x, av.x, bv.x, ev.x, new_w); wv.y = elem(vec, wv.y, gv.y, av.y, bv.y, ev.y, new_w);
    wv.z = elem(vec, wv.z, gv.z, av.z, bv.z, ev.z, new_w); wv.w = elem(vec, wv.w, gv.w, av.w, bv.w, ev.w, new_w);
    if (ema) *reinterpret_cast<float4*>(ema + e) = ev;
    if (trainable) {
      if constexpr (kA && kWr) *reinterpret_cast<float4*>(s0 + e) = av;
      if constexpr (kB && kWr) *reinterpret_cast<float4*>(s1 + e) = bv;
      *reinterpret_cast<float4*>(w + e) = wv;
    }
    if (wb) *reinterpret_cast<uint2*>(wb + e) = make_uint2(pack2bf(wv.x, wv.y), pack2bf(wv.z, wv.w));
  }
};

// The regulariser 0.5 * wd * sum w^2 of a workgroup from its threads' sums: lanes by butterfly, four partial sums through LDS,
// one atomic from thread 0.  (The only LDS of an apply kernel.)
__device__ __forceinline__ void reg_finish(float sq, float wd, float* __restrict__ reg_loss) {
  if (!reg_loss || wd == 0.f) return;
  sq = wave_sum(sq);
  __shared__ float red[kT / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < kT / 64; ++i) t += red[i];
    atomicAdd(reg_loss, 0.5f * wd * t);
  }
}

// N doubles per thread summed over the workgroup, in place: lanes by butterfly, then the four wavefronts added in order by
// thread 0 -- no atomics, a fixed order.  True on thread 0, which holds the sums; every thread of the workgroup must call it.
template <int N>
__device__ __forceinline__ bool block_sum(double (&a)[N]) {
  __shared__ double red[N][kT / 64];
#pragma unroll
  for (int k = 0; k < N; ++k) a[k] = wave_sum(a[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[k][threadIdx.x >> 6] = a[k];
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    a[k] = 0.0;
    for (int j = 0; j < kT / 64; ++j) a[k] += red[k][j];
  }
  return true;
}

}  // namespace
