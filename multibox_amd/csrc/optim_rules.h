// The optimiser's element rules, shared by the flat streaming kernels (optim.hip) and the layer-wise trust kernels (trust.hip):
// ONE copy of g', of each rule and of Adam's bias correction, so that the two sets of kernels cannot drift apart.  What stands
// around a rule in a kernel (loads, EMA, stores, the regulariser's sum): optim_body.h.
#pragma once
#include "vec8.h"
#include <type_traits>

namespace {

// The vector the optimiser consumes, g' = g + wd*w (the L2 regulariser's gradient rides with the loss gradient): ONE
// expression for the update (opt_ema_kernel) and for the norm that clips it (grad_sqnorm_kernel), so the two cannot drift.
__device__ __forceinline__ float opt_grad(float g, float wd, float w) { return fmaf(wd, w, g); }

// a * b + c in two roundings, whatever -ffp-contract says
__device__ __forceinline__ float mul_add_unfused(float a, float b, float c) {
#pragma clang fp contract(off)
  return a * b + c;
}

// ------------------------------------------------------------- optimiser choice (OPTIMIZER: rmsprop, sgd, adam, adamw)
// A rule is a host-side struct of hyper-parameters with kSlots (how many per-element slots it keeps) and ready(), which runs
// once per thread and returns the element functor: new w = f(path, w, g', slot a, slot b).  Every rounding of a functor is
// spelled out (fmaf, or a product / quotient / sum that stands alone: there is no a * b + c left for the compiler to contract),
// so the clipped and unclipped instantiations give the same bits.  path: std::true_type on the 16-byte path, std::false_type
// element by element -- known at compile time, and only RmsRule looks at it; sgd and adam give the same bits on both.
// Layer-wise trust (trust.hip) adds trust(w, g', a, b, r): the same step with the variable's ratio r applied -- to g' under sgd
// (LARS), to the update under adam (LAMB).  r == 1.0f changes no bit.  kTrustReadsG / kTrustWritesSlots: whether the trusted
// apply pass needs g and writes the slots (adam: neither -- mbx_trust_moments_adam has already updated the moments).
template <bool kMom>
struct RmsRule {                                             // tf.train.RMSPropOptimizer; kMom = false: momentum 0, one slot
  static constexpr int kSlots = kMom ? 2 : 1;                // slot 0 the mean square, slot 1 the momentum accumulator
  float lr, decay, momentum, eps;
  __device__ __forceinline__ RmsRule ready() const { return *this; }
  // the roundings this step has always had -- fused multiply-adds, except that the element-by-element path rounds decay * ms
  // on its own
  template <bool kVec>
  __device__ __forceinline__ float operator()(std::bool_constant<kVec>, float w, float g, float& ms, float& mom) const {
    const float gg = (1.0f - decay) * g * g;
    ms = kVec ? fmaf(decay, ms, gg) : mul_add_unfused(decay, ms, gg);   // decay * ms + (1 - decay) * g'^2
    float step = lr * g / sqrtf(ms + eps);
    if constexpr (kMom) { step = fmaf(momentum, mom, step); mom = step; }
    return w - step;
  }
};

template <bool kMom>
struct SgdRule {                                             // tf.train.MomentumOptimizer; kMom = false: momentum 0, no slot
  static constexpr int kSlots = kMom ? 1 : 0;
  static constexpr bool kTrustReadsG = true, kTrustWritesSlots = true;
  float lr, momentum;
  int nesterov;
  __device__ __forceinline__ SgdRule ready() const { return *this; }
  __device__ __forceinline__ float operator()(bool, float w, float g, float& acc, float&) const {
    if constexpr (!kMom) {
      return fmaf(-lr, g, w);                                // w -= lr * g'
    } else {
      acc = fmaf(momentum, acc, g);                          // acc = momentum * acc + g'
      return fmaf(-lr, nesterov ? fmaf(momentum, acc, g) : acc, w);    // w -= lr * acc, or lr * (g' + momentum * acc)
    }
  }
  __device__ __forceinline__ float trust(float w, float g, float& acc, float& b, float r) const { return (*this)(true, w, r * g, acc, b); }
};

// b^t for an integer t >= 0 by squaring, in double (at most 63 rounds, lane-uniform)
__device__ __forceinline__ double pow_int(double b, long long t) {
  double r = 1.0;
  for (; t > 0; t >>= 1, b *= b)
    if (t & 1) r *= b;
  return r;
}

struct AdamRule {                                            // Adam; wd_decoupled != 0: AdamW
  static constexpr int kSlots = 2;
  static constexpr bool kTrustReadsG = false, kTrustWritesSlots = false;
  float lr, beta1, beta2, eps, wd_decoupled;
  long long calls;
  const long long* skipped;
  struct Ready {
    float lr, b1, omb1, b2, omb2, eps, wdd, c1, c2;
    __device__ __forceinline__ void moments(float g, float& m, float& v) const {
      m = fmaf(b1, m, omb1 * g);                             // m = beta1 * m + (1 - beta1) * g'
      v = fmaf(b2, v, (omb2 * g) * g);                       // v = beta2 * v + (1 - beta2) * g'^2
    }
    // u = m^ / (sqrt(v^) + eps) + wd_decoupled * w from the UPDATED moments, w the weight before the step
    __device__ __forceinline__ float update(float w, float m, float v) const {
      const float mhat = m * c1, vhat = v * c2;              // m / bc1, v / bc2
      const float denom = sqrtf(vhat) + eps;
      float upd = mhat / denom;
      if (wdd != 0.f) upd = fmaf(wdd, w, upd);               // + wd_decoupled * w, the weight before the step
      return upd;
    }
    __device__ __forceinline__ float operator()(bool, float w, float g, float& m, float& v) const {
      moments(g, m, v);
      return fmaf(-lr, update(w, m, v), w);
    }
    __device__ __forceinline__ float trust(float w, float, float& m, float& v, float r) const { return fmaf(-lr, r * update(w, m, v), w); }
  };
  // The bias corrections 1 / (1 - beta^t), t = the APPLIED steps including this one: the host's launch count less the steps the
  // device skipped (read before this step's own increment, which comes later on the stream).  Once per thread, in double.
  __device__ __forceinline__ Ready ready() const {
    long long t = calls + 1 - (skipped ? *skipped : 0);
    if (t < 1) t = 1;                                        // calls < *skipped breaks the contract (include/mbx.h): stay defined
    const double bc1 = 1.0 - pow_int((double)beta1, t), bc2 = 1.0 - pow_int((double)beta2, t);
    return Ready{lr, beta1, 1.0f - beta1, beta2, 1.0f - beta2, eps, wd_decoupled, (float)(1.0 / bc1), (float)(1.0 / bc2)};
  }
};

inline bool in_unit(float b) { return b >= 0.f && b < 1.f; }       // [0, 1); false for a NaN

}  // namespace
