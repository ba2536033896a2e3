// libmbx: the optimiser step -- one fused launch per range (rule + L2 + EMA + bf16 refresh) for RMSProp, SGD and Adam(W), the
// EMA of the moving statistics, and global-norm clipping (the squared norm of g', the clip block).  The rules: optim_rules.h;
// what stands around them: optim_body.h; the layer-wise trust passes: trust.hip.  All HBM-bound streams, grid-stride loops
// capped at 2048 blocks.
#include "optim_body.h"

namespace {

// A rule's step over one range: 16-byte accesses over n / 4 groups where OptBody::aligned(), element by element otherwise and
// for the n % 4 tail.  kClip: ctl is the CLIP BLOCK of clip_finalize_kernel (words [0], [1] the step control block, [2] the scale)
// and g' = clip[2] * g'.  A scale of exactly 1.0f changes no bit.  A pure streaming pass: no LDS beyond the regulariser's four
// partial sums.
template <bool kClip, class Rule>
__global__ void __launch_bounds__(kT)
opt_ema_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ s0, float* __restrict__ s1,
               float* __restrict__ ema, unsigned short* __restrict__ wb, long long n, float wd, float ema_decay, int trainable,
               float* __restrict__ reg_loss, const float* __restrict__ ctl, const Rule rule) {
  if (gated(ctl)) return;
  float scale = 1.f;
  if constexpr (kClip) scale = ctl[2];
  const auto step = rule.ready();
  auto new_w = [&](auto path, float wi, float gi, float& ai, float& bi) -> float {
    gi = opt_grad(gi, wd, wi);
    if constexpr (kClip) gi = scale * gi;
    return step(path, wi, gi, ai, bi);
  };
  OptBody<Rule, true, true> body{w, g, s0, s1, ema, wb, ema_decay, trainable, 0.f};
  const long long n4 = body.aligned() ? n / 4 : 0;
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n4; i += (long long)gridDim.x * kT) body.four(4 * i, new_w);
  for (long long i = 4 * n4 + (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) body.one(i, new_w);
  reg_finish(body.sq, wd, reg_loss);
}

template <class Rule>
int launch_opt(int clipped, float* w, const float* g, float* s0, float* s1, float* ema, void* w_bf16, long long n, float wd,
               float ema_decay, int trainable, float* reg_loss, const float* ctl, const Rule& rule, mbx_stream_t stream) {
  MBX_ENTER();
  if (clipped)
    hipLaunchKernelGGL((opt_ema_kernel<true, Rule>), dim3(grid_for(n)), dim3(kT), 0, mbx_s(stream), w, g, s0, s1, ema, (us)w_bf16, n, wd,
                       ema_decay, trainable, reg_loss, ctl, rule);
  else
    hipLaunchKernelGGL((opt_ema_kernel<false, Rule>), dim3(grid_for(n)), dim3(kT), 0, mbx_s(stream), w, g, s0, s1, ema, (us)w_bf16, n, wd,
                       ema_decay, trainable, reg_loss, ctl, rule);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

// both RMSProp entry points behind their argument checks
int launch_rmsprop(int clipped, float* w, const float* g, float* ms, float* mom, float* ema, void* w_bf16, long long n, float lr,
                   float decay, float momentum, float eps, float wd, float ema_decay, int trainable, float* reg_loss,
                   const float* ctl, mbx_stream_t stream) {
  if (momentum != 0.f)
    return launch_opt(clipped, w, g, ms, mom, ema, w_bf16, n, wd, ema_decay, trainable, reg_loss, ctl,
                      RmsRule<true>{lr, decay, momentum, eps}, stream);
  return launch_opt(clipped, w, g, ms, nullptr, ema, w_bf16, n, wd, ema_decay, trainable, reg_loss, ctl,
                    RmsRule<false>{lr, decay, 0.f, eps}, stream);
}

__global__ void __launch_bounds__(kT)
ema_update_kernel(float* __restrict__ ema, const float* __restrict__ v, long long n, float d,
                  const float* __restrict__ skip_ctl) {
  if (gated(skip_ctl)) return;
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
    const float e = ema[i];
    ema[i] = e - (1.0f - d) * (e - v[i]);
  }
}

// ------------------------------------------------------------------- global-norm clipping
// Sum of g'^2 over one range, one double per workgroup in its own slot: no atomics, so the result does not depend on the order
// the workgroups arrive in.  The grid (sqnorm_grid) and the thread-to-element mapping are fixed functions of n and of the
// pointers' alignment.  A streaming read: 16-byte loads where g and w are 16-byte aligned (opt_ema_kernel's rule), two
// grid strides per iteration (four independent loads per lane; 2048 x 256 lanes x 64 B = 128 KiB in flight per CU), element by
// element otherwise and for the tail.  g' is rounded to float32 like the optimiser's, then widened: 3e19^2 overflows a float.
// kW: the range has a decay term (w is read); a compile-time switch -- a run-time "load or zero" per element turns the
// 16-byte loads of w into four guarded 4-byte ones.
template <bool kW>
__global__ void __launch_bounds__(kT)
grad_sqnorm_kernel(const float* __restrict__ g, const float* __restrict__ w, long long n, float wd, double* __restrict__ partials) {
  double acc[1] = {0.0};
  auto add = [&](float gi, float wi) { const double v = (double)opt_grad(gi, wd, wi); acc[0] += v * v; };
  auto add4 = [&](const float4 a, const float4 b) { add(a.x, b.x); add(a.y, b.y); add(a.z, b.z); add(a.w, b.w); };
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool vec = ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(w)) & 15) == 0;
  const long long n4 = vec ? n / 4 : 0, stride = (long long)gridDim.x * kT;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const float4* w4 = reinterpret_cast<const float4*>(w);
  long long i = (long long)blockIdx.x * kT + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {
    const float4 ga = g4[i], gb = g4[i + stride];
    const float4 wa = kW ? w4[i] : z4, wb = kW ? w4[i + stride] : z4;
    add4(ga, wa);
    add4(gb, wb);
  }
  if (i < n4) add4(g4[i], kW ? w4[i] : z4);
  for (i = 4 * n4 + (long long)blockIdx.x * kT + threadIdx.x; i < n; i += stride) add(g[i], kW ? w[i] : 0.f);
  if (block_sum(acc)) partials[blockIdx.x] = acc[0];
}

// One workgroup: the slots of every range in a fixed order (thread-strided, then block_sum), then the clip block.  Everything in
// double; see mbx_clip_finalize (include/mbx.h) for the words.
__global__ void __launch_bounds__(kT)
clip_finalize_kernel(const double* __restrict__ partials, long long n_slots, double max_norm, const float* __restrict__ ctl,
                     float* __restrict__ clip, long long* __restrict__ counts) {
  double acc[1] = {0.0};
  for (long long i = threadIdx.x; i < n_slots; i += kT) acc[0] += partials[i];
  if (!block_sum(acc)) return;
  const double total = acc[0];
  const float c0 = ctl[0], c1 = ctl[1];
  const bool finite = total - total == 0.0;                  // false for an infinite and for a NaN sum
  const double norm = sqrt(total);
  const bool clipped = finite && norm > max_norm;
  const double scale = clipped ? max_norm / norm : 1.0;
  clip[0] = c0;
  clip[1] = c1 + (finite ? 0.f : 1.f);
  clip[2] = (float)scale;
  clip[3] = (float)norm;
  clip[4] = clipped ? 1.f : 0.f;
  clip[5] = clip[6] = clip[7] = 0.f;
  if (c0 == 0.f && c1 == 0.f) {                              // an already flagged step has its cause: count nothing
    if (clipped) counts[0] += 1;
    if (!finite) counts[1] += 1;
  }
}

inline int sqnorm_grid(long long n) { return grid_for((n + 3) / 4); }

}  // namespace

// ================================================================================== C ABI
extern "C" int mbx_rmsprop_ema_step(float* w, const float* g, float* ms, float* mom, float* ema, void* w_bf16, int64_t n,
                                    float lr, float decay, float momentum, float eps, float wd, float ema_decay,
                                    int trainable, float* reg_loss, const float* skip_ctl, mbx_stream_t stream) {
  if (!w || n <= 0 || (trainable && (!g || !ms))) return MBX_ERR_INVALID_ARG;
  if (trainable && momentum != 0.f && !mom) return MBX_ERR_INVALID_ARG;
  return launch_rmsprop(0, w, g, ms, mom, ema, w_bf16, n, lr, decay, momentum, eps, wd, ema_decay, trainable, reg_loss, skip_ctl,
                        stream);
}

extern "C" int mbx_rmsprop_ema_step_clipped(float* w, const float* g, float* ms, float* mom, float* ema, void* w_bf16, int64_t n,
                                            float lr, float decay, float momentum, float eps, float wd, float ema_decay,
                                            int trainable, float* reg_loss, const float* clip, mbx_stream_t stream) {
  if (!w || n <= 0 || (trainable && (!g || !ms)) || !clip) return MBX_ERR_INVALID_ARG;
  if (trainable && momentum != 0.f && !mom) return MBX_ERR_INVALID_ARG;
  return launch_rmsprop(1, w, g, ms, mom, ema, w_bf16, n, lr, decay, momentum, eps, wd, ema_decay, trainable, reg_loss, clip, stream);
}

extern "C" int mbx_sgd_ema_step(float* w, const float* g, float* mom, float* ema, void* w_bf16, int64_t n, float lr, float momentum,
                                int nesterov, float wd_l2, float ema_decay, int trainable, float* reg_loss, const float* ctl,
                                int clipped, mbx_stream_t stream) {
  if (!w || n < 0 || (trainable && !g) || !in_unit(momentum) || (mom != nullptr) != (momentum != 0.f) || !(wd_l2 >= 0.f) ||
      (clipped && !ctl))
    return MBX_ERR_INVALID_ARG;
  if (n == 0) return MBX_OK;
  if (mom)
    return launch_opt(clipped, w, g, mom, nullptr, ema, w_bf16, n, wd_l2, ema_decay, trainable, reg_loss, ctl,
                      SgdRule<true>{lr, momentum, nesterov}, stream);
  return launch_opt(clipped, w, g, nullptr, nullptr, ema, w_bf16, n, wd_l2, ema_decay, trainable, reg_loss, ctl,
                    SgdRule<false>{lr, 0.f, 0}, stream);
}

extern "C" int mbx_adam_ema_step(float* w, const float* g, float* m, float* v, float* ema, void* w_bf16, int64_t n, float lr,
                                 float beta1, float beta2, float eps, float wd_l2, float wd_decoupled, int64_t calls,
                                 const int64_t* skipped, float ema_decay, int trainable, float* reg_loss, const float* ctl,
                                 int clipped, mbx_stream_t stream) {
  if (!w || n < 0 || (trainable && (!g || !m || !v)) || !in_unit(beta1) || !in_unit(beta2) || !(eps > 0.f) || !(wd_l2 >= 0.f) ||
      !(wd_decoupled >= 0.f) || calls < 0 || (clipped && !ctl))
    return MBX_ERR_INVALID_ARG;
  if (n == 0) return MBX_OK;
  return launch_opt(clipped, w, g, m, v, ema, w_bf16, n, wd_l2, ema_decay, trainable, reg_loss, ctl,
                    AdamRule{lr, beta1, beta2, eps, wd_decoupled, (long long)calls, reinterpret_cast<const long long*>(skipped)}, stream);
}

extern "C" int mbx_ema_update(float* ema, const float* value, int64_t n, float ema_decay, const float* skip_ctl,
                              mbx_stream_t stream) {
  if (!ema || !value || n <= 0) return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  hipLaunchKernelGGL(ema_update_kernel, dim3(grid_for(n)), dim3(kT), 0, mbx_s(stream), ema, value, (long long)n, ema_decay, skip_ctl);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int64_t mbx_grad_sqnorm_partials(int64_t n) { return n > 0 ? sqnorm_grid(n) : 0; }

extern "C" int mbx_grad_sqnorm(const float* g, const float* w, int64_t n, float wd, double* partials, mbx_stream_t stream) {
  if (!g || n <= 0 || !partials || (reinterpret_cast<uintptr_t>(partials) & 7) || !(wd == wd) || (wd != 0.f && !w))
    return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  if (wd != 0.f)
    hipLaunchKernelGGL(grad_sqnorm_kernel<true>, dim3(sqnorm_grid(n)), dim3(kT), 0, mbx_s(stream), g, w, (long long)n, wd, partials);
  else
    hipLaunchKernelGGL(grad_sqnorm_kernel<false>, dim3(sqnorm_grid(n)), dim3(kT), 0, mbx_s(stream), g, (const float*)nullptr,
                       (long long)n, 0.f, partials);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_clip_finalize(const double* partials, int64_t n_slots, double max_norm, const float* ctl, float* clip,
                                 int64_t* counts, mbx_stream_t stream) {
  if (!partials || n_slots <= 0 || !(max_norm > 0.0) || !ctl || !clip || !counts || (reinterpret_cast<uintptr_t>(partials) & 7))
    return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(kT), 0, mbx_s(stream), partials, (long long)n_slots, max_norm, ctl, clip,
                     reinterpret_cast<long long*>(counts));
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}
