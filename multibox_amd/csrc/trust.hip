// libmbx: layer-wise trust ratios for the optimiser (LARS on sgd, LAMB on adam / adamw); the contract is in include/mbx.h.
// A trainable range is cut into CHUNKS on the host (mbx_trust_plan): on the grid of multiples of kChunk and at every variable
// bound, so a chunk lies in one variable.  One workgroup of kT owns one chunk in every pass:
//   norm pass    two sums of squares per chunk in double, each into its own slot -- no atomics
//   ratios       one wavefront per variable sums that variable's slots in a fixed order
//   apply pass   opt_ema_kernel's element body (optim_body.h; optim_rules.h: the same rules) with the variable's ratio
// All HBM-bound streams: 16-byte accesses over the body of a chunk, scalars for the head up to 4-element alignment and for
// the tail; element by element throughout when a pointer is not 16-byte aligned.
#include "optim_body.h"

namespace {

constexpr int kChunk = 8192;                                 // elements; 8 x 16 bytes per lane and stream

typedef mbx_trust_chunk Chunk;
typedef mbx_trust_var Var;

// The split of one chunk: [0, head) scalars, n4 16-byte groups from lo + head (a multiple of 4 in range coordinates: 16-byte
// aligned where the range base is), the rest scalars.  vec = false: everything is head.
struct Split { int head, n4; };
__device__ __forceinline__ Split split_of(const Chunk& c, bool vec) {
  if (!vec) return Split{c.len, 0};
  int head = (int)((4 - (c.lo & 3)) & 3);
  if (head > c.len) head = c.len;
  return Split{head, (c.len - head) >> 2};
}

// the two sums of this workgroup's chunk (block_sum: a fixed order) into the chunk's own slots
__device__ __forceinline__ void store_sums(double (&acc)[2], double* __restrict__ partials) {
  if (!block_sum(acc)) return;
  partials[2 * (long long)blockIdx.x] = acc[0];
  partials[2 * (long long)blockIdx.x + 1] = acc[1];
}

// sgd: sum w^2 and sum x^2, x = clip[2] * g' in float32 (the optimiser's own expression), widened and squared in double
__global__ void __launch_bounds__(kT)
trust_norms_sgd_kernel(const float* __restrict__ w, const float* __restrict__ g, const Chunk* __restrict__ chunks, float wd,
                       double* __restrict__ partials, const float* __restrict__ ctl, int clipped) {
  if (gated(ctl)) return;
  const float scale = clipped ? ctl[2] : 1.f;                // (x * 1.0f is x)
  const Chunk c = chunks[blockIdx.x];
  const bool vec = ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(g)) & 15) == 0;
  const Split sp = split_of(c, vec);
  double acc[2] = {0.0, 0.0};                                // sum w^2, sum x^2
  auto add = [&](float wi, float gi) {
    const double dw = (double)wi, dx = (double)(scale * opt_grad(gi, wd, wi));
    acc[0] += dw * dw;
    acc[1] += dx * dx;
  };
  for (int i = threadIdx.x; i < sp.head; i += kT) add(w[c.lo + i], g[c.lo + i]);
  const float4* w4 = reinterpret_cast<const float4*>(w + c.lo + sp.head);
  const float4* g4 = reinterpret_cast<const float4*>(g + c.lo + sp.head);
  int i = threadIdx.x;
  for (; i + kT < sp.n4; i += 2 * kT) {                      // four independent loads per lane in flight
    const float4 wa = w4[i], wb = w4[i + kT], ga = g4[i], gb = g4[i + kT];
    add(wa.x, ga.x); add(wa.y, ga.y); add(wa.z, ga.z); add(wa.w, ga.w);
    add(wb.x, gb.x); add(wb.y, gb.y); add(wb.z, gb.z); add(wb.w, gb.w);
  }
  if (i < sp.n4) {
    const float4 wa = w4[i], ga = g4[i];
    add(wa.x, ga.x); add(wa.y, ga.y); add(wa.z, ga.z); add(wa.w, ga.w);
  }
  for (int j = sp.head + 4 * sp.n4 + threadIdx.x; j < c.len; j += kT) add(w[c.lo + j], g[c.lo + j]);
  store_sums(acc, partials);
}

// adam: the moments are UPDATED here (AdamRule::Ready::moments, as mbx_adam_ema_step does), u formed from them by the rule's own
// expression; sum w^2 and sum u^2
__global__ void __launch_bounds__(kT)
trust_moments_adam_kernel(const float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                          const Chunk* __restrict__ chunks, float wd, double* __restrict__ partials, const float* __restrict__ ctl,
                          int clipped, const AdamRule rule) {
  if (gated(ctl)) return;
  const float scale = clipped ? ctl[2] : 1.f;
  const auto step = rule.ready();
  const Chunk c = chunks[blockIdx.x];
  const bool vec = ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                     reinterpret_cast<uintptr_t>(v)) & 15) == 0;
  const Split sp = split_of(c, vec);
  double acc[2] = {0.0, 0.0};                                // sum w^2, sum u^2
  auto one = [&](float wi, float gi, float& mi, float& vi) {
    step.moments(scale * opt_grad(gi, wd, wi), mi, vi);
    const double dw = (double)wi, du = (double)step.update(wi, mi, vi);
    acc[0] += dw * dw;
    acc[1] += du * du;
  };
  auto scalar = [&](long long e) {
    float mi = m[e], vi = v[e];
    one(w[e], g[e], mi, vi);
    m[e] = mi;
    v[e] = vi;
  };
  for (int i = threadIdx.x; i < sp.head; i += kT) scalar(c.lo + i);
  const long long b = c.lo + sp.head;
  const float4* w4 = reinterpret_cast<const float4*>(w + b);
  const float4* g4 = reinterpret_cast<const float4*>(g + b);
  float4* m4 = reinterpret_cast<float4*>(m + b);
  float4* v4 = reinterpret_cast<float4*>(v + b);
  for (int i = threadIdx.x; i < sp.n4; i += kT) {
    const float4 wv = w4[i], gv = g4[i];
    float4 mv = m4[i], vv = v4[i];
    one(wv.x, gv.x, mv.x, vv.x); one(wv.y, gv.y, mv.y, vv.y); one(wv.z, gv.z, mv.z, vv.z); one(wv.w, gv.w, mv.w, vv.w);
    m4[i] = mv;
    v4[i] = vv;
  }
  for (int j = sp.head + 4 * sp.n4 + threadIdx.x; j < c.len; j += kT) scalar(c.lo + j);
  store_sums(acc, partials);
}

// One wavefront per variable: lane l sums the slots of chunks first + l, first + l + 64, ... in that order, then the butterfly.
// r = coeff * sqrt(sum w^2) / sqrt(sum x^2) in double, rounded to float32 once; exactly 1.0f for a variable that does not
// adapt or has a zero norm.  No epsilon, no special case for a non-finite norm.
__global__ void __launch_bounds__(kT)
trust_ratios_kernel(const double* __restrict__ partials, const Var* __restrict__ vars, int n_vars, float coeff,
                    float* __restrict__ ratio, const float* __restrict__ ctl) {
  if (gated(ctl)) return;
  const int var = blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
  if (var >= n_vars) return;                                 // (wavefront-uniform)
  const Var vr = vars[var];
  double sw = 0.0, sx = 0.0;
  for (int k = mbx_lane(); k < vr.n_chunks; k += 64) {
    sw += partials[2 * (long long)(vr.first_chunk + k)];
    sx += partials[2 * (long long)(vr.first_chunk + k) + 1];
  }
  sw = wave_sum(sw);
  sx = wave_sum(sx);
  if (mbx_lane() != 0) return;
  float r = 1.0f;
  if (vr.adapt) {
    const double nw = sqrt(sw), nx = sqrt(sx);
    if (nw > 0.0 && nx > 0.0) r = (float)((double)coeff * nw / nx);
  }
  ratio[var] = r;
}

// OptBody's surroundings around Rule::trust, one workgroup per chunk, the variable's ratio loaded once per workgroup.  s0 / s1:
// the rule's slots; adam only reads them (kTrustWritesSlots) and does not read g (kTrustReadsG).
template <class Rule>
__global__ void __launch_bounds__(kT)
trust_apply_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ s0, float* __restrict__ s1,
                   float* __restrict__ ema, unsigned short* __restrict__ wb, float wd, float ema_decay, int trainable,
                   float* __restrict__ reg_loss, const float* __restrict__ ctl, int clipped, const Chunk* __restrict__ chunks,
                   const float* __restrict__ ratio, const Rule rule) {
  if (gated(ctl)) return;
  constexpr bool kG = Rule::kTrustReadsG;
  const float scale = clipped ? ctl[2] : 1.f;
  const auto step = rule.ready();
  const Chunk c = chunks[blockIdx.x];
  const float r = ratio[c.var];
  auto new_w = [&](auto, float wi, float gi, float& ai, float& bi) -> float {
    return step.trust(wi, kG ? scale * opt_grad(gi, wd, wi) : 0.f, ai, bi, r);
  };
  OptBody<Rule, kG, Rule::kTrustWritesSlots> body{w, g, s0, s1, ema, wb, ema_decay, trainable, 0.f};
  const Split sp = split_of(c, body.aligned());
  for (int i = threadIdx.x; i < sp.head; i += kT) body.one(c.lo + i, new_w);
  const long long b = c.lo + sp.head;
  for (int i = threadIdx.x; i < sp.n4; i += kT) body.four(b + 4 * i, new_w);
  for (int j = sp.head + 4 * sp.n4 + threadIdx.x; j < c.len; j += kT) body.one(c.lo + j, new_w);
  reg_finish(body.sq, wd, reg_loss);
}

template <class Rule>
int launch_trust_apply(float* w, const float* g, float* s0, float* s1, float* ema, void* w_bf16, float wd, float ema_decay,
                       int trainable, float* reg_loss, const float* ctl, int clipped, const Chunk* chunks, int n_chunks,
                       const float* ratio, const Rule& rule, mbx_stream_t stream) {
  MBX_ENTER();
  hipLaunchKernelGGL((trust_apply_kernel<Rule>), dim3(n_chunks), dim3(kT), 0, mbx_s(stream), w, g, s0, s1, ema, (us)w_bf16, wd,
                     ema_decay, trainable, reg_loss, ctl, clipped, chunks, ratio, rule);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

// the plan's arguments: n_vars >= 1, bounds ascending from 0 with no empty variable, fewer than 2^31 chunks
bool bounds_ok(const int64_t* bounds, int64_t n_vars) {
  if (!bounds || n_vars < 1 || n_vars >= (1LL << 31) || bounds[0] != 0) return false;
  for (int64_t i = 0; i < n_vars; ++i)
    if (bounds[i + 1] <= bounds[i]) return false;
  return bounds[n_vars] / kChunk + 2 * n_vars < (1LL << 31);
}

// chunks of variable [lo, hi): cut at every multiple of kChunk strictly inside
inline int64_t chunks_of(int64_t lo, int64_t hi) { return (hi - 1) / kChunk - lo / kChunk + 1; }

inline bool count_ok(int64_t n) { return n > 0 && n < (1LL << 31); }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

// ================================================================================== C ABI
extern "C" int64_t mbx_trust_chunk_elems(void) { return kChunk; }

extern "C" int64_t mbx_trust_plan_count(const int64_t* bounds, int64_t n_vars) {
  if (!bounds_ok(bounds, n_vars)) return 0;
  int64_t n = 0;
  for (int64_t i = 0; i < n_vars; ++i) n += chunks_of(bounds[i], bounds[i + 1]);
  return n;
}

extern "C" int mbx_trust_plan(const int64_t* bounds, const int32_t* adapt, int64_t n_vars, mbx_trust_chunk* chunks_out,
                              mbx_trust_var* vars_out) {
  if (!bounds_ok(bounds, n_vars) || !adapt || !chunks_out || !vars_out) return MBX_ERR_INVALID_ARG;
  int64_t k = 0;
  for (int64_t i = 0; i < n_vars; ++i) {
    const int64_t hi = bounds[i + 1], first = k;
    for (int64_t lo = bounds[i]; lo < hi; ++k) {
      int64_t end = (lo / kChunk + 1) * kChunk;
      if (end > hi) end = hi;
      chunks_out[k] = mbx_trust_chunk{lo, (int32_t)(end - lo), (int32_t)i};
      lo = end;
    }
    vars_out[i] = mbx_trust_var{(int32_t)first, (int32_t)(k - first), adapt[i] != 0, 0};
  }
  return MBX_OK;
}

extern "C" int mbx_trust_norms_sgd(const float* w, const float* g, const mbx_trust_chunk* chunks, int64_t n_chunks, float wd_l2,
                                   double* partials, const float* ctl, int clipped, mbx_stream_t stream) {
  if (!w || !g || !chunks || !count_ok(n_chunks) || !(wd_l2 >= 0.f) || !partials || !al8(partials) || !al8(chunks) ||
      (clipped && !ctl))
    return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  hipLaunchKernelGGL(trust_norms_sgd_kernel, dim3((int)n_chunks), dim3(kT), 0, mbx_s(stream), w, g, chunks, wd_l2, partials, ctl,
                     clipped);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_trust_moments_adam(const float* w, const float* g, float* m, float* v, const mbx_trust_chunk* chunks,
                                      int64_t n_chunks, float beta1, float beta2, float eps, float wd_l2, float wd_decoupled,
                                      int64_t calls, const int64_t* skipped, double* partials, const float* ctl, int clipped,
                                      mbx_stream_t stream) {
  if (!w || !g || !m || !v || !chunks || !count_ok(n_chunks) || !in_unit(beta1) || !in_unit(beta2) || !(eps > 0.f) ||
      !(wd_l2 >= 0.f) || !(wd_decoupled >= 0.f) || calls < 0 || !partials || !al8(partials) || !al8(chunks) || (clipped && !ctl))
    return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  hipLaunchKernelGGL(trust_moments_adam_kernel, dim3((int)n_chunks), dim3(kT), 0, mbx_s(stream), w, g, m, v, chunks, wd_l2, partials,
                     ctl, clipped,
                     AdamRule{0.f, beta1, beta2, eps, wd_decoupled, (long long)calls, reinterpret_cast<const long long*>(skipped)});
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_trust_ratios(const double* partials, const mbx_trust_var* vars, int64_t n_vars, float coeff, float* ratio,
                                const float* ctl, mbx_stream_t stream) {
  if (!partials || !al8(partials) || !vars || !count_ok(n_vars) || !(coeff > 0.f) || !(coeff - coeff == 0.f) || !ratio)
    return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  hipLaunchKernelGGL(trust_ratios_kernel, dim3((int)((n_vars + kT / 64 - 1) / (kT / 64))), dim3(kT), 0, mbx_s(stream), partials, vars,
                     (int)n_vars, coeff, ratio, ctl);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_sgd_ema_step_trust(float* w, const float* g, float* mom, float* ema, void* w_bf16, int64_t n, float lr,
                                      float momentum, int nesterov, float wd_l2, float ema_decay, int trainable, float* reg_loss,
                                      const float* ctl, int clipped, const mbx_trust_chunk* chunks, int64_t n_chunks,
                                      const float* ratio, mbx_stream_t stream) {
  if (!w || n < 0 || (trainable && !g) || !in_unit(momentum) || (mom != nullptr) != (momentum != 0.f) || !(wd_l2 >= 0.f) ||
      (clipped && !ctl) || !chunks || !al8(chunks) || n_chunks < 0 || n_chunks >= (1LL << 31) || !ratio)
    return MBX_ERR_INVALID_ARG;
  if (n == 0 || n_chunks == 0) return MBX_OK;
  if (mom)
    return launch_trust_apply(w, g, mom, nullptr, ema, w_bf16, wd_l2, ema_decay, trainable, reg_loss, ctl, clipped, chunks,
                              (int)n_chunks, ratio, SgdRule<true>{lr, momentum, nesterov}, stream);
  return launch_trust_apply(w, g, nullptr, nullptr, ema, w_bf16, wd_l2, ema_decay, trainable, reg_loss, ctl, clipped, chunks,
                            (int)n_chunks, ratio, SgdRule<false>{lr, 0.f, 0}, stream);
}

extern "C" int mbx_adam_ema_step_trust(float* w, const float* g, float* m, float* v, float* ema, void* w_bf16, int64_t n, float lr,
                                       float beta1, float beta2, float eps, float wd_l2, float wd_decoupled, int64_t calls,
                                       const int64_t* skipped, float ema_decay, int trainable, float* reg_loss, const float* ctl,
                                       int clipped, const mbx_trust_chunk* chunks, int64_t n_chunks, const float* ratio,
                                       mbx_stream_t stream) {
  if (!w || n < 0 || (trainable && (!g || !m || !v)) || !in_unit(beta1) || !in_unit(beta2) || !(eps > 0.f) || !(wd_l2 >= 0.f) ||
      !(wd_decoupled >= 0.f) || calls < 0 || (clipped && !ctl) || !chunks || !al8(chunks) || n_chunks < 0 ||
      n_chunks >= (1LL << 31) || !ratio)
    return MBX_ERR_INVALID_ARG;
  if (n == 0 || n_chunks == 0) return MBX_OK;
  return launch_trust_apply(w, g, m, v, ema, w_bf16, wd_l2, ema_decay, trainable, reg_loss, ctl, clipped, chunks, (int)n_chunks,
                            ratio,
                            AdamRule{lr, beta1, beta2, eps, wd_decoupled, (long long)calls, reinterpret_cast<const long long*>(skipped)},
                            stream);
}
