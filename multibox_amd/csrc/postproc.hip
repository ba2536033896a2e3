// libmbx: detection post-processing -- decode + filter + top-K per patch, and the optional per-patch NMS.  The training
// side (prior decode, matching, loss) is loss.hip.
// HBM/latency-bound integer+float kernels; one workgroup per patch, wave64 shuffle reductions.  Built with
// -ffp-contract=off: the keep decisions are compared bit for bit with the numpy restatements (boxes.h).
#include "boxes.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// A prediction's box: residual + prior in float32, each corner clipped to [0, 1] -> (x1, y1, x2, y2).
__device__ __forceinline__ float4 decode_clipped(const float4 a, const float4 p) {
  return make_float4(fminf(fmaxf(__fadd_rn(a.x, p.x), 0.f), 1.f), fminf(fmaxf(__fadd_rn(a.y, p.y), 0.f), 1.f),
                     fminf(fmaxf(__fadd_rn(a.z, p.z), 0.f), 1.f), fminf(fmaxf(__fadd_rn(a.w, p.w), 0.f), 1.f));
}

// ------------------------------------------------------- decode + filter + top-K
// Key: kept flag (bit 63) | order-preserving image of the confidence's float bits (32 bits) | prediction index
// (31 bits); bitonic sort, descending.  The float image (score_order_key, boxes.h) orders ANY float like a comparison
// sort does -- negative scores and scores >= 2 included; a NaN sorts above everything, where numpy's
// argsort(...)[::-1] (detect.py:423) puts it.
__global__ void __launch_bounds__(kThreads)
decode_filter_topk_kernel(const float4* __restrict__ raw, const float* __restrict__ conf,
                          const float4* __restrict__ priors, const mbx_patch_meta* __restrict__ meta,
                          int P, int N /*pow2 >= P*/, int k_max, double* __restrict__ out_boxes,
                          float* __restrict__ out_scores, int* __restrict__ out_index,
                          int* __restrict__ out_count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
  __shared__ int kept_waves[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const mbx_patch_meta m = meta[b];
  const float4* r = raw + (size_t)b * P;
  const float* c = conf + (size_t)b * P;
  int kept = 0;
  for (int j = tid; j < N; j += kThreads) {
    unsigned long long key = 0ull;
    if (j < P) {
      const float4 q = decode_clipped(r[j], priors[j]);
      // detect.py:92-99 (strict)
      const bool drop = (q.x < m.restrictions[0]) || (q.y < m.restrictions[1]) || (q.z > m.restrictions[2]) || (q.w > m.restrictions[3]);
      if (!drop) {
        key = (1ull << 63) | ((unsigned long long)score_order_key(c[j]) << 31) | (unsigned long long)j;
        ++kept;
      }
    }
    keys[j] = key;
  }
  kept = wave_sum(kept);
  if ((tid & 63) == 0) kept_waves[tid >> 6] = kept;
  __syncthreads();
  int total_kept = 0;
  for (int w = 0; w < kWaves; ++w) total_kept += kept_waves[w];

  lds_bitonic_sort_desc(keys, N, tid, kThreads);
  int count = total_kept < m.max_to_keep ? total_kept : m.max_to_keep;   // detect.py:424
  if (count > k_max) count = k_max;
  if (count < 0) count = 0;
  if (tid == 0) out_count[b] = count;
  // detect.py:119-129
  const double xs = (double)m.patch_w / (double)m.image_w, ys = (double)m.patch_h / (double)m.image_h;
  const double xo = (double)m.offset_x / (double)m.image_w, yo = (double)m.offset_y / (double)m.image_h;
  for (int t = tid; t < k_max; t += kThreads) {
    double* ob = out_boxes + ((size_t)b * k_max + t) * 4;
    if (t < count) {
      const unsigned long long key = keys[t];
      const int j = (int)(key & 0x7fffffffull);
      const float4 q = decode_clipped(r[j], priors[j]);
      double X1 = __dadd_rn(__dmul_rn((double)q.x, xs), xo), Y1 = __dadd_rn(__dmul_rn((double)q.y, ys), yo);
      double X2 = __dadd_rn(__dmul_rn((double)q.z, xs), xo), Y2 = __dadd_rn(__dmul_rn((double)q.w, ys), yo);
      if (m.is_flipped) { const double t1 = 1.0 - X2, t2 = 1.0 - X1; X1 = t1; X2 = t2; }
      ob[0] = X1; ob[1] = Y1; ob[2] = X2; ob[3] = Y2;
      out_scores[(size_t)b * k_max + t] = c[j];
      out_index[(size_t)b * k_max + t] = j;
    } else {
      ob[0] = ob[1] = ob[2] = ob[3] = 0.0;
      out_scores[(size_t)b * k_max + t] = 0.f;
      out_index[(size_t)b * k_max + t] = -1;
    }
  }
}

}  // namespace

// =============================================================================== C ABI
// ------------------------------------------------------------------------------------------ optional NMS (N1)
// The reference has NO non-maximum suppression (detect.py keeps the top max_to_keep boxes of every patch);
// BASELINE's north_star names one, so it exists as an OPTIONAL stage after mbx_decode_filter_topk, off by default.
// Greedy NMS per patch over the score-sorted list: box i is kept iff its IoU with every earlier KEPT box is <= thr.
// One workgroup per patch: the K x K "suppresses" relation as bit rows in LDS (pair (i, j), j > i, computed in
// float64 in the operation order of the numpy restatement: bit-exact decisions), then one wave walks the rows in
// order OR-ing the rows of kept boxes into the removed set (wavefront ballot-free: 64-bit words per lane), then the
// survivors are compacted in place.  K <= 1024.
constexpr int kNmsMaxK = 1024;

__global__ void __launch_bounds__(kThreads)
nms_kernel(double* __restrict__ boxes, float* __restrict__ scores, int32_t* __restrict__ index,
           int32_t* __restrict__ count, int k_max, double thr) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long nms_lds[];
  const int b = blockIdx.x;
  const int K = max(min(count[b], k_max), 0);                // (a count <= -64 made W negative and K * W a positive trip count)
  const int W = (K + 63) >> 6;                               // 64-bit words per row
  unsigned long long* rows = nms_lds;                        // [K][W]
  unsigned long long* removed = nms_lds + (size_t)K * W;     // [W]
  double* bx = boxes + (size_t)b * k_max * 4;
  for (int i = threadIdx.x; i < K * W; i += kThreads) rows[i] = 0ull;
  if (threadIdx.x < W) removed[threadIdx.x] = 0ull;
  __syncthreads();
  // pair (i, j), j > i: thread t takes row i = t / W', word w: 64 columns at a time
  for (int t = threadIdx.x; t < K * W; t += kThreads) {
    const int i = t / W, w = t - i * W;
    const Box bi = {bx[i * 4], bx[i * 4 + 1], bx[i * 4 + 2], bx[i * 4 + 3]};
    const double ai = box_area(bi);
    unsigned long long bits = 0ull;
    const int j0 = max(w * 64, i + 1), j1 = min(w * 64 + 64, K);
    for (int j = j0; j < j1; ++j) {
      const Box bj = {bx[j * 4], bx[j * 4 + 1], bx[j * 4 + 2], bx[j * 4 + 3]};
      if (iou_corners(bi, bj, ai, box_area(bj)) > thr) bits |= 1ull << (j & 63);
    }
    rows[t] = bits;
  }
  __syncthreads();
  if (threadIdx.x < 64) {                                    // one wave: lane w owns word w of the removed set (W <= 16)
    const int lane = threadIdx.x;
    unsigned long long rem = 0ull;
    for (int i = 0; i < K; ++i) {
      const unsigned long long word = __shfl(rem, i >> 6, 64);          // is box i still alive?
      if (!((word >> (i & 63)) & 1ull) && lane < W) rem |= rows[i * W + lane];
    }
    if (lane < W) removed[lane] = rem;
  }
  __syncthreads();
  // compaction: survivor i moves to position (number of survivors before i); one thread per box, prefix by popcount
  int dst = -1;
  double kb[4] = {0, 0, 0, 0};
  float ks = 0.f;
  int ki = 0;
  const int i = threadIdx.x;
  for (int base = 0; base < K; base += kThreads) {           // K <= 1024: at most four sweeps, each box read before any write
    const int ii = base + i;
    dst = -1;
    if (ii < K && !((removed[ii >> 6] >> (ii & 63)) & 1ull)) {
      int before = 0;
      for (int w = 0; w < (ii >> 6); ++w) before += __popcll(~removed[w]);
      before += __popcll(~removed[ii >> 6] & ((1ull << (ii & 63)) - 1ull));
      dst = before;
      kb[0] = bx[ii * 4]; kb[1] = bx[ii * 4 + 1]; kb[2] = bx[ii * 4 + 2]; kb[3] = bx[ii * 4 + 3];
      ks = scores[(size_t)b * k_max + ii];
      ki = index[(size_t)b * k_max + ii];
    }
    __syncthreads();                                          // dst <= ii and all sources of this sweep are in registers
    if (dst >= 0) {
      bx[dst * 4] = kb[0]; bx[dst * 4 + 1] = kb[1]; bx[dst * 4 + 2] = kb[2]; bx[dst * 4 + 3] = kb[3];
      scores[(size_t)b * k_max + dst] = ks;
      index[(size_t)b * k_max + dst] = ki;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int kept = 0;
    for (int w = 0; w < W; ++w) kept += __popcll(~removed[w] & (w == W - 1 && (K & 63) ? ((1ull << (K & 63)) - 1ull) : ~0ull));
    count[b] = K == 0 ? 0 : kept;
  }
}

extern "C" int mbx_nms(double* boxes, float* scores, int32_t* index, int32_t* count, int B, int k_max,
                       double iou_threshold, mbx_stream_t stream) {
  if (!boxes || !scores || !index || !count || B < 0 || k_max <= 0) return MBX_ERR_INVALID_ARG;
  if (k_max > kNmsMaxK) return MBX_ERR_UNSUPPORTED;
  if (B == 0) return MBX_OK;
  const int W = (k_max + 63) / 64;
  const size_t lds = ((size_t)k_max * W + W) * sizeof(unsigned long long);
  MBX_ENTER();
  if (lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(nms_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess) return MBX_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(nms_kernel, dim3(B), dim3(kThreads), lds, mbx_s(stream), boxes, scores, index, count, k_max,
                     iou_threshold);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_decode_filter_topk(const float* raw_locs, const float* conf, const float* priors,
                                      const mbx_patch_meta* meta, int B, int P, int k_max, double* out_boxes,
                                      float* out_scores, int32_t* out_index, int32_t* out_count,
                                      mbx_stream_t stream) {
  if (!raw_locs || !conf || !priors || !meta || !out_boxes || !out_scores || !out_index || !out_count)
    return MBX_ERR_INVALID_ARG;
  if (B < 0 || P <= 0 || k_max <= 0) return MBX_ERR_INVALID_ARG;
  if (B == 0) return MBX_OK;
  int N = 64;
  while (N < P) N <<= 1;
  if (N > 16384) return MBX_ERR_UNSUPPORTED;
  const size_t lds = (size_t)N * sizeof(unsigned long long);
  MBX_ENTER();
  if (lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(decode_filter_topk_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return MBX_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(decode_filter_topk_kernel, dim3(B), dim3(kThreads), lds, mbx_s(stream),
                     reinterpret_cast<const float4*>(raw_locs), conf, reinterpret_cast<const float4*>(priors), meta,
                     P, N, k_max, out_boxes, out_scores, out_index, out_count);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}
