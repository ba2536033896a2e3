// Device helpers shared by the box kernels: detection post-processing (postproc.hip: top-K and per-patch NMS; merge.hip: the
// per-image merge and box voting) and the training side (loss.hip: threshold matching takes Box / box_area, the mining keys
// score_order_key).  Keep decisions are compared bit for bit with the numpy restatements, so these files are
// built with -ffp-contract=off and the float64 IoU below keeps the operation order of oracle.ref_numpy.nms_greedy.
// (cocomatch.hip's IoU is NOT this one: the xywh form of the host's _iou_xywh, with its own term order.)
#pragma once
#include "common.h"
#include <math.h>

namespace {

struct Box { double x1, y1, x2, y2; };

__device__ __forceinline__ double box_area(const Box& b) { return (b.x2 - b.x1) * (b.y2 - b.y1); }

// A ground-truth box as the matching kernels behind match_kernel stage it in LDS (loss.hip, match_tal.hip): widened to
// float64 once, with its area (40 B a box).
struct StagedBox { Box box; double area; };

// IoU of the EARLIER (kept) box e and the later box b, given their areas: term by term
//   iw = min(e.x2, b.x2) - max(e.x1, b.x1), ih likewise; inter = iw > 0 && ih > 0 ? iw * ih : 0;
//   uni = area(e) + area(b) - inter (in that order); iou = uni > 0 ? inter / uni : 0
__device__ __forceinline__ double iou_corners(const Box& e, const Box& b, double area_e, double area_b) {
  const double iw = fmin(e.x2, b.x2) - fmax(e.x1, b.x1), ih = fmin(e.y2, b.y2) - fmax(e.y1, b.y1);
  const double inter = (iw > 0.0 && ih > 0.0) ? iw * ih : 0.0;
  const double uni = area_e + area_b - inter;
  return uni > 0.0 ? inter / uni : 0.0;
}
__device__ __forceinline__ double iou_corners(const Box& e, const Box& b, double area_b) {
  return iou_corners(e, b, box_area(e), area_b);
}

// Order-preserving 32-bit image of a float score: flip the sign bit of non-negative values, all bits of negative ones, so
// that unsigned comparison orders ANY float like a comparison sort does; -0 == +0, a NaN sorts above everything (where
// numpy's argsort(...)[::-1] puts it).  Never 0 for a real score: an all-zero key sorts below every candidate.
__device__ __forceinline__ unsigned score_order_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (v != v) ? 0xffffffffu : (v == 0.f) ? 0x80000000u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

// Bitonic sort of keys[0, N) in LDS, DESCENDING; N a power of two >= 2, called by all nthreads threads of the workgroup
// with the keys already visible (a barrier behind the last write).  Ends on a barrier.
__device__ __forceinline__ void lds_bitonic_sort_desc(unsigned long long* keys, const int N, const int tid, const int nthreads) {
  for (int size = 2; size <= N; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (N >> 1); t += nthreads) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long a = keys[lo], bb = keys[hi];
        if ((a < bb) == desc) { keys[lo] = bb; keys[hi] = a; }
      }
      __syncthreads();
    }
  }
}

// The float a score_order_key came from, but for what the key forgets: -0 comes back as +0, every NaN as one NaN.
__device__ __forceinline__ float score_from_order_key(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// Step 1 of the per-image merge kernels (merge.hip, merge_wbf.hip), called by all THREADS threads of the workgroup that
// owns rows [r0, r1): the candidates are the slots [0, clamp(count[r], 0, k_max)) of those rows; key = score_order_key of
// the score << 32 | ~(offset of the slot from the image's first slot), so that a descending sort gives score descending,
// ties by ascending flat index.  keys [MBX_MERGE_MAX_CANDIDATES] is sorted in LDS (bitonic, padded with 0 to a power of
// two).  Returns the number of candidates, the same in every thread; 0 with *too_many set above the limit, and nothing
// is sorted then.  tile_cnt [THREADS] and wave_tot [THREADS / 64] are LDS scratch.  Ends on a barrier.
template <int THREADS>
__device__ __forceinline__ int sorted_candidate_keys(const float* __restrict__ scores, const int32_t* __restrict__ count,
                                                     int r0, int r1, int k_max, unsigned long long* keys, int* tile_cnt,
                                                     int* wave_tot, bool* too_many) {
  const int tid = threadIdx.x;
  // ---- 1a. number of candidates
  int mine = 0;
  for (int r = r0 + tid; r < r1; r += THREADS) mine += min(max(count[r], 0), k_max);
  mine = wave_sum(mine);
  if ((tid & 63) == 0) wave_tot[tid >> 6] = mine;
  __syncthreads();
  int total = 0;
  for (int w = 0; w < THREADS / 64; ++w) total += wave_tot[w];
  *too_many = total > MBX_MERGE_MAX_CANDIDATES;
  if (*too_many) total = 0;
  if (total == 0) return 0;
  // ---- 1b. keys
  int N = 64;
  while (N < total) N <<= 1;
  int off = 0;
  for (int t0 = r0; t0 < r1; t0 += THREADS) {
    const int nrows = min(THREADS, r1 - t0);
    __syncthreads();                                             // the previous tile's counts have been read
    if (tid < nrows) tile_cnt[tid] = min(max(count[t0 + tid], 0), k_max);
    __syncthreads();
    for (int q = 0; q < nrows; ++q) {
      const int c = tile_cnt[q];
      const float* sr = scores + (size_t)(t0 + q) * k_max;
      const unsigned rel0 = (unsigned)(t0 + q - r0) * (unsigned)k_max;
      for (int s = tid; s < c; s += THREADS) {
        keys[off + s] = ((unsigned long long)score_order_key(sr[s]) << 32) | (unsigned long long)(~(rel0 + (unsigned)s));
      }
      off += c;
    }
  }
  for (int j = total + tid; j < N; j += THREADS) keys[j] = 0ull;        // below every candidate's key (its score image is > 0)
  __syncthreads();
  lds_bitonic_sort_desc(keys, N, tid, THREADS);
  return total;
}

}  // namespace
