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

}  // namespace
