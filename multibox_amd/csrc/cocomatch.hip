// libmbx: matching of detections to ground truth for the COCO bounding-box metric (eval.py:212-226 hands its boxes to
// pycocotools' COCOeval; this is evaluateImg of that package for one category and no crowd annotations, as
// multibox_amd/cocoeval.py:_evaluate_img restates it).  Built with -ffp-contract=off: the float64 IoU keeps the operation
// order of cocoeval._iou_xywh, so every comparison against a threshold or another IoU is the host's, bit for bit.
#include "common.h"
#include <math.h>

namespace {

constexpr int kMaxDet = MBX_COCO_MAX_DET;
constexpr int kMaxGt = MBX_COCO_MAX_GT;
constexpr int kMaxT = 16;
constexpr int kMaxA = 8;
static_assert(kMaxGt == 128 && kMaxDet <= 128, "two gts and two detections per lane");

// the HOST arrays of the entry point, by value: start[t] = min(iou_thrs[t], 1 - 1e-10), area range a = [a0[a], a1[a]]
struct CocoParams { double start[kMaxT]; double a0[kMaxA]; double a1[kMaxA]; };

// A candidate gt is (class, IoU, row): class 2 = area in range, 1 = out of range, 0 = none; the larger triple wins.
// `code` is class << 8 | row (row < 128).  evaluateImg walks the gts in-range first and keeps the LAST one whose IoU is
// >= the best so far, and it stops before the out-of-range ones once it holds an in-range one: the maximum of this order.
__device__ __forceinline__ bool better(double ia, int ca, double ib, int cb) {
  const int ka = ca >> 8, kb = cb >> 8;
  if (ka != kb) return ka > kb;
  if (ia != ib) return ia > ib;
  return ca > cb;
}

// One workgroup per image, one wavefront per IoU threshold (a wave takes thresholds wave, wave + #waves, ...).
//   1. all threads: the gt corners, then the [nd][128] IoU matrix in LDS (annotation order, independent of the area range).
//   2. per wave and area range: lane l owns gt rows l and l + 64 (in range? still free?) and detections l and l + 64
//      (result registers).  Detections in order: each lane offers the better of its two free gts with IoU >= start, a
//      butterfly of shuffles leaves the winner in every lane, its owner clears the free bit.  A detection nobody can take
//      (one ballot) costs two LDS reads.
//   3. lanes write their detections' match / ignore; slots past the image's detections are -1 / 0.
__global__ void __launch_bounds__(64 * kMaxT)
coco_match_kernel(const double* __restrict__ dt, const int32_t* __restrict__ dt_rows, const double* __restrict__ gt,
                  const int32_t* __restrict__ gt_rows, int T, int A, CocoParams p, int16_t* __restrict__ match,
                  uint8_t* __restrict__ ignore, int32_t* __restrict__ n_gt_counted, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char coco_lds[];
  double* iou = reinterpret_cast<double*>(coco_lds);                 // [kMaxDet][kMaxGt]
  double* gbox = iou + kMaxDet * kMaxGt;                              // [5][kMaxGt]: x0, y0, x1, y1, w * h

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, nthreads = blockDim.x;
  const int d0 = dt_rows[img], g0 = gt_rows[img];
  int nd = dt_rows[img + 1] - d0, ng = gt_rows[img + 1] - g0;
  const bool refused = nd < 0 || nd > kMaxDet || ng < 0 || ng > kMaxGt;
  if (refused) nd = ng = 0;                                           // nothing is read; the outputs become -1 / 0 / 0
  if (tid == 0) status[img] = refused ? 1 : 0;
  const double* dti = dt + (size_t)d0 * 5;
  const double* gti = gt + (size_t)g0 * 5;

  // ---- 1. IoU matrix (cocoeval._iou_xywh, term by term)
  for (int j = tid; j < ng; j += nthreads) {
    const double x = gti[j * 5], y = gti[j * 5 + 1], w = gti[j * 5 + 2], h = gti[j * 5 + 3];
    gbox[j] = x; gbox[kMaxGt + j] = y; gbox[2 * kMaxGt + j] = x + w; gbox[3 * kMaxGt + j] = y + h; gbox[4 * kMaxGt + j] = w * h;
  }
  __syncthreads();
  for (int e = tid; e < nd * kMaxGt; e += nthreads) {
    const int d = e >> 7, j = e & (kMaxGt - 1);
    if (j >= ng) continue;
    const double x = dti[d * 5], y = dti[d * 5 + 1], w = dti[d * 5 + 2], h = dti[d * 5 + 3];
    const double dx1 = x + w, dy1 = y + h;
    const double iw = fmax(fmin(dx1, gbox[2 * kMaxGt + j]) - fmax(x, gbox[j]), 0.0);
    const double ih = fmax(fmin(dy1, gbox[3 * kMaxGt + j]) - fmax(y, gbox[kMaxGt + j]), 0.0);
    const double inter = iw * ih;
    const double uni = (w * h + gbox[4 * kMaxGt + j]) - inter;
    iou[e] = uni > 0.0 ? inter / uni : 0.0;
  }
  __syncthreads();

  // ---- 2. matching
  const bool has0 = lane < ng, has1 = lane + 64 < ng;
  const double ga0 = has0 ? gti[lane * 5 + 4] : 0.0, ga1 = has1 ? gti[(lane + 64) * 5 + 4] : 0.0;       // the ANNOTATION's area
  const double da0 = lane < nd ? dti[lane * 5 + 2] * dti[lane * 5 + 3] : 0.0;
  const double da1 = lane + 64 < nd ? dti[(lane + 64) * 5 + 2] * dti[(lane + 64) * 5 + 3] : 0.0;
  for (int t = tid >> 6; t < T; t += nthreads >> 6) {
    const double start = p.start[t];
    for (int a = 0; a < A; ++a) {
      const double lo = p.a0[a], hi = p.a1[a];
      const bool in0 = has0 && ga0 >= lo && ga0 <= hi, in1 = has1 && ga1 >= lo && ga1 <= hi;
      if (t == 0) {
        const int n = __popcll(__ballot(in0)) + __popcll(__ballot(in1));
        if (lane == 0) n_gt_counted[(size_t)img * A + a] = n;
      }
      const int code0 = ((in0 ? 2 : 1) << 8) | lane, code1 = ((in1 ? 2 : 1) << 8) | (lane + 64);
      bool free0 = has0, free1 = has1;
      const size_t out = (((size_t)img * A + a) * T + t) * kMaxDet;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        int row = -1, row_ignored = 0;                                // of detection half * 64 + lane
        const int dend = min(nd - half * 64, 64);
        for (int dd = 0; dd < dend; ++dd) {
          const double* r = iou + (half * 64 + dd) * kMaxGt;
          const double v0 = r[lane], v1 = r[lane + 64];               // (rows >= ng are never read as candidates)
          const bool c0 = free0 && v0 >= start, c1 = free1 && v1 >= start;
          if (__ballot(c0 || c1) == 0ull) continue;
          double bi = 0.0;
          int bc = 0;
          if (c0) { bi = v0; bc = code0; }
          if (c1 && better(v1, code1, bi, bc)) { bi = v1; bc = code1; }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const double oi = __shfl_xor(bi, o, 64);
            const int oc = __shfl_xor(bc, o, 64);
            if (better(oi, oc, bi, bc)) { bi = oi; bc = oc; }
          }
          const int win = bc & 255;
          if (win == lane) free0 = false;
          if (win == lane + 64) free1 = false;
          if (lane == dd) { row = win; row_ignored = (bc >> 8) == 1; }
        }
        // ---- 3. outputs
        const int slot = half * 64 + lane;
        if (slot < kMaxDet) {
          int ig = 0;
          if (slot < nd) {
            const double da = half ? da1 : da0;
            ig = row >= 0 ? row_ignored : (da < lo || da > hi);
          }
          match[out + slot] = (int16_t)row;
          ignore[out + slot] = (uint8_t)ig;
        }
      }
    }
  }
}

}  // namespace

extern "C" int mbx_coco_match(const double* dt, const int32_t* dt_rows, const double* gt, const int32_t* gt_rows, int I,
                              const double* iou_thrs, int T, const double* area_rng, int A, int16_t* match,
                              uint8_t* ignore, int32_t* n_gt_counted, int32_t* status, mbx_stream_t stream) {
  if (!dt || !dt_rows || !gt || !gt_rows || !iou_thrs || !area_rng || !match || !ignore || !n_gt_counted || !status)
    return MBX_ERR_INVALID_ARG;
  if (I < 0 || T < 1 || T > kMaxT || A < 1 || A > kMaxA) return MBX_ERR_INVALID_ARG;
  if (I == 0) return MBX_OK;
  CocoParams p = {};
  for (int t = 0; t < T; ++t) p.start[t] = iou_thrs[t] <= 1 - 1e-10 ? iou_thrs[t] : 1 - 1e-10;     // min(t, 1 - 1e-10)
  for (int a = 0; a < A; ++a) { p.a0[a] = area_rng[2 * a]; p.a1[a] = area_rng[2 * a + 1]; }
  const size_t lds = ((size_t)kMaxDet * kMaxGt + 5 * kMaxGt) * sizeof(double);
  MBX_ENTER();
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(coco_match_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess) return MBX_ERR_LAUNCH;
  hipLaunchKernelGGL(coco_match_kernel, dim3(I), dim3(64 * T), lds, mbx_s(stream), dt, dt_rows, gt, gt_rows, T, A, p, match,
                     ignore, n_gt_counted, status);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}
