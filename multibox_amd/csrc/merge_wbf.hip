// libmbx: weighted boxes fusion in the per-image merge of multi-crop detections (Solovyev, Wang, Gabruseva 2021; the
// contract is in include/mbx.h).  Where merge.hip's kernels SELECT among an image's candidates, this one clusters them
// against the running fused box of each cluster and reports the clusters.  Built with -ffp-contract=off: every float64
// operation of the definition is rounded once, in the stated order, so all outputs are exact against a numpy restatement.
#include "boxes.h"

namespace {

constexpr int kWbfThreads = 1024;
constexpr int kWbfWaves = kWbfThreads / 64;
constexpr int kMaxCand = MBX_MERGE_MAX_CANDIDATES;
constexpr int kMergeMaxDet = 640;                      // the family's limit (merge.hip)
// LDS plan: keys [16384] u64 (128 KiB), the whole state of the first kWbfLds clusters -- F (4), A, S, X (4) as [10][kWbfLds]
// f64, then n as [kWbfLds] i32 (26.25 KiB) -- and the boxes of one chunk of kWbfChunk candidates (4 KiB; step 1 keeps its
// row counts there).  Clusters from kWbfLds on keep all of it in the workspace.
constexpr int kWbfLds = 320;
constexpr int kWbfChunk = 128;
static_assert(kWbfChunk * sizeof(Box) >= kWbfThreads * sizeof(int), "the row counts of step 1 fit in the chunk's room");
// The workspace, per slot of the input (an image's cluster k sits at the image's first slot + k; it has at most as many
// clusters as slots): arrays [R * k_max] of float64 -- F (4), A, S, X (4) -- then of int32 -- n, first.
constexpr int kWsDoubles = 10, kWsInts = 2;
constexpr size_t kWbfLdsBytes = (size_t)kMaxCand * sizeof(unsigned long long) +
                                (size_t)kWbfLds * (kWsDoubles * sizeof(double) + sizeof(int32_t)) + (size_t)kWbfChunk * sizeof(Box);

// What a wavefront found for the candidate of this step: its largest IoU with a cluster, and which (0xffffffff: none).
struct WbfBest { double o; unsigned k; unsigned pad; };

// The larger IoU, of bit-equal ones the lower cluster number.  An IoU here is > 0 or the 0.0 of "none".
__device__ __forceinline__ bool wbf_better(double oa, unsigned ka, double ob, unsigned kb) {
  return oa > ob || (oa == ob && ka < kb);
}

// The state of the image's clusters: the first kWbfLds in LDS, the rest in the workspace.  at(k, fn) hands fn the address
// of cluster k's first float64 (F.x1), the distance s between its ten float64 arrays (F.x1 F.y1 F.x2 F.y2 A S X0..X3) and
// the address of its member count, each in the memory the cluster lives in.
struct WbfClusters {
  double* lds;                                         // [kWsDoubles][kWbfLds]
  int32_t* lds_n;                                      // [kWbfLds]
  double* ws;                                          // the image's first slot of the workspace's first array
  int32_t* ws_n;
  long long stride;                                    // from one workspace array to the next: R * k_max
  template <typename Fn>
  __device__ __forceinline__ void at(int k, Fn&& fn) const {
    if (k < kWbfLds) fn(lds + k, (long long)kWbfLds, lds_n + k);
    else fn(ws + k, stride, ws_n + k);
  }
  __device__ __forceinline__ void load(int k, Box& f, double& a) const {
    at(k, [&](const double* p, long long s, const int32_t*) { f.x1 = p[0]; f.y1 = p[s]; f.x2 = p[2 * s]; f.y2 = p[3 * s]; a = p[4 * s]; });
  }
};

// One workgroup of kWbfThreads per image.
//   1. the sorted candidate list, as merge_kernel (boxes.h: sorted_candidate_keys).
//   2. the walk, one candidate per step.  Cluster k belongs to thread k % kWbfThreads for good: that thread alone reads and
//      writes its F, A, S, X and n (LDS or workspace), so a step needs ONE barrier -- every thread takes the IoU of the
//      candidate with its clusters (a cluster the candidate does not intersect has IoU 0 and cannot be joined:
//      iou_threshold >= 0 and the test is strict), the wave's best goes to the wave's slot, barrier,
//      every thread reads the kWbfWaves slots and knows the decision (the slots alternate between two sets, so the next
//      step's writes need no second barrier); the owner of the joined or founded cluster updates it.  The candidates'
//      boxes are staged kWbfChunk at a time; their scores come back out of the sort keys.  The walk skips the NaN / +inf
//      head of the list and ends at the first candidate behind it that is not live: nobody after it is.
//   3. cluster scores -> keys (score image << 32 | ~cluster number), the same LDS sort, the first max_det go out.
// The walk is sequential and every cluster has one owner, so the outputs are a function of the image's rows only.
__global__ void __launch_bounds__(kWbfThreads)
wbf_merge_kernel(const double* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ count,
                 const int32_t* __restrict__ image_rows, int R, int k_max, int max_det, int conf_type, double thr,
                 double min_score, int views, double* __restrict__ out_boxes, float* __restrict__ out_scores,
                 int32_t* __restrict__ out_src, int32_t* __restrict__ out_count, int32_t* __restrict__ out_status,
                 int32_t* __restrict__ out_votes, double* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wbf_lds[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(wbf_lds);          // [kMaxCand]
  double* state = reinterpret_cast<double*>(keys + kMaxCand);                         // [kWsDoubles][kWbfLds]
  Box* chunk = reinterpret_cast<Box*>(state + kWsDoubles * kWbfLds);                  // [kWbfChunk]
  int32_t* state_n = reinterpret_cast<int32_t*>(chunk + kWbfChunk);                   // [kWbfLds]
  int* tile_cnt = reinterpret_cast<int*>(chunk);                                      // [kWbfThreads], step 1 only
  __shared__ int wave_tot[kWbfWaves];
  __shared__ WbfBest wave_best[2][kWbfWaves];

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = image_rows[img], r1 = image_rows[img + 1];
  const bool bad_rows = r0 < 0 || r1 < r0 || r1 > R;           // rows the workspace has no room for: nothing is read or written
  const long long base = (long long)r0 * k_max;                 // flat index of the image's first slot
  const long long stride = (long long)R * k_max;
  double* ob = out_boxes + (size_t)img * max_det * 4;
  float* os = out_scores + (size_t)img * max_det;
  int32_t* oi = out_src + (size_t)img * max_det;
  int32_t* ov = out_votes + (size_t)img * max_det;

  // ---- 1. the sorted candidate list
  bool too_many = false;
  int total = 0;
  if (!bad_rows) total = sorted_candidate_keys<kWbfThreads>(scores, count, r0, r1, k_max, keys, tile_cnt, wave_tot, &too_many);

  int32_t* ws_n = reinterpret_cast<int32_t*>(ws + kWsDoubles * stride) + base;
  int32_t* first = ws_n + stride;                               // (written once per cluster and read at the end: workspace only)
  const WbfClusters clusters = {state, state_n, ws + base, ws_n, stride};
  int nc = 0;
  if (total > 0) {
    // ---- 2. the walk
    int step = 0;
    bool done = false;
    for (int c0 = 0; c0 < total && !done; c0 += kWbfChunk) {
      __syncthreads();                                           // the previous chunk's boxes (or the row counts) have been read
      if (tid < kWbfChunk && c0 + tid < total) {
        const unsigned rel = ~(unsigned)(keys[c0 + tid] & 0xffffffffull);
        const double* p = boxes + (size_t)(base + rel) * 4;
        chunk[tid].x1 = p[0]; chunk[tid].y1 = p[1]; chunk[tid].x2 = p[2]; chunk[tid].y2 = p[3];
      }
      __syncthreads();
      const int cend = min(kWbfChunk, total - c0);
      for (int j = 0; j < cend; ++j) {                           // (everything that steers this loop is uniform)
        const unsigned long long key = keys[c0 + j];
        const double t = (double)score_from_order_key((unsigned)(key >> 32));
        if (!(t < INFINITY)) continue;                           // the head of the list: NaN, +inf
        if (!(t > min_score)) { done = true; break; }
        const Box x = chunk[j];
        const double a = box_area(x);
        double bo = 0.0;
        unsigned bk = 0xffffffffu;
        for (int k = tid; k < nc; k += kWbfThreads) {
          Box f;
          double af;
          clusters.load(k, f, af);
          const double iw = fmin(f.x2, x.x2) - fmax(f.x1, x.x1), ih = fmin(f.y2, x.y2) - fmax(f.y1, x.y1);
          if (!(iw > 0.0 && ih > 0.0)) continue;                 // IoU exactly 0
          const double o = iou_corners(f, x, af, a);
          if (o > bo) { bo = o; bk = (unsigned)k; }              // ascending k: of equal IoUs the first stays
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
          const double oo = __shfl_xor(bo, s, 64);
          const unsigned ok = __shfl_xor(bk, s, 64);
          if (wbf_better(oo, ok, bo, bk)) { bo = oo; bk = ok; }
        }
        WbfBest* slots = wave_best[step & 1];
        ++step;
        if (lane == 0) { slots[wave].o = bo; slots[wave].k = bk; }
        __syncthreads();
        double mo = slots[0].o;
        unsigned m = slots[0].k;
#pragma unroll
        for (int w = 1; w < kWbfWaves; ++w) {
          const double oo = slots[w].o;
          const unsigned ok = slots[w].k;
          if (wbf_better(oo, ok, mo, m)) { mo = oo; m = ok; }
        }
        if (mo > thr) {                                          // joins cluster m
          if ((int)(m & (kWbfThreads - 1)) == tid) {
            clusters.at((int)m, [&](double* p, long long s, int32_t* n) {
              const double S = p[5 * s] + t;
              const double X0 = p[6 * s] + t * x.x1, X1 = p[7 * s] + t * x.y1, X2 = p[8 * s] + t * x.x2, X3 = p[9 * s] + t * x.y2;
              p[5 * s] = S; p[6 * s] = X0; p[7 * s] = X1; p[8 * s] = X2; p[9 * s] = X3;
              *n += 1;
              Box f;
              f.x1 = X0 / S; f.y1 = X1 / S; f.x2 = X2 / S; f.y2 = X3 / S;
              p[0] = f.x1; p[s] = f.y1; p[2 * s] = f.x2; p[3 * s] = f.y2; p[4 * s] = box_area(f);
            });
          }
        } else {                                                 // founds cluster nc
          if ((nc & (kWbfThreads - 1)) == tid) {
            clusters.at(nc, [&](double* p, long long s, int32_t* n) {
              p[0] = x.x1; p[s] = x.y1; p[2 * s] = x.x2; p[3 * s] = x.y2; p[4 * s] = a;
              p[5 * s] = t; p[6 * s] = t * x.x1; p[7 * s] = t * x.y1; p[8 * s] = t * x.x2; p[9 * s] = t * x.y2;
              *n = 1;
            });
            first[nc] = (int32_t)(base + (long long)(~(unsigned)(key & 0xffffffffull)));
          }
          ++nc;
        }
      }
    }
    __syncthreads();                                             // the walk's keys have been read; every cluster is written

    // ---- 3. the clusters' scores and their order
    int N = 64;
    while (N < nc) N <<= 1;
    for (int k = tid; k < N; k += kWbfThreads) {
      unsigned long long key = 0ull;                             // below every cluster's key
      if (k < nc) {
        int n = 0;
        double S = 0.0;
        clusters.at(k, [&](const double* p, long long s, const int32_t* pn) { S = p[5 * s]; n = *pn; });
        double q = conf_type == MBX_WBF_AVG ? S / (double)n : (double)scores[first[k]];
        if (views > 1) q = (q * (double)min(n, views)) / (double)views;
        key = ((unsigned long long)score_order_key((float)q) << 32) | (unsigned long long)(~(unsigned)k);
      }
      keys[k] = key;
    }
    __syncthreads();
    lds_bitonic_sort_desc(keys, N, tid, kWbfThreads);
  }

  const int nk = min(nc, max_det);
  if (tid == 0) { out_count[img] = nk; out_status[img] = bad_rows ? 2 : too_many ? 1 : 0; }
  for (int t = tid; t < max_det; t += kWbfThreads) {
    if (t < nk) {
      const unsigned long long key = keys[t];
      const int k = (int)(~(unsigned)(key & 0xffffffffull));
      Box f;
      double af;
      clusters.load(k, f, af);
      ob[t * 4] = f.x1; ob[t * 4 + 1] = f.y1; ob[t * 4 + 2] = f.x2; ob[t * 4 + 3] = f.y2;
      os[t] = score_from_order_key((unsigned)(key >> 32));       // (a cluster's score is > 0 and no NaN: the key keeps it)
      oi[t] = first[k];
      clusters.at(k, [&](const double*, long long, const int32_t* pn) { ov[t] = *pn; });
    } else {
      ob[t * 4] = ob[t * 4 + 1] = ob[t * 4 + 2] = ob[t * 4 + 3] = 0.0;
      os[t] = 0.f;
      oi[t] = -1;
      ov[t] = 0;
    }
  }
}

}  // namespace

extern "C" size_t mbx_merge_wbf_workspace(int R, int k_max) {
  if (R <= 0 || k_max <= 0) return 0;
  const size_t slots = (size_t)R * (size_t)k_max;
  if (slots > 0x7fffffffull) return 0;                          // flat indices are int32
  return slots * (kWsDoubles * sizeof(double) + kWsInts * sizeof(int32_t));
}

extern "C" int mbx_merge_detections_wbf(const double* boxes, const float* scores, const int32_t* count,
                                        const int32_t* image_rows, int R, int I, int k_max, int max_det, int conf_type,
                                        double iou_threshold, double min_score, int expected_views, double* out_boxes,
                                        float* out_scores, int32_t* out_src, int32_t* out_count, int32_t* out_status,
                                        int32_t* out_votes, void* workspace, size_t workspace_bytes, mbx_stream_t stream) {
  if (!boxes || !scores || !count || !image_rows || !out_boxes || !out_scores || !out_src || !out_count || !out_status)
    return MBX_ERR_INVALID_ARG;
  if (!out_votes || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return MBX_ERR_INVALID_ARG;
  if (I < 0 || k_max <= 0 || max_det <= 0) return MBX_ERR_INVALID_ARG;
  if (conf_type != MBX_WBF_AVG && conf_type != MBX_WBF_MAX) return MBX_ERR_INVALID_ARG;
  if (!(iou_threshold >= 0.0 && iou_threshold <= 1.0)) return MBX_ERR_INVALID_ARG;                 // a NaN too
  if (!(min_score >= 0.0 && min_score < INFINITY)) return MBX_ERR_INVALID_ARG;                     // a NaN too
  if (expected_views < 1) return MBX_ERR_INVALID_ARG;
  const size_t need = mbx_merge_wbf_workspace(R, k_max);
  if (need == 0 || workspace_bytes < need) return MBX_ERR_INVALID_ARG;
  if (max_det > kMergeMaxDet) return MBX_ERR_UNSUPPORTED;
  if (I == 0) return MBX_OK;
  const size_t lds = kWbfLdsBytes;
  MBX_ENTER();
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(wbf_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess) return MBX_ERR_LAUNCH;
  hipLaunchKernelGGL(wbf_merge_kernel, dim3(I), dim3(kWbfThreads), lds, mbx_s(stream), boxes, scores, count, image_rows, R,
                     k_max, max_det, conf_type, iou_threshold, min_score, expected_views, out_boxes, out_scores, out_src,
                     out_count, out_status, out_votes, static_cast<double*>(workspace));
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}
