// libmbx: the training side of the box arithmetic -- prior decode, bipartite matching, threshold / ATSS matching, loss fwd+bwd
// (plain, with hard-negative mining, focal, with a choice of location term).  The detection side is postproc.hip.
// HBM/latency-bound integer+float kernels; one workgroup per image,
// wave64 shuffle reductions.  Built with -ffp-contract=off: the float32 cost arithmetic
// must keep the reference's rounding sequence (loss.py:21-35).
#include "boxes.h"
#include "wave_select.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// ------------------------------------------------------------------ decode + conf
__global__ void __launch_bounds__(kThreads)
decode_conf_kernel(const float4* __restrict__ raw, const float* __restrict__ logits,
                   const float4* __restrict__ priors, int total, int P, float eps_add,
                   float4* __restrict__ decoded, float* __restrict__ conf) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    if (decoded) {
      const float4 r = raw[i], p = priors[i % P];
      decoded[i] = make_float4(__fadd_rn(r.x, p.x), __fadd_rn(r.y, p.y), __fadd_rn(r.z, p.z), __fadd_rn(r.w, p.w));
    }
    if (conf) {
      const float s = 1.0f / (1.0f + expf(-logits[i]));     // model.py:322
      conf[i] = __fadd_rn(s, eps_add);                      // loss.py:74
    }
  }
}

// ----------------------------------------------------------------------- matching
// cost of (prediction, gt) in the reference's float32 operation order, loss.py:35:
//   (alpha/2) * norm(l - g)**2 - log c + log(1-c)          (left to right)
__device__ __forceinline__ double match_cost(const float4 l, const float4 g, float half_alpha,
                                             float lc, float l1c) {
  const float d0 = __fsub_rn(l.x, g.x), d1 = __fsub_rn(l.y, g.y), d2 = __fsub_rn(l.z, g.z), d3 = __fsub_rn(l.w, g.w);
  const float ss = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)), __fmul_rn(d3, d3));
  const float nrm = __fsqrt_rn(ss);
  float t = __fmul_rn(half_alpha, __fmul_rn(nrm, nrm));
  t = __fsub_rn(t, lc);
  t = __fadd_rn(t, l1c);
  return (double)t;
}

struct Cand {
  double val;
  int j;      // column (prediction); -1 = none
  int free_;  // 1 if the column is unassigned
};

__device__ __forceinline__ bool cand_better(const Cand& a, const Cand& b) {
  if (a.j < 0) return false;
  if (b.j < 0) return true;
  if (a.val < b.val) return true;
  if (a.val > b.val) return false;
  if (a.free_ != b.free_) return a.free_ > b.free_;   // scipy prefers an unassigned column among equals
  return a.j < b.j;
}

__device__ __forceinline__ Cand cand_shfl_xor(const Cand& c, int o) {
  Cand r;
  r.val = __shfl_xor(c.val, o, 64);
  r.j = __shfl_xor(c.j, o, 64);
  r.free_ = __shfl_xor(c.free_, o, 64);
  return r;
}

// One workgroup per image.  Rectangular LSAP on the transposed problem (rows = gt boxes,
// columns = predictions), shortest augmenting path with float64 duals, as scipy's
// linear_sum_assignment (loss.py:40).  LDS: 36 B per prediction + 16 B per gt.  256 threads per image up to 1536 predictions,
// 512 beyond (round 4, tools/match_bench.py on random boxes: P = 3199 / G = 100 812 -> 589 us; P = 646 is fastest at 256:
// 47 us against 84 with one wave -- the column scan, not the barriers, is what an iteration costs; staging the locations in
// LDS changed nothing: they are L1 hits).
__global__ void __launch_bounds__(1024)
match_kernel(const float4* __restrict__ decoded, const float* __restrict__ conf,
             const float4* __restrict__ gt, const int* __restrict__ n_gt, float alpha, int P, int G,
             int* __restrict__ match, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* v = reinterpret_cast<double*>(smem);            // [P] column duals
  double* spc = v + P;                                    // [P] shortest path costs
  double* u = spc + P;                                    // [G] row duals
  float2* lcl = reinterpret_cast<float2*>(u + G);         // [P] {log c, log(1-c)}
  int* path = reinterpret_cast<int*>(lcl + P);            // [P]
  int* row4col = path + P;                                // [P]
  int* SC = row4col + P;                                  // [P]
  int* col4row = SC + P;                                  // [G]
  int* SR = col4row + G;                                  // [G]
  __shared__ Cand wave_best[16];
  __shared__ int sh_i, sh_sink, sh_bad;
  __shared__ double sh_min;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int nt = (int)blockDim.x, nwaves = nt >> 6;       // 256 or 512 threads (mbx_match)
  const float4* loc = decoded + (size_t)b * P;
  const float* cf = conf + (size_t)b * P;
  const float4* g = gt + (size_t)b * G;
  int* mt = match + (size_t)b * P;
  const int n = n_gt[b];
  const float half_alpha = alpha / 2.0f;

  if (tid == 0) sh_bad = 0;
  __syncthreads();
  int bad = 0;
  for (int j = tid; j < P; j += nt) {
    mt[j] = -1;
    const float c = cf[j];
    const float lc = logf(c);                              // loss.py:21
    float w = __fsub_rn(1.0f, c);                          // loss.py:22-24
    if (w > 1.0f) w = 1.0f;
    if (w <= 0.0f) w = 1e-10f;
    const float l1c = logf(w);                             // loss.py:25
    lcl[j] = make_float2(lc, l1c);
    v[j] = 0.0;
    row4col[j] = -1;
    const float4 l = loc[j];
    if (!(isfinite(lc) && isfinite(l1c) && isfinite(l.x) && isfinite(l.y) && isfinite(l.z) && isfinite(l.w))) bad = 1;
  }
  for (int i = tid; i < G; i += nt) {
    u[i] = 0.0;
    col4row[i] = -1;
    if (i < n) {
      const float4 q = g[i];
      if (!(isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && isfinite(q.w))) bad = 1;
    }
  }
  if (bad) sh_bad = 1;
  __syncthreads();
  if (n <= 0) { if (tid == 0) status[b] = 0; return; }
  if (n > P || n > G) { if (tid == 0) status[b] = 1; return; }
  if (sh_bad) { if (tid == 0) status[b] = 2; return; }

  for (int cur = 0; cur < n; ++cur) {
    for (int j = tid; j < P; j += nt) { spc[j] = INFINITY; SC[j] = 0; }
    for (int i = tid; i < n; i += nt) SR[i] = 0;
    if (tid == 0) { sh_i = cur; sh_sink = -1; sh_min = 0.0; }
    __syncthreads();
    while (true) {
      const int i = sh_i;
      const double min_val = sh_min;
      const float4 gi = g[i];
      const double ui = u[i];
      Cand best; best.val = INFINITY; best.j = -1; best.free_ = 0;
      for (int j = tid; j < P; j += nt) {
        if (SC[j]) continue;
        const float2 ll = lcl[j];
        // scipy: r = minVal + cost[i][j] - u[i] - v[j]
        const double r = ((min_val + match_cost(loc[j], gi, half_alpha, ll.x, ll.y)) - ui) - v[j];
        double s = spc[j];
        if (r < s) { path[j] = i; spc[j] = r; s = r; }
        Cand c; c.val = s; c.j = j; c.free_ = row4col[j] < 0;
        if (cand_better(c, best)) best = c;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const Cand other = cand_shfl_xor(best, o);
        if (cand_better(other, best)) best = other;
      }
      if ((tid & 63) == 0) wave_best[tid >> 6] = best;
      __syncthreads();
      if (tid == 0) {
        Cand bb = wave_best[0];
        for (int w = 1; w < nwaves; ++w) if (cand_better(wave_best[w], bb)) bb = wave_best[w];
        if (bb.j < 0 || !(bb.val < INFINITY)) {
          sh_sink = -2;                                    // infeasible
        } else {
          sh_min = bb.val;
          SC[bb.j] = 1;
          SR[i] = 1;
          const int r4c = row4col[bb.j];
          if (r4c < 0) sh_sink = bb.j; else sh_i = r4c;
        }
      }
      __syncthreads();
      if (sh_sink != -1) break;
    }
    const int sink = sh_sink;
    if (sink == -2) { if (tid == 0) status[b] = 2; return; }
    const double min_val = sh_min;
    // dual updates
    for (int i = tid; i < n; i += nt) {
      if (i == cur) u[i] += min_val;
      else if (SR[i]) u[i] += min_val - spc[col4row[i]];
    }
    for (int j = tid; j < P; j += nt)
      if (SC[j]) v[j] -= min_val - spc[j];
    __syncthreads();
    if (tid == 0) {                                        // augment along the path
      int j = sink;
      while (true) {
        const int i = path[j];
        row4col[j] = i;
        const int t = col4row[i];
        col4row[i] = j;
        j = t;
        if (i == cur) break;
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += nt) mt[col4row[i]] = i;
  if (tid == 0) status[b] = 0;
}

// ------------------------------------------------------------- threshold matching
// SSD's second matching step behind match_kernel (mbx_match_extend, mbx.h): every prior the bipartite match left free goes
// to the box it overlaps most, if that IoU is over `thr`.  One workgroup per image, blockDim.x a multiple of 64 (P rounded
// up, at most 1024).  The image's n boxes and their areas are widened to float64 into LDS once (40 B a box); a thread keeps
// its prior's box and area in registers and walks the staged boxes, every lane reading the same LDS address (a broadcast).
// The IoU is iou_corners' (boxes.h), term by term, with the prior as its first box; a pair that does not overlap has IoU 0,
// which is never over a threshold > 0, so the float64 division is done for overlapping pairs only.  `best` starts at the
// threshold and moves on a strictly larger IoU: the lowest j among the largest, and only where that is over the threshold.
__global__ void __launch_bounds__(1024)
match_extend_kernel(const float4* __restrict__ priors, const float4* __restrict__ gt, const int* __restrict__ n_gt,
                    const int* __restrict__ status, double thr, int P, int G, int* __restrict__ match,
                    int* __restrict__ n_extra) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  StagedBox* boxes = reinterpret_cast<StagedBox*>(smem);      // [n]
  __shared__ int added_waves[16];
  const int b = blockIdx.x, tid = threadIdx.x, nt = (int)blockDim.x;
  const int n = n_gt[b];
  if (status[b] != 0 || n <= 0 || n > G) {                    // skipped: the row stays as it is (n > G never has status 0)
    if (tid == 0 && n_extra) n_extra[b] = 0;
    return;
  }
  for (int j = tid; j < n; j += nt) {
    const float4 q = gt[(size_t)b * G + j];
    StagedBox s;
    s.box = {(double)q.x, (double)q.y, (double)q.z, (double)q.w};
    s.area = box_area(s.box);
    boxes[j] = s;
  }
  __syncthreads();
  int* mt = match + (size_t)b * P;
  int added = 0;
  for (int p = tid; p < P; p += nt) {
    if (mt[p] >= 0) continue;                                 // mbx_match's choice stands
    const float4 q = priors[p];
    const Box e = {(double)q.x, (double)q.y, (double)q.z, (double)q.w};
    const double area_e = box_area(e);
    double best = thr;
    int best_j = -1;
    for (int j = 0; j < n; ++j) {
      const Box g = boxes[j].box;
      const double iw = fmin(e.x2, g.x2) - fmax(e.x1, g.x1), ih = fmin(e.y2, g.y2) - fmax(e.y1, g.y1);
      if (iw > 0.0 && ih > 0.0) {
        const double inter = iw * ih;
        const double uni = area_e + boxes[j].area - inter;
        const double iou = uni > 0.0 ? inter / uni : 0.0;
        if (iou > best) { best = iou; best_j = j; }
      }
    }
    if (best_j >= 0) { mt[p] = best_j; ++added; }
  }
  if (!n_extra) return;
  added = wave_sum(added);
  if ((tid & 63) == 0) added_waves[tid >> 6] = added;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < (nt >> 6); ++w) total += added_waves[w];
    n_extra[b] = total;
  }
}

// -------------------------------------------------------------------- ignore band
// The third state of a prior, behind match_kernel and behind match_extend_kernel / match_atss_kernel when one of them runs
// (mbx_match_ignore, mbx.h has the rule): a prior that is still free (match == MBX_MATCH_FREE exactly) and overlaps some box
// of its image by at least `thr` becomes MBX_MATCH_IGNORED, which the loss of mbx_loss_fwd_bwd_ignore leaves out.  The frame
// is match_extend_kernel's: one workgroup per image, blockDim.x a multiple of 64, the image's n boxes and their areas
// widened to float64 into LDS once (StagedBox, 40 B a box), a thread keeps its box and area in registers and walks the staged
// boxes (a broadcast read).  The IoU is match_extend_kernel's, line by line -- the same float64 inter / uni, so that `>= thr`
// here and `> thr` there split the free priors without a gap or an overlap -- but there is no argmax: the walk stops at the
// first box that reaches the threshold.  A pair that does not overlap has IoU 0, never at a threshold > 0; a NaN fails
// every comparison on the way and passes nothing.  `image_stride` is 0 (the priors, shared by all images) or P (a row of
// boxes per image: the decoded predictions, taken as they are).
__global__ void __launch_bounds__(1024)
match_ignore_kernel(const float4* __restrict__ boxes_in, size_t image_stride, const float4* __restrict__ gt,
                    const int* __restrict__ n_gt, const int* __restrict__ status, double thr, int P, int G,
                    int* __restrict__ match, int* __restrict__ n_ignored) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  StagedBox* boxes = reinterpret_cast<StagedBox*>(smem);      // [n]
  __shared__ int ignored_waves[16];
  const int b = blockIdx.x, tid = threadIdx.x, nt = (int)blockDim.x;
  const int n = n_gt[b];
  if (status[b] != 0 || n <= 0 || n > G) {                    // skipped: the row stays as it is (mbx_match_extend's rule)
    if (tid == 0 && n_ignored) n_ignored[b] = 0;
    return;
  }
  for (int j = tid; j < n; j += nt) {
    const float4 q = gt[(size_t)b * G + j];
    StagedBox s;
    s.box = {(double)q.x, (double)q.y, (double)q.z, (double)q.w};
    s.area = box_area(s.box);
    boxes[j] = s;
  }
  __syncthreads();
  int* mt = match + (size_t)b * P;
  const float4* own = boxes_in + (size_t)b * image_stride;
  int ignored = 0;
  for (int p = tid; p < P; p += nt) {
    if (mt[p] != MBX_MATCH_FREE) continue;                    // a positive keeps its box, -2 and below stay: a second call is a no-op
    const float4 q = own[p];
    const Box e = {(double)q.x, (double)q.y, (double)q.z, (double)q.w};
    const double area_e = box_area(e);
    bool hit = false;
    for (int j = 0; j < n && !hit; ++j) {
      const Box g = boxes[j].box;
      const double iw = fmin(e.x2, g.x2) - fmax(e.x1, g.x1), ih = fmin(e.y2, g.y2) - fmax(e.y1, g.y1);
      if (iw > 0.0 && ih > 0.0) {
        const double inter = iw * ih;
        const double uni = area_e + boxes[j].area - inter;
        const double iou = uni > 0.0 ? inter / uni : 0.0;
        hit = iou >= thr;
      }
    }
    if (hit) { mt[p] = MBX_MATCH_IGNORED; ++ignored; }
  }
  if (!n_ignored) return;
  ignored = wave_sum(ignored);
  if ((tid & 63) == 0) ignored_waves[tid >> 6] = ignored;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < (nt >> 6); ++w) total += ignored_waves[w];
    n_ignored[b] = total;
  }
}

// ------------------------------------------------------------------- ATSS matching
// Adaptive Training Sample Selection behind match_kernel (mbx_match_atss, mbx.h has the rule): per box the `topk` priors
// nearest to its centre on every level are its candidates, its threshold is the mean plus the sample standard deviation of
// their IoUs, and a candidate at or over it whose centre lies inside the box is a positive; a free prior goes to the
// positive box of the largest IoU, the lowest j among equals.  One workgroup of `nw` wavefronts per image.
//   LDS: claim[P] (8 B: the largest IoU bit pattern a positive box has claimed the prior with) | boxes[G] (StagedBox) |
//        iou[nw][m] (8 B, a wavefront's scratch) | cand[G][m] (2 B: a box's candidates, then its positives).
//   Pass 1, a wavefront per box j = wave, wave + nw, ...: per level it finds the cut -- the min(topk, size)-th smallest
//     (distance key, index) pair (wave_select.h, shared with match_tal.hip).  A strided scan leaves in every lane's registers the kKeepPairs smallest of its own pairs,
//     in order; each round a 64-lane min over the heads of the lists takes the next pair.  Only when a lane has handed out
//     its whole list and had more to offer does the wavefront scan again, for the pairs over the last one taken: with topk
//     9 and the priors of one cell on neighbouring lanes that is one scan a level, not nine (the launch at P = 3199,
//     G = 100: 1 159 us with a scan a round, 539 with the lists, 490 with the rounds' minimum on DPP moves, 432 as it is;
//     profiles/match_atss_bench.txt).  Nothing is marked or stored; a level no larger than topk is taken whole without a
//     round.  One more scan in 64-prior chunks writes the priors at or under the cut in ascending index (ballot + prefix
//     count); their IoUs follow, m divisions and not one per prior of the level.  Every lane then runs the two serial sums
//     over the m IoUs (the same LDS address for all: a broadcast), so the threshold needs no hand-off.
//     A positive whose prior mbx_match left free raises claim[p] with a 64-bit unsigned LDS
//     max: IoUs are >= 0, so their bit patterns order like the values and the result does not depend on who came first.
//     A candidate that is no such positive is struck from cand.
//   Pass 2, every thread over the G x m entries: a positive whose IoU (the same function on the same inputs: the same
//     bits) equals claim[p] lowers match[b,p] with an unsigned integer min -- a free entry is negative, as unsigned above
//     every j -- so the lowest j among the largest IoUs stays; whoever finds the entry still negative counts the prior.
// Lanes of one wavefront hand LDS values to each other without a workgroup barrier (the wavefronts run different numbers
// of boxes): wave_lds_sync() (wave_select.h) stands at each hand-off.
struct AtssLevels { int start[9]; };                          // level_start by value: at most 8 levels

// Squared centre distance of prior q to (cxj, cyj) as an unsigned key: a non-negative double orders like its bit pattern;
// a NaN goes behind every number, +inf included.
__device__ __forceinline__ unsigned long long atss_d2_key(const float4 q, double cxj, double cyj) {
  const double cx = ((double)q.x + (double)q.z) * 0.5, cy = ((double)q.y + (double)q.w) * 0.5;
  const double dx = cx - cxj, dy = cy - cyj;
  const double d2 = dx * dx + dy * dy;
  return d2 != d2 ? ~0ull : (d2 == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(d2));
}

constexpr unsigned short kAtssNone = 0xffffu;                // P <= 65535: no prior has this index

__global__ void __launch_bounds__(1024)
match_atss_kernel(const float4* __restrict__ priors, const AtssLevels lv, int n_levels, const float4* __restrict__ gt,
                  const int* __restrict__ n_gt, const int* __restrict__ status, int topk, int m, int P, int G,
                  int* __restrict__ match, int* __restrict__ n_extra, double* __restrict__ thr_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x, tid = threadIdx.x, nt = (int)blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  unsigned long long* claim = reinterpret_cast<unsigned long long*>(smem);          // [P]
  StagedBox* boxes = reinterpret_cast<StagedBox*>(claim + P);                       // [G]
  double* iou_w = reinterpret_cast<double*>(boxes + G) + (size_t)wave * m;          // [nw][m], this wavefront's row
  unsigned short* cand = reinterpret_cast<unsigned short*>(reinterpret_cast<double*>(boxes + G) + (size_t)nw * m);   // [G][m]
  __shared__ int ls[9];
  __shared__ int added_waves[16];
  const int n = n_gt[b];
  if (status[b] != 0 || n <= 0 || n > G) {                    // skipped: the row stays as it is (mbx_match_extend's rule)
    if (tid == 0 && n_extra) n_extra[b] = 0;
    if (thr_out) for (int j = tid; j < G; j += nt) thr_out[(size_t)b * G + j] = 0.0;
    return;
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) ls[i] = lv.start[i];
  }
  for (int p = tid; p < P; p += nt) claim[p] = 0ull;
  for (int j = tid; j < n; j += nt) {
    const float4 q = gt[(size_t)b * G + j];
    StagedBox s;
    s.box = {(double)q.x, (double)q.y, (double)q.z, (double)q.w};
    s.area = box_area(s.box);
    boxes[j] = s;
  }
  if (thr_out) for (int j = n + tid; j < G; j += nt) thr_out[(size_t)b * G + j] = 0.0;
  __syncthreads();
  int* mt = match + (size_t)b * P;

  for (int j = wave; j < n; j += nw) {                        // pass 1
    const StagedBox sb = boxes[j];
    const double cxj = (sb.box.x1 + sb.box.x2) * 0.5, cyj = (sb.box.y1 + sb.box.y2) * 0.5;
    unsigned short* cj = cand + (size_t)j * m;
    int cnt = 0;
    for (int l = 0; l < n_levels; ++l) {
      const int lo = ls[l], hi = ls[l + 1];
      const int c = topk < hi - lo ? topk : hi - lo;
      unsigned long long cut_k = ~0ull;                       // the whole level: no pair is over (all ones, INT_MAX)
      int cut_i = 0x7fffffff;
      if (c < hi - lo) {
        unsigned long long last_k = 0ull;                     // every pair is over (0, -1)
        int last_i = -1;
        int taken = 0;
        while (taken < c) {
          // scan: the lane's kKeepPairs smallest pairs over the last one taken, then the rounds (wave_select.h)
          KeepList list;
          list.reset();
          for (int p = lo + lane; p < hi; p += 128) {         // two loads in flight: the scan waits on L2, not on arithmetic
            const int p1 = p + 64;
            const float4 q0 = priors[p], q1 = priors[p1 < hi ? p1 : p];
            list.offer(atss_d2_key(q0, cxj, cyj), p, last_k, last_i);
            if (p1 < hi) list.offer(atss_d2_key(q1, cxj, cyj), p1, last_k, last_i);
          }
          keep_list_rounds(list, c, taken, last_k, last_i);
        }
        cut_k = last_k;
        cut_i = last_i;
      }
      for (int base = lo; base < hi; base += 64) {            // the priors at or under the cut, in ascending index
        const int p = base + lane;
        const bool in = p < hi && !pair_less(cut_k, cut_i, atss_d2_key(priors[p], cxj, cyj), p);
        const unsigned long long mask = __ballot(in);
        const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
        if (in && slot < m) cj[slot] = (unsigned short)p;
        cnt += __popcll(mask);
      }
    }
    wave_lds_sync();
    for (int t = lane; t < m; t += 64) {                      // the candidates' IoUs, once for the m of them
      const float4 q = priors[cj[t]];
      const Box e = {(double)q.x, (double)q.y, (double)q.z, (double)q.w};
      iou_w[t] = iou_corners(e, sb.box, sb.area);
    }
    wave_lds_sync();
    double sum = 0.0;                                         // the statistic: every lane, the same serial order
    for (int t = 0; t < m; ++t) sum += iou_w[t];
    const double mean = sum / (double)m;
    double sq = 0.0;
    for (int t = 0; t < m; ++t) { const double d = iou_w[t] - mean; sq += d * d; }
    const double sd = m > 1 ? __dsqrt_rn(sq / (double)(m - 1)) : 0.0;
    const double thr = mean + sd;
    if (lane == 0 && thr_out) thr_out[(size_t)b * G + j] = thr;
    for (int t = lane; t < m; t += 64) {
      const int p = cj[t];
      const double iou = iou_w[t];
      const float4 q = priors[p];
      const double cx = ((double)q.x + (double)q.z) * 0.5, cy = ((double)q.y + (double)q.w) * 0.5;
      const bool inside = sb.box.x1 < cx && cx < sb.box.x2 && sb.box.y1 < cy && cy < sb.box.y2;
      if (iou > 0.0 && iou >= thr && inside && mt[p] < 0)     // a NaN fails both comparisons
        atomicMax(&claim[p], (unsigned long long)__double_as_longlong(iou));
      else
        cj[t] = kAtssNone;
    }
    wave_lds_sync();                                          // the next box reuses iou_w
  }
  __syncthreads();

  int added = 0;                                              // pass 2
  for (int e = tid; e < n * m; e += nt) {
    const int p = cand[e];
    if (p == kAtssNone) continue;
    const int j = e / m;
    const float4 q = priors[p];
    const Box pe = {(double)q.x, (double)q.y, (double)q.z, (double)q.w};
    const double iou = iou_corners(pe, boxes[j].box, boxes[j].area);
    if ((unsigned long long)__double_as_longlong(iou) != claim[p]) continue;
    const unsigned old = atomicMin(reinterpret_cast<unsigned*>(mt + p), (unsigned)j);
    if (old & 0x80000000u) ++added;                           // it was still free: counted once
  }
  if (!n_extra) return;
  added = wave_sum(added);
  if (lane == 0) added_waves[wave] = added;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < nw; ++w) total += added_waves[w];
    n_extra[b] = total;
  }
}

// ---------------------------------------------------------------------- loss
// loc_factor: 0.5 where partial[2b] holds sums of squares (L2: alpha * tf.nn.l2_loss), 1 where it holds the terms themselves.
__global__ void loss_final_kernel(const double* __restrict__ partial, int B, float alpha, double loc_factor,
                                  float* __restrict__ loss2) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double a = 0.0, c = 0.0;
    for (int b = 0; b < B; ++b) { a += partial[2 * b]; c += partial[2 * b + 1]; }
    loss2[0] = alpha * (float)(a * loc_factor);
    loss2[1] = (float)c;
  }
}

// ------------------------------------------------------------- location terms
// The location terms of mbx_loss_fwd_bwd_loc other than L2 (mbx.h has the definitions), in float64 from the widened
// float32 corners: the term L of one positive and dL/d(l.x1, l.y1, l.x2, l.y2).  Every min / max takes its FIRST argument at
// a tie and hands its gradient to it; max(0, .) passes gradient only where its argument is > 0.
//
// One axis of the IoU family (x or y): the prediction's two coordinates a, b put in order, and every quantity of that axis
// with its derivative by the ordered pair (lo, hi).
struct LocAxis {
  double ext, gext;          // hi - lo of the prediction (w or h), of the ground truth as given (gw or gh)
  double ov, ov_lo, ov_hi;   // intersection side max(0, min(hi, g.hi) - max(lo, g.lo)), its derivatives
  double enc, enc_lo, enc_hi;  // enclosing side max(hi, g.hi) - min(lo, g.lo), its derivatives
  double s;                  // lo + hi - g.lo - g.hi: twice the centre distance
  bool lo_is_a, hi_is_a;     // lo = min(a, b) is a, hi = max(a, b) is a: where the gradients of lo and hi go
};

__device__ __forceinline__ LocAxis loc_axis(double a, double b, double glo, double ghi) {
  LocAxis t;
  t.lo_is_a = a <= b;
  t.hi_is_a = a >= b;
  const double lo = t.lo_is_a ? a : b, hi = t.hi_is_a ? a : b;
  t.ext = hi - lo;
  t.gext = ghi - glo;
  const bool hi_in = hi <= ghi, lo_in = lo >= glo;           // min(hi, g.hi), max(lo, g.lo)
  const double side = (hi_in ? hi : ghi) - (lo_in ? lo : glo);
  const bool open = side > 0.0;
  t.ov = open ? side : 0.0;
  t.ov_hi = (open && hi_in) ? 1.0 : 0.0;
  t.ov_lo = (open && lo_in) ? -1.0 : 0.0;
  const bool hi_out = hi >= ghi, lo_out = lo <= glo;         // max(hi, g.hi), min(lo, g.lo)
  t.enc = (hi_out ? hi : ghi) - (lo_out ? lo : glo);
  t.enc_hi = hi_out ? 1.0 : 0.0;
  t.enc_lo = lo_out ? -1.0 : 0.0;
  t.s = ((lo + hi) - glo) - ghi;
  return t;
}

// loc_type is the same for the whole launch: the switch is wavefront-uniform.  Returns L; (dx1, dy1, dx2, dy2) = dL/dl.
__device__ __forceinline__ double loc_term(int loc_type, double beta, const float4 lf, const float4 gf, double& dx1,
                                           double& dy1, double& dx2, double& dy2) {
  if (loc_type == MBX_LOC_SMOOTH_L1) {
    const double r0 = (double)lf.x - (double)gf.x, r1 = (double)lf.y - (double)gf.y, r2 = (double)lf.z - (double)gf.z,
                 r3 = (double)lf.w - (double)gf.w;
    double L = 0.0;
    auto side = [&](double r, double& d) {                   // |r| == beta takes the linear branch
      const double m = fabs(r);
      if (m < beta) { L += 0.5 * m * m / beta; d = r / beta; }
      else { L += m - 0.5 * beta; d = r > 0.0 ? 1.0 : -1.0; }
    };
    side(r0, dx1); side(r1, dy1); side(r2, dx2); side(r3, dy2);
    return L;
  }
  constexpr double kEps = 1e-7, kPi = 3.14159265358979323846;
  const LocAxis X = loc_axis((double)lf.x, (double)lf.z, (double)gf.x, (double)gf.z);
  const LocAxis Y = loc_axis((double)lf.y, (double)lf.w, (double)gf.y, (double)gf.w);
  const double inter = X.ov * Y.ov;
  const double uni = X.ext * Y.ext + X.gext * Y.gext - inter;
  const double ue = uni + kEps, iou = inter / ue;
  // derivatives by (x lo, x hi, y lo, y hi): of the intersection, of the union, then of 1 - IoU = (IoU dU - dI) / (U + eps)
  const double i_xl = Y.ov * X.ov_lo, i_xh = Y.ov * X.ov_hi, i_yl = X.ov * Y.ov_lo, i_yh = X.ov * Y.ov_hi;
  const double u_xl = -Y.ext - i_xl, u_xh = Y.ext - i_xh, u_yl = -X.ext - i_yl, u_yh = X.ext - i_yh;
  double L = 1.0 - iou;
  double g_xl = (iou * u_xl - i_xl) / ue, g_xh = (iou * u_xh - i_xh) / ue, g_yl = (iou * u_yl - i_yl) / ue,
         g_yh = (iou * u_yh - i_yh) / ue;
  if (loc_type == MBX_LOC_GIOU) {                            // + t, t = (C - U) / (C + eps): dt = (dC - dU - t dC) / (C + eps)
    const double c = X.enc * Y.enc, ce = c + kEps, t = (c - uni) / ce;
    const double c_xl = Y.enc * X.enc_lo, c_xh = Y.enc * X.enc_hi, c_yl = X.enc * Y.enc_lo, c_yh = X.enc * Y.enc_hi;
    L += t;
    g_xl += (c_xl - u_xl - t * c_xl) / ce;
    g_xh += (c_xh - u_xh - t * c_xh) / ce;
    g_yl += (c_yl - u_yl - t * c_yl) / ce;
    g_yh += (c_yh - u_yh - t * c_yh) / ce;
  } else {                                                   // DIoU, CIoU: + q, q = rho^2 / D: dq = (d rho^2 - q dD) / D
    const double dd = X.enc * X.enc + Y.enc * Y.enc + kEps;
    const double q = (X.s * X.s + Y.s * Y.s) / 4.0 / dd;
    L += q;
    g_xl += (0.5 * X.s - q * 2.0 * X.enc * X.enc_lo) / dd;
    g_xh += (0.5 * X.s - q * 2.0 * X.enc * X.enc_hi) / dd;
    g_yl += (0.5 * Y.s - q * 2.0 * Y.enc * Y.enc_lo) / dd;
    g_yh += (0.5 * Y.s - q * 2.0 * Y.enc * Y.enc_hi) / dd;
    if (loc_type == MBX_LOC_CIOU) {                          // + a v, a held constant
      const double delta = atan2(X.gext, Y.gext) - atan2(X.ext, Y.ext);
      const double v = (4.0 / (kPi * kPi)) * delta * delta;
      const double a = v / (1.0 - iou + v + kEps);
      L += a * v;
      const double sq = X.ext * X.ext + Y.ext * Y.ext;
      if (sq != 0.0) {                                       // d atan2(w, h) = (h dw - w dh) / (w^2 + h^2); 0 at w = h = 0
        const double k = a * (8.0 / (kPi * kPi)) * delta / sq;
        const double v_w = -k * Y.ext, v_h = k * X.ext;      // a dv/dw, a dv/dh
        g_xl -= v_w; g_xh += v_w; g_yl -= v_h; g_yh += v_h;
      }
    }
  }
  dx1 = (X.lo_is_a ? g_xl : 0.0) + (X.hi_is_a ? g_xh : 0.0);
  dx2 = (X.lo_is_a ? 0.0 : g_xl) + (X.hi_is_a ? 0.0 : g_xh);
  dy1 = (Y.lo_is_a ? g_yl : 0.0) + (Y.hi_is_a ? g_yh : 0.0);
  dy2 = (Y.lo_is_a ? 0.0 : g_yl) + (Y.hi_is_a ? 0.0 : g_yh);
  return L;
}

// ------------------------------------------------------- IoU-aware confidence target
// The positive side of mbx_loss_fwd_bwd_quality (mbx.h has the definition), in float64 from the widened float32 values.
// q is the IoU of loc_term's IoU family, from the same loc_axis on the same inputs: the prediction put in order, the ground
// truth as given, I / (U + 1e-7).
__device__ __forceinline__ double quality_iou(const float4 lf, const float4 gf) {
  const LocAxis X = loc_axis((double)lf.x, (double)lf.z, (double)gf.x, (double)gf.z);
  const LocAxis Y = loc_axis((double)lf.y, (double)lf.w, (double)gf.y, (double)gf.w);
  const double inter = X.ov * Y.ov;
  const double uni = X.ext * Y.ext + X.gext * Y.gext - inter;
  return inter / (uni + 1e-7);
}

// Returns the term L = -w_pos M t, t = q log c + (1 - q) log w; dLds = -w_pos (dM/ds t + M dt/ds), q a constant.
//   QFL: M = |q - s|^gamma; dM/ds = -gamma |q - s|^(gamma-1) sgn(q - s), taken as M / |q - s| (one pow), and exactly 0 at
//        q == s; with gamma == 0 M is the constant 1 and the dM term is left out.  gamma is 0 or >= 1 (the entry checks);
//        gamma == 2, the papers' exponent and the host's default, is (q - s)^2 and -2 (q - s): no pow, no quotient (the pow and
//        the quotient are 2.2 of the 4.8 us QFL adds to a call at P = 646, tools/loss_quality_bench.py).
//   VFL: M = q, no dM term.
// `quality` is the same for the whole launch: the switch is wavefront-uniform.  c, w >= 1e-10: both logs are finite.
__device__ __forceinline__ double quality_positive(int quality, double q, float sf, float cf, float wf, float gamma,
                                                   float w_pos, double& dLds) {
  const double s = (double)sf, c = (double)cf, w = (double)wf, wp = (double)w_pos;
  const double t = q * log(c) + (1.0 - q) * log(w);
  const double dt = q / c - (1.0 - q) / w;
  if (quality == MBX_QUALITY_VFL || gamma == 0.0f) {
    const double M = quality == MBX_QUALITY_VFL ? q : 1.0;
    dLds = -wp * (M * dt);
    return -wp * M * t;
  }
  const double diff = q - s;
  double M, dM;
  if (gamma == 2.0f) {                                       // the papers' exponent: (q - s)^2 and -2 (q - s), no pow, no quotient
    M = diff * diff;
    dM = -2.0 * diff;
  } else {
    const double a = fabs(diff);
    M = pow(a, (double)gamma);
    dM = diff == 0.0 ? 0.0 : (diff > 0.0 ? -(double)gamma : (double)gamma) * (M / a);
  }
  dLds = -wp * (dM * t + M * dt);
  return -wp * M * t;
}

// ------------------------------------------------- loss with hard-negative mining
// Composite key of a negative: the order-preserving image of its input float (score_order_key) above the INVERTED index
// P-1-p, so that unsigned order = (score descending, p ascending) and no two candidates are equal.
__device__ __forceinline__ unsigned long long mined_key(float conf_in, int P, int p) {
  return ((unsigned long long)score_order_key(conf_in) << 32) | (unsigned)(P - 1 - p);
}

// The cut of hard-negative mining for image b: the K-th largest composite key among its negatives, K as in mbx.h
// (mbx_loss_fwd_bwd_mined); a negative is selected iff its key is >= the cut.  Called by every thread of a workgroup of
// kThreads (loss_mined_kernel, loss_focal_kernel).  Found by a radix select: per 8-bit digit, most significant
// first, a 256-bin LDS histogram of the candidates that still share the digits fixed so far, then one wave
// walks the bins from the top to the one that holds the K-th.  No sort, nothing held per thread: any P.  A pass re-reads
// the row (2.6-26 KB: L1 / L2 hits).  The select ends as soon as the bin it lands in is taken whole (its count is what is
// still needed): with distinct scores that is after 3-4 passes, and at once when K is 0 or every negative is taken.  Index
// digits above the bits of P-1 are zero for every candidate and are skipped.  K goes to n_neg[b] (n_neg may be null).
// IGNORE (mbx_loss_fwd_bwd_ignore): a prior with match == MBX_MATCH_IGNORED is no candidate and no positive -- the first
// pass counts them (a wave sum, then an integer LDS add: any order, one result) and takes them off P before n_pos.
template <bool IGNORE = false>
__device__ __forceinline__ unsigned long long mined_select_cut(const int* __restrict__ mt, const float* __restrict__ cf,
                                                               int P, int neg_per_pos, int min_neg, int b,
                                                               int* __restrict__ n_neg) {
  static_assert(kThreads == 256, "one thread per histogram bin, four bins per lane of the walking wave");
  __shared__ unsigned hist[256];
  __shared__ unsigned long long sh_cut;
  __shared__ int sh_need, sh_done;
  __shared__ int sh_ignored;         // IGNORE only
  const int tid = threadIdx.x;
  if (IGNORE && tid == 0) sh_ignored = 0;                     // before the first pass's barrier
  unsigned long long cut = 0ull;     // the digits fixed so far, zeros below
  int need = 0;                      // candidates still to take among those that share them
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (shift < 32 && ((unsigned)(P - 1) >> shift) == 0) continue;
    const unsigned long long fixed = shift == 56 ? 0ull : ~0ull << (shift + 8);
    hist[tid] = 0u;
    __syncthreads();
    int ignored = 0;
    for (int p = tid; p < P; p += kThreads) {
      const int m = mt[p];
      if (m >= 0) continue;
      if (IGNORE && m == MBX_MATCH_IGNORED) { ++ignored; continue; }
      const unsigned long long key = mined_key(cf[p], P, p);
      if (((key ^ cut) & fixed) == 0ull) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    if (IGNORE && shift == 56) {
      ignored = wave_sum(ignored);
      if ((tid & 63) == 0 && ignored) atomicAdd(&sh_ignored, ignored);
    }
    __syncthreads();
    if (tid < 64) {                  // lane l owns bins 4l .. 4l+3; `incl` = candidates in its bins and all higher ones
      const unsigned h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
      const unsigned own = h0 + h1 + h2 + h3;
      unsigned incl = own;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_down(incl, o, 64);
        if (tid + o < 64) incl += t;
      }
      bool whole = false;            // the answer is known without looking at a bin: nothing, or every negative
      if (shift == 56) {             // first pass: every negative was counted
        const int n_negatives = (int)__shfl(incl, 0, 64), n_pos = P - n_negatives - (IGNORE ? sh_ignored : 0);
        long long K = (long long)neg_per_pos * (long long)n_pos;
        if (K < (long long)min_neg) K = min_neg;
        if (K > (long long)n_negatives) K = n_negatives;
        need = (int)K;
        whole = need == 0 || need == n_negatives;
        if (tid == 0) {
          if (n_neg) n_neg[b] = need;
          if (whole) { sh_cut = need == 0 ? ~0ull : 0ull; sh_need = 0; sh_done = 1; }   // no key is all ones: index < 2^31
        }
      }
      const unsigned above = incl - own, k = (unsigned)need;
      if (!whole && above < k && k <= incl) {                 // exactly one lane: the K-th lies in one of its four bins
        unsigned a = above, cnt = h3;
        int d = 3;
        if (k > a + h3) { a += h3; cnt = h2; d = 2;
          if (k > a + h2) { a += h2; cnt = h1; d = 1;
            if (k > a + h1) { a += h1; cnt = h0; d = 0; } } }
        sh_cut = cut | ((unsigned long long)(4 * tid + d) << shift);
        sh_need = (int)(k - a);
        sh_done = cnt == k - a;
      }
    }
    __syncthreads();
    cut = sh_cut;
    need = sh_need;
    if (sh_done) break;
  }
  return cut;
}

// --------------------------------------------------------- the three loss kernels
// One body for mbx_loss_fwd_bwd, _mined and _focal (mbx.h).  One workgroup of kThreads per image: a strided pass over the
// image's priors that writes both gradients and accumulates the two loss terms in double, a wave64 + LDS reduction, and
// partial[2b], partial[2b + 1] for loss_final_kernel.
//   FOCAL: a positive's -log c is weighted by w_pos * w^gamma, a counted negative's -log w by w_neg * c^gamma.  One powf per
//     prior on top of the expf / logf (x^(gamma-1) is x^gamma / x); the term is formed in double from the float32 power and
//     logarithm, the gradient in float32.  Without FOCAL the power and the weight are the constant 1 and gamma, w_pos and
//     w_neg are not read.
//   MINED: only the negatives at or over mined_select_cut's cut count, and the select writes n_neg[b].  Without MINED
//     there is no select, no key and every negative counts; then n_neg[b] = P - positives is written under FOCAL (if n_neg
//     is given) and nothing is counted without it: the plain entry has no n_neg.
// gamma == 0 with unit weights is the plain function bit for bit: the power is then the constant 1 and the
// gamma * x^(gamma-1) * log term is left out, so every product with the power or a weight is `x * 1.0f` (or 1.0 * x in
// double), which is x; the file is built with -ffp-contract=off, so no product is fused into a sum either.  That is what
// makes loss_kernel and loss_focal_kernel<false> at gamma = 0, weights (1, 1) agree (loss_mined_kernel and <true> likewise).
// An unselected negative adds no loss and gets the gradient +0, not 0 * grad_scale: +0 whatever the sign of grad_scale.
//   LOC_ANY: the location term of a positive is the one `loc_type` names (loc_term above, float64; MBX_LOC_L2 takes the
//     float32 lines of the other kernels, so that type gives their bytes).  Without LOC_ANY it is L2 at compile time and
//     loc_type and loc_beta are not read: the four kernels from before the choice keep their code.
//   QUALITY (with FOCAL): a positive's confidence target is q, the IoU of its prediction with its box (quality_positive
//     above, float64: two logs and at most one pow for the few lanes that hold a positive), and the image's sum of q and
//     number of positives go to q_stats.  `quality` (MBX_QUALITY_QFL or _VFL) is the same for the whole launch, like
//     loc_type.  The negatives run the float32 lines below unchanged: their d_logits are loss_loc_kernel's bytes.  q is
//     taken from loc_axis here, not handed over by loc_term: the location lines stay what they are.  Without QUALITY
//     `quality` and q_stats are not read and nothing of this is compiled in.
//   IGNORE (with FOCAL and LOC_ANY; mbx_loss_fwd_bwd_ignore): a prior with match == MBX_MATCH_IGNORED is neither positive nor
//     negative -- no term in either sum, d_locs 0 and d_logits +0 whatever the sign of grad_scale, no key in the select
//     (mined_select_cut<true>), nothing in q_stats; without MINED they are counted and n_neg[b] = P - positives - ignored.
//     Every other negative value of match is a negative, as without the flag.  One compare per prior and one count; without
//     IGNORE the compare is a compile-time false and the eight kernels from before the flag keep their code.
template <bool MINED, bool FOCAL, bool LOC_ANY, bool QUALITY, bool IGNORE = false>
__device__ __forceinline__ void loss_body(const float4* __restrict__ decoded, const float* __restrict__ logits, int is_logit,
                                          const float4* __restrict__ gt, const int* __restrict__ match, float alpha,
                                          float grad_scale, int P, int G, int loc_type, float loc_beta, float gamma,
                                          float w_pos, float w_neg, int neg_per_pos, int min_neg,
                                          double* __restrict__ partial /*[B,2]*/, float4* __restrict__ d_locs,
                                          float* __restrict__ d_logits, int* __restrict__ n_neg, int quality,
                                          double* __restrict__ q_stats /*[B,2]*/) {
  static_assert(!QUALITY || FOCAL, "the quality target replaces the focal positive term");
  static_assert(!IGNORE || (FOCAL && LOC_ANY), "the ignore band has the superset entry only");
  constexpr bool kNegFromPositives = FOCAL && !MINED;        // n_neg[b] = P - positives
  constexpr bool kCountIgnored = IGNORE && kNegFromPositives;   // ... - ignored
  constexpr bool kCountPositives = kNegFromPositives || QUALITY;
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned long long cut = 0ull;                             // no key is below 0: every negative counts
  if (MINED) cut = mined_select_cut<IGNORE>(match + (size_t)b * P, logits + (size_t)b * P, P, neg_per_pos, min_neg, b, n_neg);
  const bool modulated = FOCAL && gamma != 0.0f;

  double loc_acc = 0.0, conf_acc = 0.0, q_acc = 0.0;
  int n_pos = 0, n_ign = 0;
  for (int p = tid; p < P; p += kThreads) {
    const size_t i = (size_t)b * P + p;
    const int m = match[i];
    const float z = logits[i];
    float4 dl = make_float4(0.f, 0.f, 0.f, 0.f);
    float g;
    if (IGNORE && m == MBX_MATCH_IGNORED) {
      g = 0.f;                                              // neither positive nor negative: no loss, +0 whatever grad_scale is
      if (kCountIgnored) ++n_ign;
    } else if (MINED && m < 0 && mined_key(z, P, p) < cut) {
      g = 0.f;                                              // an unselected negative: no loss, +0 whatever grad_scale is
    } else {
      const float s = is_logit ? 1.0f / (1.0f + expf(-z)) : z;
      const float c = __fadd_rn(s, 1e-10f);                  // loss.py:74
      const float w = __fadd_rn(__fsub_rn(1.0f, c), 1e-10f);
      const float ds = is_logit ? s * (1.0f - s) : 1.0f;
      const bool pos = m >= 0;
      if (pos) {
        const float4 l = decoded[i], q = gt[(size_t)b * G + m];
        if (!LOC_ANY || loc_type == MBX_LOC_L2) {
          const float d0 = __fsub_rn(l.x, q.x), d1 = __fsub_rn(l.y, q.y), d2 = __fsub_rn(l.z, q.z), d3 = __fsub_rn(l.w, q.w);
          loc_acc += (double)d0 * d0 + (double)d1 * d1 + (double)d2 * d2 + (double)d3 * d3;   // loss.py:100
          const float a = alpha * grad_scale;
          dl = make_float4(a * d0, a * d1, a * d2, a * d3);
        } else {
          double dx1, dy1, dx2, dy2;
          loc_acc += loc_term(loc_type, (double)loc_beta, l, q, dx1, dy1, dx2, dy2);
          const double a = (double)alpha * (double)grad_scale;                                // one rounding, at the store
          dl = make_float4((float)(a * dx1), (float)(a * dy1), (float)(a * dx2), (float)(a * dy2));
        }
        if (kCountPositives) ++n_pos;
        if (QUALITY) {
          const double iou = quality_iou(l, q);
          double dLds;
          conf_acc += quality_positive(quality, iou, s, c, w, gamma, w_pos, dLds);
          q_acc += iou;
          g = (float)(dLds * (double)ds * (double)grad_scale);                                // one rounding, at the store
        }
      }
      if (!(QUALITY && pos)) {
        // The two sides are one expression with c and w exchanged, -wt * base^gamma * log(arg): one logf and one powf for
        // a wavefront that holds positives and negatives, not one of each per side.
        const float arg = pos ? c : w, base = pos ? w : c, wt = FOCAL ? (pos ? w_pos : w_neg) : 1.0f;
        const float lg = logf(arg);                                                         // loss.py:101
        const float pw = modulated ? powf(base, gamma) : 1.0f;
        conf_acc -= (double)wt * ((double)pw * (double)lg);
        float d = (ds * pw) / arg;
        if (modulated) d = d - gamma * (pw / base) * lg * ds;               // lg <= 0: both terms are >= 0, no cancellation
        d = wt * d;
        g = (pos ? -d : d) * grad_scale;
      }
    }
    if (d_locs) d_locs[i] = dl;
    if (d_logits) d_logits[i] = g;
  }
  loc_acc = wave_sum(loc_acc);
  conf_acc = wave_sum(conf_acc);
  if (QUALITY) q_acc = wave_sum(q_acc);
  __shared__ double red[kWaves][QUALITY ? 3 : 2];
  __shared__ int pos_waves[kWaves];
  __shared__ int ign_waves[kWaves];                          // kCountIgnored only
  if (kCountPositives) n_pos = wave_sum(n_pos);
  if (kCountIgnored) n_ign = wave_sum(n_ign);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = loc_acc; red[tid >> 6][1] = conf_acc;
    if (QUALITY) red[tid >> 6][QUALITY ? 2 : 0] = q_acc;
    if (kCountPositives) pos_waves[tid >> 6] = n_pos;
    if (kCountIgnored) ign_waves[tid >> 6] = n_ign;
  }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, c = 0.0;
    for (int w = 0; w < kWaves; ++w) { a += red[w][0]; c += red[w][1]; }
    partial[2 * b] = a;
    partial[2 * b + 1] = c;
    int total = 0;
    if (kCountPositives)
      for (int w = 0; w < kWaves; ++w) total += pos_waves[w];
    int ignored = 0;
    if (kCountIgnored)
      for (int w = 0; w < kWaves; ++w) ignored += ign_waves[w];
    if (kNegFromPositives && n_neg) n_neg[b] = P - total - ignored;    // every negative counts
    if (QUALITY && q_stats) {                                // the wavefronts' sums in their fixed order: the same bytes every call
      double qs = 0.0;
      for (int w = 0; w < kWaves; ++w) qs += red[w][QUALITY ? 2 : 0];
      q_stats[2 * b] = qs;
      q_stats[2 * b + 1] = (double)total;
    }
  }
}

__global__ void __launch_bounds__(kThreads)
loss_kernel(const float4* __restrict__ decoded, const float* __restrict__ logits, int is_logit,
            const float4* __restrict__ gt, const int* __restrict__ match, float alpha, float grad_scale,
            int P, int G, double* __restrict__ partial /*[B,2]*/, float4* __restrict__ d_locs,
            float* __restrict__ d_logits) {
  loss_body<false, false, false, false>(decoded, logits, is_logit, gt, match, alpha, grad_scale, P, G, MBX_LOC_L2, 0.0f, 0.0f, 1.0f,
                                 1.0f, 0, 0, partial, d_locs, d_logits, nullptr, MBX_QUALITY_NONE, nullptr);
}

__global__ void __launch_bounds__(kThreads)
loss_mined_kernel(const float4* __restrict__ decoded, const float* __restrict__ logits, int is_logit,
                  const float4* __restrict__ gt, const int* __restrict__ match, float alpha, float grad_scale,
                  int P, int G, int neg_per_pos, int min_neg, double* __restrict__ partial /*[B,2]*/,
                  float4* __restrict__ d_locs, float* __restrict__ d_logits, int* __restrict__ n_neg) {
  loss_body<true, false, false, false>(decoded, logits, is_logit, gt, match, alpha, grad_scale, P, G, MBX_LOC_L2, 0.0f, 0.0f, 1.0f,
                                1.0f, neg_per_pos, min_neg, partial, d_locs, d_logits, n_neg, MBX_QUALITY_NONE, nullptr);
}

template <bool MINED>
__global__ void __launch_bounds__(kThreads)
loss_focal_kernel(const float4* __restrict__ decoded, const float* __restrict__ logits, int is_logit,
                  const float4* __restrict__ gt, const int* __restrict__ match, float alpha, float grad_scale,
                  int P, int G, float gamma, float w_pos, float w_neg, int neg_per_pos, int min_neg,
                  double* __restrict__ partial /*[B,2]*/, float4* __restrict__ d_locs, float* __restrict__ d_logits,
                  int* __restrict__ n_neg) {
  loss_body<MINED, true, false, false>(decoded, logits, is_logit, gt, match, alpha, grad_scale, P, G, MBX_LOC_L2, 0.0f, gamma, w_pos,
                                w_neg, neg_per_pos, min_neg, partial, d_locs, d_logits, n_neg, MBX_QUALITY_NONE, nullptr);
}

// mbx_loss_fwd_bwd_loc: loss_focal_kernel<MINED> with the location term chosen at run time.
template <bool MINED>
__global__ void __launch_bounds__(kThreads)
loss_loc_kernel(const float4* __restrict__ decoded, const float* __restrict__ logits, int is_logit,
                const float4* __restrict__ gt, const int* __restrict__ match, float alpha, float grad_scale,
                int P, int G, int loc_type, float loc_beta, float gamma, float w_pos, float w_neg, int neg_per_pos,
                int min_neg, double* __restrict__ partial /*[B,2]*/, float4* __restrict__ d_locs,
                float* __restrict__ d_logits, int* __restrict__ n_neg) {
  loss_body<MINED, true, true, false>(decoded, logits, is_logit, gt, match, alpha, grad_scale, P, G, loc_type, loc_beta, gamma, w_pos,
                               w_neg, neg_per_pos, min_neg, partial, d_locs, d_logits, n_neg, MBX_QUALITY_NONE, nullptr);
}

// mbx_loss_fwd_bwd_quality under MBX_QUALITY_QFL / _VFL: loss_loc_kernel<MINED> with the IoU as the positives' target.
template <bool MINED>
__global__ void __launch_bounds__(kThreads)
loss_quality_kernel(const float4* __restrict__ decoded, const float* __restrict__ logits, int is_logit,
                    const float4* __restrict__ gt, const int* __restrict__ match, float alpha, float grad_scale,
                    int P, int G, int loc_type, float loc_beta, int quality, float gamma, float w_pos, float w_neg,
                    int neg_per_pos, int min_neg, double* __restrict__ partial /*[B,2]*/, float4* __restrict__ d_locs,
                    float* __restrict__ d_logits, int* __restrict__ n_neg, double* __restrict__ q_stats /*[B,2]*/) {
  loss_body<MINED, true, true, true>(decoded, logits, is_logit, gt, match, alpha, grad_scale, P, G, loc_type, loc_beta, gamma,
                                     w_pos, w_neg, neg_per_pos, min_neg, partial, d_locs, d_logits, n_neg, quality, q_stats);
}

// mbx_loss_fwd_bwd_ignore: loss_loc_kernel<MINED> (QUALITY = false) or loss_quality_kernel<MINED> with the ignore band.
template <bool MINED, bool QUALITY>
__global__ void __launch_bounds__(kThreads)
loss_ignore_kernel(const float4* __restrict__ decoded, const float* __restrict__ logits, int is_logit,
                   const float4* __restrict__ gt, const int* __restrict__ match, float alpha, float grad_scale,
                   int P, int G, int loc_type, float loc_beta, int quality, float gamma, float w_pos, float w_neg,
                   int neg_per_pos, int min_neg, double* __restrict__ partial /*[B,2]*/, float4* __restrict__ d_locs,
                   float* __restrict__ d_logits, int* __restrict__ n_neg, double* __restrict__ q_stats /*[B,2]*/) {
  loss_body<MINED, true, true, QUALITY, true>(decoded, logits, is_logit, gt, match, alpha, grad_scale, P, G, loc_type, loc_beta,
                                              gamma, w_pos, w_neg, neg_per_pos, min_neg, partial, d_locs, d_logits, n_neg,
                                              quality, q_stats);
}

}  // namespace

// =============================================================================== C ABI
extern "C" int mbx_decode_conf(const float* raw_locs, const float* logits, const float* priors, int B,
                               int P, float eps_add, float* decoded, float* conf, mbx_stream_t stream) {
  if (B < 0 || P <= 0) return MBX_ERR_INVALID_ARG;
  if ((decoded && (!raw_locs || !priors)) || (conf && !logits)) return MBX_ERR_INVALID_ARG;
  if (B == 0 || (!decoded && !conf)) return MBX_OK;
  const int total = B * P;
  int blocks = (total + kThreads - 1) / kThreads;
  if (blocks > 2048) blocks = 2048;
  MBX_ENTER();
  hipLaunchKernelGGL(decode_conf_kernel, dim3(blocks), dim3(kThreads), 0, mbx_s(stream),
                     reinterpret_cast<const float4*>(raw_locs), logits, reinterpret_cast<const float4*>(priors),
                     total, P, eps_add, reinterpret_cast<float4*>(decoded), conf);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

static size_t match_lds_bytes(int P, int G) { return (size_t)P * 36 + (size_t)G * 16 + 16; }

extern "C" size_t mbx_match_workspace_bytes(int, int, int) { return 0; }

extern "C" int mbx_match(const float* decoded, const float* conf, const float* gt, const int32_t* n_gt,
                         float alpha, int B, int P, int G, int32_t* match, int32_t* status, void*, size_t,
                         mbx_stream_t stream) {
  if (!decoded || !conf || !gt || !n_gt || !match || !status || B < 0 || P <= 0 || G <= 0) return MBX_ERR_INVALID_ARG;
  if (B == 0) return MBX_OK;
  const size_t lds = match_lds_bytes(P, G);
  if (lds > 150 * 1024) return MBX_ERR_UNSUPPORTED;        // P > ~4200 at G=100
  static const int force_nt = mbx_env_int("MBX_MATCH_THREADS", 0);     // (tools/match_bench.py)
  const int nthreads = force_nt ? force_nt : (P > 1536 ? 512 : kThreads);
  MBX_ENTER();
  if (lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(match_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess) return MBX_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(match_kernel, dim3(B), dim3(nthreads), lds, mbx_s(stream),
                     reinterpret_cast<const float4*>(decoded), conf, reinterpret_cast<const float4*>(gt), n_gt,
                     alpha, P, G, match, status);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_match_extend(const float* priors, const float* gt, const int32_t* n_gt, const int32_t* status,
                                float iou_threshold, int B, int P, int G, int32_t* match, int32_t* n_extra,
                                mbx_stream_t stream) {
  if (!priors || !gt || !n_gt || !status || !match || B < 0 || P <= 0 || G <= 0) return MBX_ERR_INVALID_ARG;
  if (!(iou_threshold > 0.0f && iou_threshold <= 1.0f)) return MBX_ERR_INVALID_ARG;      // a NaN fails both
  const size_t lds = (size_t)G * sizeof(StagedBox);
  if (lds > 60 * 1024) return MBX_ERR_UNSUPPORTED;           // G > 1536: under the 64 KB a launch gets without asking
  if (B == 0) return MBX_OK;
  const int nthreads = P >= 1024 ? 1024 : (P + 63) / 64 * 64;
  MBX_ENTER();
  hipLaunchKernelGGL(match_extend_kernel, dim3(B), dim3(nthreads), lds, mbx_s(stream),
                     reinterpret_cast<const float4*>(priors), reinterpret_cast<const float4*>(gt), n_gt, status,
                     (double)iou_threshold, P, G, match, n_extra);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

// The checks of mbx_match_atss that need no GPU, and what the launch is sized by: m = the candidates per box, the wavefronts
// per image (the most of 16, 8, 4, 2, 1 whose LDS fits a plain launch) and the LDS bytes (mbx.h has the formula).
static int atss_plan(int P, int G, int n_levels, const int32_t* level_start, int topk, int* m_out, int* waves_out,
                     size_t* lds_out) {
  if (!level_start || P <= 0 || G <= 0 || topk < 1 || n_levels < 1 || n_levels > 8) return MBX_ERR_INVALID_ARG;
  if (level_start[0] != 0 || level_start[n_levels] != P) return MBX_ERR_INVALID_ARG;
  long long m = 0;
  for (int l = 0; l < n_levels; ++l) {
    const int size = level_start[l + 1] - level_start[l];
    if (level_start[l + 1] <= level_start[l]) return MBX_ERR_INVALID_ARG;
    m += topk < size ? topk : size;
  }
  if (P >= (int)kAtssNone) return MBX_ERR_UNSUPPORTED;       // (8 P alone is over the LDS of a plain launch there)
  for (int waves = 16; waves >= 1; waves >>= 1) {
    const long long lds = 8ll * P + (long long)sizeof(StagedBox) * G + 2ll * G * m + 8ll * waves * m;
    if (lds + 128 <= 64 * 1024) {                             // 128: the kernel's static LDS (112 bytes) rounded up
      if (m_out) *m_out = (int)m;
      if (waves_out) *waves_out = waves;
      if (lds_out) *lds_out = (size_t)lds;
      return MBX_OK;
    }
  }
  return MBX_ERR_UNSUPPORTED;
}

extern "C" int mbx_match_ignore(const float* boxes, int per_image, const float* gt, const int32_t* n_gt,
                                const int32_t* status, float iou_threshold, int B, int P, int G, int32_t* match,
                                int32_t* n_ignored, mbx_stream_t stream) {
  if (!boxes || !gt || !n_gt || !status || !match || B < 0 || P <= 0 || G <= 0) return MBX_ERR_INVALID_ARG;
  if (!(iou_threshold > 0.0f && iou_threshold <= 1.0f)) return MBX_ERR_INVALID_ARG;      // a NaN fails both
  const size_t lds = (size_t)G * sizeof(StagedBox);
  if (lds > 60 * 1024) return MBX_ERR_UNSUPPORTED;           // G > 1536, as mbx_match_extend
  if (B == 0) return MBX_OK;
  const int nthreads = P >= 1024 ? 1024 : (P + 63) / 64 * 64;
  MBX_ENTER();
  hipLaunchKernelGGL(match_ignore_kernel, dim3(B), dim3(nthreads), lds, mbx_s(stream),
                     reinterpret_cast<const float4*>(boxes), per_image ? (size_t)P : (size_t)0,
                     reinterpret_cast<const float4*>(gt), n_gt, status, (double)iou_threshold, P, G, match, n_ignored);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_match_atss_supported(int P, int G, int n_levels, const int32_t* level_start, int topk) {
  return atss_plan(P, G, n_levels, level_start, topk, nullptr, nullptr, nullptr);
}

extern "C" int mbx_match_atss(const float* priors, const int32_t* level_start, int n_levels, const float* gt,
                              const int32_t* n_gt, const int32_t* status, int topk, int B, int P, int G, int32_t* match,
                              int32_t* n_extra, double* thr, mbx_stream_t stream) {
  if (!priors || !gt || !n_gt || !status || !match || B < 0) return MBX_ERR_INVALID_ARG;
  int m = 0, waves = 0;
  size_t lds = 0;
  const int plan = atss_plan(P, G, n_levels, level_start, topk, &m, &waves, &lds);
  if (plan != MBX_OK) return plan;
  if (B == 0) return MBX_OK;
  AtssLevels lv;
  for (int i = 0; i < 9; ++i) lv.start[i] = i <= n_levels ? level_start[i] : P;
  MBX_ENTER();
  hipLaunchKernelGGL(match_atss_kernel, dim3(B), dim3(waves * 64), lds, mbx_s(stream),
                     reinterpret_cast<const float4*>(priors), lv, n_levels, reinterpret_cast<const float4*>(gt), n_gt,
                     status, topk, m, P, G, match, n_extra, thr);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" size_t mbx_loss_workspace_bytes(int B) { return (size_t)(B > 0 ? B : 1) * 2 * sizeof(double); }
extern "C" size_t mbx_loss_mined_workspace_bytes(int B, int) { return mbx_loss_workspace_bytes(B); }
extern "C" size_t mbx_loss_focal_workspace_bytes(int B, int) { return mbx_loss_workspace_bytes(B); }
extern "C" size_t mbx_loss_loc_workspace_bytes(int B, int) { return mbx_loss_workspace_bytes(B); }
extern "C" size_t mbx_loss_quality_workspace_bytes(int B, int) { return mbx_loss_workspace_bytes(B); }
extern "C" size_t mbx_loss_ignore_workspace_bytes(int B, int) { return mbx_loss_workspace_bytes(B); }

// What the six loss entries share: the argument and workspace checks (every entry needs mbx_loss_workspace_bytes(B)),
// the kernel of `kind`, then loss_final_kernel.  An entry checks its own arguments first; those and the ones here all
// answer MBX_ERR_INVALID_ARG, so a bad argument still goes before a bad workspace.  Focal, loc and quality mine iff
// neg_per_pos != 0; loc_type is MBX_LOC_L2 for every kind but kLoc, kQuality and kIgnore; quality and q_stats are kQuality's
// and kIgnore's (kIgnore with MBX_QUALITY_NONE is the loc kernel's body with the ignore band).
enum class LossKind { kPlain, kMined, kFocal, kLoc, kQuality, kIgnore };

static int launch_loss(LossKind kind, const float* decoded, const float* logits, int conf_is_logit, const float* gt,
                       const int32_t* match, float alpha, float grad_scale, int B, int P, int G, float* loss2,
                       float* d_raw_locs, float* d_logits, int loc_type, float loc_beta, float gamma, float w_pos,
                       float w_neg, int neg_per_pos, int min_neg, int32_t* n_neg, void* workspace, size_t workspace_bytes,
                       mbx_stream_t stream, int quality = MBX_QUALITY_NONE, double* q_stats = nullptr) {
  if (!decoded || !logits || !gt || !match || !loss2 || B <= 0 || P <= 0 || G <= 0) return MBX_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < mbx_loss_workspace_bytes(B)) return MBX_ERR_WORKSPACE;
  double* partial = reinterpret_cast<double*>(workspace);
  const float4* dec4 = reinterpret_cast<const float4*>(decoded);
  const float4* gt4 = reinterpret_cast<const float4*>(gt);
  float4* dl4 = reinterpret_cast<float4*>(d_raw_locs);
  MBX_ENTER();
  switch (kind) {
    case LossKind::kPlain:
      hipLaunchKernelGGL(loss_kernel, dim3(B), dim3(kThreads), 0, mbx_s(stream), dec4, logits, conf_is_logit, gt4, match,
                         alpha, grad_scale, P, G, partial, dl4, d_logits);
      break;
    case LossKind::kMined:
      hipLaunchKernelGGL(loss_mined_kernel, dim3(B), dim3(kThreads), 0, mbx_s(stream), dec4, logits, conf_is_logit, gt4,
                         match, alpha, grad_scale, P, G, neg_per_pos, min_neg, partial, dl4, d_logits, n_neg);
      break;
    case LossKind::kFocal:
      hipLaunchKernelGGL(neg_per_pos ? loss_focal_kernel<true> : loss_focal_kernel<false>, dim3(B), dim3(kThreads), 0,
                         mbx_s(stream), dec4, logits, conf_is_logit, gt4, match, alpha, grad_scale, P, G, gamma, w_pos,
                         w_neg, neg_per_pos, min_neg, partial, dl4, d_logits, n_neg);
      break;
    case LossKind::kLoc:
      hipLaunchKernelGGL(neg_per_pos ? loss_loc_kernel<true> : loss_loc_kernel<false>, dim3(B), dim3(kThreads), 0,
                         mbx_s(stream), dec4, logits, conf_is_logit, gt4, match, alpha, grad_scale, P, G, loc_type, loc_beta,
                         gamma, w_pos, w_neg, neg_per_pos, min_neg, partial, dl4, d_logits, n_neg);
      break;
    case LossKind::kQuality:
      hipLaunchKernelGGL(neg_per_pos ? loss_quality_kernel<true> : loss_quality_kernel<false>, dim3(B), dim3(kThreads), 0,
                         mbx_s(stream), dec4, logits, conf_is_logit, gt4, match, alpha, grad_scale, P, G, loc_type, loc_beta,
                         quality, gamma, w_pos, w_neg, neg_per_pos, min_neg, partial, dl4, d_logits, n_neg, q_stats);
      break;
    case LossKind::kIgnore: {
      auto kernel = quality != MBX_QUALITY_NONE ? (neg_per_pos ? loss_ignore_kernel<true, true> : loss_ignore_kernel<false, true>)
                                                : (neg_per_pos ? loss_ignore_kernel<true, false> : loss_ignore_kernel<false, false>);
      hipLaunchKernelGGL(kernel, dim3(B), dim3(kThreads), 0, mbx_s(stream), dec4, logits, conf_is_logit, gt4, match, alpha,
                         grad_scale, P, G, loc_type, loc_beta, quality, gamma, w_pos, w_neg, neg_per_pos, min_neg, partial, dl4,
                         d_logits, n_neg, q_stats);
      break;
    }
  }
  MBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, mbx_s(stream), partial, B, alpha,
                     loc_type == MBX_LOC_L2 ? 0.5 : 1.0, loss2);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_loss_fwd_bwd(const float* decoded, const float* logits, int conf_is_logit, const float* gt,
                                const int32_t* match, float alpha, float grad_scale, int B, int P, int G, float* loss2,
                                float* d_raw_locs, float* d_logits, void* workspace, size_t workspace_bytes,
                                mbx_stream_t stream) {
  return launch_loss(LossKind::kPlain, decoded, logits, conf_is_logit, gt, match, alpha, grad_scale, B, P, G, loss2,
                     d_raw_locs, d_logits, MBX_LOC_L2, 0.0f, 0.0f, 1.0f, 1.0f, 0, 0, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int mbx_loss_fwd_bwd_mined(const float* decoded, const float* logits, int conf_is_logit, const float* gt,
                                      const int32_t* match, float alpha, float grad_scale, int B, int P, int G, float* loss2,
                                      float* d_raw_locs, float* d_logits, int neg_per_pos, int min_neg, int32_t* n_neg,
                                      void* workspace, size_t workspace_bytes, mbx_stream_t stream) {
  if (neg_per_pos < 1 || min_neg < 0) return MBX_ERR_INVALID_ARG;
  return launch_loss(LossKind::kMined, decoded, logits, conf_is_logit, gt, match, alpha, grad_scale, B, P, G, loss2,
                     d_raw_locs, d_logits, MBX_LOC_L2, 0.0f, 0.0f, 1.0f, 1.0f, neg_per_pos, min_neg, n_neg, workspace,
                     workspace_bytes, stream);
}

// The checks of the focal arguments, shared by mbx_loss_fwd_bwd_focal and mbx_loss_fwd_bwd_loc.
static bool focal_arguments_ok(float gamma, float w_pos, float w_neg, int neg_per_pos, int min_neg) {
  if (!(gamma >= 0.0f && gamma <= 10.0f)) return false;                                    // a NaN fails both
  if (!(w_pos >= 0.0f && w_neg >= 0.0f) || isinf(w_pos) || isinf(w_neg)) return false;
  return !(neg_per_pos < 0 || min_neg < 0 || (neg_per_pos == 0 && min_neg > 0));
}

extern "C" int mbx_loss_fwd_bwd_focal(const float* decoded, const float* logits, int conf_is_logit, const float* gt,
                                      const int32_t* match, float alpha, float grad_scale, int B, int P, int G, float* loss2,
                                      float* d_raw_locs, float* d_logits, float gamma, float w_pos, float w_neg,
                                      int neg_per_pos, int min_neg, int32_t* n_neg, void* workspace, size_t workspace_bytes,
                                      mbx_stream_t stream) {
  if (!focal_arguments_ok(gamma, w_pos, w_neg, neg_per_pos, min_neg)) return MBX_ERR_INVALID_ARG;
  return launch_loss(LossKind::kFocal, decoded, logits, conf_is_logit, gt, match, alpha, grad_scale, B, P, G, loss2,
                     d_raw_locs, d_logits, MBX_LOC_L2, 0.0f, gamma, w_pos, w_neg, neg_per_pos, min_neg, n_neg, workspace,
                     workspace_bytes, stream);
}

extern "C" int mbx_loss_fwd_bwd_loc(const float* decoded, const float* logits, int conf_is_logit, const float* gt,
                                    const int32_t* match, float alpha, float grad_scale, int B, int P, int G, float* loss2,
                                    float* d_raw_locs, float* d_logits, int loc_type, float loc_beta, float gamma, float w_pos,
                                    float w_neg, int neg_per_pos, int min_neg, int32_t* n_neg, void* workspace,
                                    size_t workspace_bytes, mbx_stream_t stream) {
  if (loc_type < MBX_LOC_L2 || loc_type > MBX_LOC_CIOU) return MBX_ERR_INVALID_ARG;
  if (loc_type == MBX_LOC_SMOOTH_L1 && !(loc_beta > 0.0f && !isinf(loc_beta))) return MBX_ERR_INVALID_ARG;   // a NaN fails
  if (!focal_arguments_ok(gamma, w_pos, w_neg, neg_per_pos, min_neg)) return MBX_ERR_INVALID_ARG;
  return launch_loss(LossKind::kLoc, decoded, logits, conf_is_logit, gt, match, alpha, grad_scale, B, P, G, loss2,
                     d_raw_locs, d_logits, loc_type, loc_beta, gamma, w_pos, w_neg, neg_per_pos, min_neg, n_neg, workspace,
                     workspace_bytes, stream);
}

extern "C" int mbx_loss_fwd_bwd_quality(const float* decoded, const float* logits, int conf_is_logit, const float* gt,
                                        const int32_t* match, float alpha, float grad_scale, int B, int P, int G,
                                        float* loss2, float* d_raw_locs, float* d_logits, int loc_type, float loc_beta,
                                        int quality, float gamma, float w_pos, float w_neg, int neg_per_pos, int min_neg,
                                        int32_t* n_neg, double* q_stats, void* workspace, size_t workspace_bytes,
                                        mbx_stream_t stream) {
  if (quality < MBX_QUALITY_NONE || quality > MBX_QUALITY_VFL) return MBX_ERR_INVALID_ARG;
  if (quality == MBX_QUALITY_NONE && q_stats) return MBX_ERR_INVALID_ARG;
  if (quality == MBX_QUALITY_QFL && gamma > 0.0f && gamma < 1.0f) return MBX_ERR_INVALID_ARG;   // |q - s|^(gamma-1) is unbounded
  if (quality == MBX_QUALITY_NONE)                           // the same launches: mbx_loss_fwd_bwd_loc's bytes
    return mbx_loss_fwd_bwd_loc(decoded, logits, conf_is_logit, gt, match, alpha, grad_scale, B, P, G, loss2, d_raw_locs,
                                d_logits, loc_type, loc_beta, gamma, w_pos, w_neg, neg_per_pos, min_neg, n_neg, workspace,
                                workspace_bytes, stream);
  if (loc_type < MBX_LOC_L2 || loc_type > MBX_LOC_CIOU) return MBX_ERR_INVALID_ARG;
  if (loc_type == MBX_LOC_SMOOTH_L1 && !(loc_beta > 0.0f && !isinf(loc_beta))) return MBX_ERR_INVALID_ARG;   // a NaN fails
  if (!focal_arguments_ok(gamma, w_pos, w_neg, neg_per_pos, min_neg)) return MBX_ERR_INVALID_ARG;
  return launch_loss(LossKind::kQuality, decoded, logits, conf_is_logit, gt, match, alpha, grad_scale, B, P, G, loss2,
                     d_raw_locs, d_logits, loc_type, loc_beta, gamma, w_pos, w_neg, neg_per_pos, min_neg, n_neg, workspace,
                     workspace_bytes, stream, quality, q_stats);
}

extern "C" int mbx_loss_fwd_bwd_ignore(const float* decoded, const float* logits, int conf_is_logit, const float* gt,
                                       const int32_t* match, float alpha, float grad_scale, int B, int P, int G,
                                       float* loss2, float* d_raw_locs, float* d_logits, int loc_type, float loc_beta,
                                       int quality, float gamma, float w_pos, float w_neg, int neg_per_pos, int min_neg,
                                       int32_t* n_neg, double* q_stats, void* workspace, size_t workspace_bytes,
                                       mbx_stream_t stream) {
  if (quality < MBX_QUALITY_NONE || quality > MBX_QUALITY_VFL) return MBX_ERR_INVALID_ARG;
  if (quality == MBX_QUALITY_NONE && q_stats) return MBX_ERR_INVALID_ARG;
  if (quality == MBX_QUALITY_QFL && gamma > 0.0f && gamma < 1.0f) return MBX_ERR_INVALID_ARG;   // as mbx_loss_fwd_bwd_quality
  if (loc_type < MBX_LOC_L2 || loc_type > MBX_LOC_CIOU) return MBX_ERR_INVALID_ARG;
  if (loc_type == MBX_LOC_SMOOTH_L1 && !(loc_beta > 0.0f && !isinf(loc_beta))) return MBX_ERR_INVALID_ARG;   // a NaN fails
  if (!focal_arguments_ok(gamma, w_pos, w_neg, neg_per_pos, min_neg)) return MBX_ERR_INVALID_ARG;
  return launch_loss(LossKind::kIgnore, decoded, logits, conf_is_logit, gt, match, alpha, grad_scale, B, P, G, loss2,
                     d_raw_locs, d_logits, loc_type, loc_beta, gamma, w_pos, w_neg, neg_per_pos, min_neg, n_neg, workspace,
                     workspace_bytes, stream, quality, q_stats);
}
