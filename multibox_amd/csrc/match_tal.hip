// libmbx: task-aligned matching behind the bipartite match (mbx_match_tal, mbx.h has the rule; TOOD, Feng et al., ICCV 2021).
// Per box the `topk` priors whose PREDICTION is both confident and well placed -- the largest t = s^alpha * u^beta among the
// priors whose centre lies inside the box -- are selected, and a free prior goes to the selecting box of the largest u, the
// lowest j among equals.  Built with -ffp-contract=off: the float64 metric keeps the order of the numpy restatement
// (tests/tal_oracle.py) and is compared with it bit for bit.
//
// One workgroup of `nw` wavefronts per image, match_atss_kernel's frame (loss.hip).
//   LDS: claim[P] (8 B: the largest bit pattern of u a selecting box has claimed the prior with) | boxes[G] (StagedBox) |
//        added[16] (4 B, the wavefronts' counts) | cand[G][m] (2 B: the free priors a box selected), m = min(topk, P).
//   Pass 1, a wavefront per box j = wave, wave + nw, ...: the selection of wave_select.h over all P priors.  The key of a
//     candidate is the complement of t's bit pattern -- t > 0, so the patterns order like the values and the smallest key is
//     the largest t; equal keys go to the lowest index as they do there; all ones is no candidate (it would be t = +0).  The
//     first scan also counts the candidates: with no more than topk of them every one is selected and no round runs.
//     Otherwise the rounds take min(topk, candidates) pairs and the last one taken is the cut.  One more pass in 64-prior
//     chunks takes the candidates at or under the cut: one that mbx_match left free raises claim[p] with a 64-bit unsigned
//     LDS max on u's bit pattern (u > 0 where t > 0: the patterns order like the values, whoever comes first) and is
//     written to cand (ballot + prefix count).  The metric is computed again in every scan: nothing is stored per prior.
//   Pass 2, every thread over the n x m entries: a selected prior whose u (the same function on the same inputs: the same
//     bits) equals claim[p] lowers match[b,p] with an unsigned integer min -- a free entry is negative, as unsigned above
//     every j -- so the lowest j among the largest u stays; whoever finds the entry still negative counts the prior.
#include "boxes.h"
#include "wave_select.h"

namespace {

constexpr unsigned short kTalNone = 0xffffu;                  // P < 65535: no prior has this index
constexpr unsigned long long kTalNoKey = ~0ull;

// The key of prior p (q its corners) for the box sb, or kTalNoKey where p is no candidate; u = the prediction's IoU with the
// box where it is one.  The centre test reads the prior alone, so the prediction and the score are loaded for the priors
// inside the box only.
__device__ __forceinline__ unsigned long long tal_key(const float4 q, const float4* __restrict__ dec,
                                                      const float* __restrict__ cf, int p, const StagedBox& sb,
                                                      int alpha_halves, int beta, double& u) {
  const double cx = ((double)q.x + (double)q.z) * 0.5, cy = ((double)q.y + (double)q.w) * 0.5;
  if (!(sb.box.x1 < cx && cx < sb.box.x2 && sb.box.y1 < cy && cy < sb.box.y2)) return kTalNoKey;
  const float4 d = dec[p];
  const double s = (double)cf[p];
  const Box e = {(double)d.x, (double)d.y, (double)d.z, (double)d.w};
  u = iou_corners(e, sb.box, sb.area);
  double r = 1.0;
  for (int i = 0; i < (alpha_halves >> 1); ++i) r = r * s;
  if (alpha_halves & 1) r = r * __dsqrt_rn(s);
  double w = 1.0;
  for (int i = 0; i < beta; ++i) w = w * u;
  const double t = r * w;
  return t > 0.0 ? ~(unsigned long long)__double_as_longlong(t) : kTalNoKey;      // a NaN fails
}

__global__ void __launch_bounds__(1024)
match_tal_kernel(const float4* __restrict__ priors, const float4* __restrict__ decoded, const float* __restrict__ conf,
                 const float4* __restrict__ gt, const int* __restrict__ n_gt, const int* __restrict__ status, int topk,
                 int alpha_halves, int beta, int m, int P, int G, int* __restrict__ match, int* __restrict__ n_extra,
                 double* __restrict__ thr_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x, tid = threadIdx.x, nt = (int)blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  unsigned long long* claim = reinterpret_cast<unsigned long long*>(smem);          // [P]
  StagedBox* boxes = reinterpret_cast<StagedBox*>(claim + P);                       // [G]
  int* added_waves = reinterpret_cast<int*>(boxes + G);                             // [16]
  unsigned short* cand = reinterpret_cast<unsigned short*>(added_waves + 16);       // [G][m]
  const int n = n_gt[b];
  if (status[b] != 0 || n <= 0 || n > G) {                    // skipped: the row stays as it is (mbx_match_extend's rule)
    if (tid == 0 && n_extra) n_extra[b] = 0;
    if (thr_out) for (int j = tid; j < G; j += nt) thr_out[(size_t)b * G + j] = 0.0;
    return;
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
  const float4* dec = decoded + (size_t)b * P;
  const float* cf = conf + (size_t)b * P;

  for (int j = wave; j < n; j += nw) {                        // pass 1
    const StagedBox sb = boxes[j];
    unsigned short* cj = cand + (size_t)j * m;
    unsigned long long last_k = 0ull;                         // every pair is over (0, -1)
    int last_i = -1;
    int taken = 0, total = 0, c = 0;
    unsigned long long low = ~0ull;                           // the smallest t, as bits, among the lane's candidates
    bool first = true;
    do {
      KeepList list;
      list.reset();
      double u;
      for (int p = lane; p < P; p += 128) {                   // two loads in flight, as match_atss_kernel's scan
        const int p1 = p + 64;
        const float4 q0 = priors[p], q1 = priors[p1 < P ? p1 : p];
        const unsigned long long k0 = tal_key(q0, dec, cf, p, sb, alpha_halves, beta, u);
        if (k0 != kTalNoKey) {
          if (~k0 < low) low = ~k0;
          list.offer(k0, p, last_k, last_i);
        }
        if (p1 < P) {
          const unsigned long long k1 = tal_key(q1, dec, cf, p1, sb, alpha_halves, beta, u);
          if (k1 != kTalNoKey) {
            if (~k1 < low) low = ~k1;
            list.offer(k1, p1, last_k, last_i);
          }
        }
      }
      if (first) {                                            // nothing was taken yet: every candidate was eligible
        first = false;
        total = wave_sum(list.eligible);
        c = topk < total ? topk : total;
        if (c == total) break;                                // all of them: no round
      }
      keep_list_rounds(list, c, taken, last_k, last_i);
    } while (taken < c);
    unsigned long long cut_k = ~0ull;                         // every candidate: no pair is over (all ones, INT_MAX)
    int cut_i = 0x7fffffff;
    double thr = 0.0;                                         // no candidate
    if (c < total) {
      cut_k = last_k;
      cut_i = last_i;
      thr = __longlong_as_double((long long)~cut_k);
    } else if (total > 0) {
      thr = __longlong_as_double((long long)wave_min_key(low));
    }
    if (lane == 0 && thr_out) thr_out[(size_t)b * G + j] = thr;
    int cnt = 0;
    if (total > 0) {
      for (int base = 0; base < P; base += 64) {              // the selected priors that are free, in ascending index
        const int p = base + lane;
        bool sel = false;
        double u = 0.0;
        if (p < P) {
          const unsigned long long k = tal_key(priors[p], dec, cf, p, sb, alpha_halves, beta, u);
          sel = k != kTalNoKey && !pair_less(cut_k, cut_i, k, p) && mt[p] < 0;
        }
        const unsigned long long mask = __ballot(sel);
        const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
        if (sel && slot < m) {
          cj[slot] = (unsigned short)p;
          atomicMax(&claim[p], (unsigned long long)__double_as_longlong(u));
        }
        cnt += __popcll(mask);
      }
    }
    for (int t = cnt + lane; t < m; t += 64) cj[t] = kTalNone;
  }
  __syncthreads();

  int added = 0;                                              // pass 2
  for (int e = tid; e < n * m; e += nt) {
    const int p = cand[e];
    if (p == kTalNone) continue;
    const int j = e / m;
    const float4 d = dec[p];
    const Box pe = {(double)d.x, (double)d.y, (double)d.z, (double)d.w};
    const double u = iou_corners(pe, boxes[j].box, boxes[j].area);
    if ((unsigned long long)__double_as_longlong(u) != claim[p]) continue;
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

// The checks of mbx_match_tal that need no GPU, and what the launch is sized by (mbx.h has the formula).
int tal_plan(int P, int G, int topk, int* m_out, int* waves_out, size_t* lds_out) {
  if (P <= 0 || G <= 0 || topk < 1) return MBX_ERR_INVALID_ARG;
  if (P >= (int)kTalNone) return MBX_ERR_UNSUPPORTED;
  const long long m = topk < P ? topk : P;
  const long long lds = 8ll * P + (long long)sizeof(StagedBox) * G + 64 + 2ll * G * m;
  if (lds > 64 * 1024) return MBX_ERR_UNSUPPORTED;
  if (m_out) *m_out = (int)m;
  if (waves_out) *waves_out = G < 16 ? G : 16;
  if (lds_out) *lds_out = (size_t)lds;
  return MBX_OK;
}

}  // namespace

extern "C" int mbx_match_tal_supported(int P, int G, int topk) { return tal_plan(P, G, topk, nullptr, nullptr, nullptr); }

extern "C" int mbx_match_tal(const float* priors, const float* decoded, const float* conf, const float* gt,
                             const int32_t* n_gt, const int32_t* status, int topk, int alpha_halves, int beta, int B, int P,
                             int G, int32_t* match, int32_t* n_extra, double* thr, mbx_stream_t stream) {
  if (!priors || !decoded || !conf || !gt || !n_gt || !status || !match || B < 0) return MBX_ERR_INVALID_ARG;
  if (alpha_halves < 0 || alpha_halves > 8 || beta < 1 || beta > 16) return MBX_ERR_INVALID_ARG;
  int m = 0, waves = 0;
  size_t lds = 0;
  const int plan = tal_plan(P, G, topk, &m, &waves, &lds);
  if (plan != MBX_OK) return plan;
  if (B == 0) return MBX_OK;
  MBX_ENTER();
  hipLaunchKernelGGL(match_tal_kernel, dim3(B), dim3(waves * 64), lds, mbx_s(stream),
                     reinterpret_cast<const float4*>(priors), reinterpret_cast<const float4*>(decoded), conf,
                     reinterpret_cast<const float4*>(gt), n_gt, status, topk, alpha_halves, beta, m, P, G, match, n_extra,
                     thr);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}
