// libmbx: per-image merge of multi-crop detections (greedy NMS across patches + top-N, or Soft-NMS), and box voting on
// what it keeps.
// The reference writes every patch's boxes one after the other (detect.py:408-460) and has no such stage; this one is
// optional and sits behind mbx_decode_filter_topk (+ mbx_nms), reading exactly what they write.  Built with
// -ffp-contract=off: the float64 IoU keeps the operation order of oracle.ref_numpy.nms_greedy, so keep decisions are exact.
#include "boxes.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxCand = MBX_MERGE_MAX_CANDIDATES;
// LDS plan of merge_kernel: keys [16384] u64, kept boxes [max_det][4] f64, kept offsets [max_det] i32, the boxes of one
// chunk of kThreads candidates [kThreads][4] f64.  640 is what fits beside the keys in the 160 KiB of a workgroup.
constexpr int kMergeMaxDet = 640;

// does the EARLIER (kept) box e suppress the later box b of area ab?  oracle.ref_numpy.nms_greedy (boxes.h)
__device__ __forceinline__ bool suppresses(const Box& e, const Box& b, double ab, double thr) {
  return iou_corners(e, b, ab) > thr;
}

__device__ __forceinline__ Box box_shfl(const Box& b, int src) {
  Box r;
  r.x1 = __shfl(b.x1, src, 64); r.y1 = __shfl(b.y1, src, 64);
  r.x2 = __shfl(b.x2, src, 64); r.y2 = __shfl(b.y2, src, 64);
  return r;
}

// One workgroup per image.
//   1. candidates = slots [0, count[r]) of the image's rows; key = order-preserving image of the score's float bits
//      (as decode_filter_topk_kernel: -0 == +0, NaN above everything) << 32 | ~(offset of the slot from the image's first
//      slot): a descending sort gives score descending, ties by ascending flat index.  Bitonic sort in LDS.
//   2. walk the sorted list kThreads candidates at a time: every thread tests its candidate against the kept list as it
//      stands (kept boxes in LDS, broadcast reads); then wave 0 goes through the chunk 64 at a time, tests the survivors
//      against what the chunk itself has added since, resolves the 64 among themselves in order (ballot + shuffle of
//      the next kept box) and appends.  Stops at max_det kept.
//   3. kept boxes / scores / flat indices go out in kept order, unused slots 0 / 0 / -1.
__global__ void __launch_bounds__(kThreads)
merge_kernel(const double* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ count,
             const int32_t* __restrict__ image_rows, int k_max, int max_det, double thr, int use_iou,
             double* __restrict__ out_boxes, float* __restrict__ out_scores, int32_t* __restrict__ out_src,
             int32_t* __restrict__ out_count, int32_t* __restrict__ out_status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char merge_lds[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(merge_lds);       // [kMaxCand]
  Box* kept = reinterpret_cast<Box*>(keys + kMaxCand);                                // [max_det]
  Box* chunk = kept + max_det;                                                        // [kThreads]
  unsigned* kept_rel = reinterpret_cast<unsigned*>(chunk + kThreads);                 // [max_det]
  __shared__ int tile_cnt[kThreads];
  __shared__ int wave_tot[kWaves];
  __shared__ unsigned long long alive_mask[kWaves];
  __shared__ int sh_nk;

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int r0 = image_rows[img], r1 = image_rows[img + 1];
  const long long base = (long long)r0 * k_max;                 // flat index of the image's first slot
  double* ob = out_boxes + (size_t)img * max_det * 4;
  float* os = out_scores + (size_t)img * max_det;
  int32_t* oi = out_src + (size_t)img * max_det;

  // ---- 1. the sorted candidate list (boxes.h)
  if (tid == 0) sh_nk = 0;
  bool too_many;
  const int total = sorted_candidate_keys<kThreads>(scores, count, r0, r1, k_max, keys, tile_cnt, wave_tot, &too_many);

  int nk = 0;
  if (total > 0) {
    if (!use_iou) {
      // ---- 2'. no suppression: the first max_det of the sorted list
      nk = min(total, max_det);
      for (int t = tid; t < nk; t += kThreads) {
        const unsigned rel = ~(unsigned)(keys[t] & 0xffffffffull);
        const double* b = boxes + (size_t)(base + rel) * 4;
        kept[t].x1 = b[0]; kept[t].y1 = b[1]; kept[t].x2 = b[2]; kept[t].y2 = b[3];
        kept_rel[t] = rel;
      }
      __syncthreads();
    } else {
      // ---- 2. greedy walk
      for (int pos = 0; pos < total && nk < max_det; pos += kThreads) {
        const int c = pos + tid;
        const bool valid = c < total;
        Box b = {0.0, 0.0, 0.0, 0.0};
        bool dead = !valid;
        if (valid) {
          const unsigned rel = ~(unsigned)(keys[c] & 0xffffffffull);
          const double* p = boxes + (size_t)(base + rel) * 4;
          b.x1 = p[0]; b.y1 = p[1]; b.x2 = p[2]; b.y2 = p[3];
          const double ab = box_area(b);
          for (int j = 0; j < nk && !dead; ++j) dead = suppresses(kept[j], b, ab, thr);
        }
        chunk[tid] = b;
        const unsigned long long alive_w = __ballot(!dead);
        if (lane == 0) alive_mask[tid >> 6] = alive_w;
        __syncthreads();
        if (tid < 64) {
          const int nk0 = nk;
          int n = nk;
          for (int s = 0; s < kWaves && n < max_det; ++s) {
            unsigned long long alive = alive_mask[s];
            if (alive == 0ull) continue;
            const Box m = chunk[s * 64 + lane];
            const double am = box_area(m);
            bool d = !((alive >> lane) & 1ull);
            for (int j = nk0; j < n && !d; ++j) d = suppresses(kept[j], m, am, thr);     // kept since this chunk began
            alive = __ballot(!d);
            while (alive != 0ull) {
              const int i = __ffsll((long long)alive) - 1;       // the first survivor is kept
              const Box e = box_shfl(m, i);
              if (lane == i) {
                kept[n] = m;
                kept_rel[n] = ~(unsigned)(keys[pos + s * 64 + lane] & 0xffffffffull);
              }
              ++n;
              if (n >= max_det) break;
              if (!d && lane > i) d = suppresses(e, m, am, thr);
              alive = __ballot(!d) & ~(i == 63 ? ~0ull : ((2ull << i) - 1ull));
            }
          }
          if (lane == 0) sh_nk = n;
        }
        __syncthreads();
        nk = sh_nk;
      }
    }
  }

  // ---- 3. outputs
  if (tid == 0) { out_count[img] = nk; out_status[img] = too_many ? 1 : 0; }
  for (int t = tid; t < max_det; t += kThreads) {
    if (t < nk) {
      const long long flat = base + kept_rel[t];
      const Box b = kept[t];
      ob[t * 4] = b.x1; ob[t * 4 + 1] = b.y1; ob[t * 4 + 2] = b.x2; ob[t * 4 + 3] = b.y2;
      os[t] = scores[flat];
      oi[t] = (int32_t)flat;
    } else {
      ob[t * 4] = ob[t * 4 + 1] = ob[t * 4 + 2] = ob[t * 4 + 3] = 0.0;
      os[t] = 0.f;
      oi[t] = -1;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ box voting
constexpr int kVotePerWave = 2;                        // kept boxes per wavefront: every candidate load serves both
constexpr int kVotePerBlock = kWaves * kVotePerWave;

// One candidate (score w, box b) against the wavefront's kept boxes: the sums of those it votes for.
__device__ __forceinline__ void vote_add(float w, const Box& b, const Box (&e)[kVotePerWave], double vthr,
                                         double (&sw)[kVotePerWave], double (&sx)[kVotePerWave][4], int (&nv)[kVotePerWave]) {
  if (!(w > 0.f && w < INFINITY)) return;                            // NaN, +-0, negatives and +inf do not vote
  const double ab = box_area(b), wd = (double)w;
#pragma unroll
  for (int j = 0; j < kVotePerWave; ++j) {
    if (iou_corners(e[j], b, ab) >= vthr) {
      sw[j] += wd;
      sx[j][0] += wd * b.x1; sx[j][1] += wd * b.y1; sx[j][2] += wd * b.x2; sx[j][3] += wd * b.y2;
      ++nv[j];
    }
  }
}

// Second launch behind merge_kernel, grid (groups of kVotePerBlock kept slots, images): one wavefront per kVotePerWave
// kept boxes of one image.  It reads the kept boxes merge_kernel wrote to out_boxes and ALL candidates of the image
// (slots [0, count[r]) of its rows), keeps per kept box sum(w), sum(w * x_j) and the number of voters in registers, and
// ends with the fixed xor tree of wave_sum.  The rows are taken kVoteRows at a time: lane l first takes slot l of
// each of them (their loads are issued together: a row of the usual 50 candidates is one pass, and one load's latency
// per row was most of the kernel's time), then slots l + 64, l + 128, ... of each.  So the order of the sums depends
// on the image's own rows only.  Each wavefront writes the slots it read and no other.
constexpr int kVoteRows = 4;
static_assert(64 % kVoteRows == 0, "a group of rows does not wrap around the 64 counts a wavefront holds");

__global__ void __launch_bounds__(kThreads)
vote_kernel(const double* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ count,
            const int32_t* __restrict__ image_rows, int img0, int k_max, int max_det, double vthr,
            double* out_boxes, const int32_t* __restrict__ out_count, int32_t* __restrict__ out_votes) {
  const int img = img0 + blockIdx.y, lane = threadIdx.x & 63;
  const int k0 = (blockIdx.x * kWaves + (threadIdx.x >> 6)) * kVotePerWave;
  if (k0 >= max_det) return;
  const int nk = min(max(out_count[img], 0), max_det);
  double* ob = out_boxes + (size_t)img * max_det * 4;
  int32_t* ov = out_votes + (size_t)img * max_det;
  if (k0 >= nk) {                                                    // unused slots: boxes are merge_kernel's zeros
    if (lane < kVotePerWave && k0 + lane < max_det) ov[k0 + lane] = 0;
    return;
  }
  Box e[kVotePerWave];
  double sw[kVotePerWave], sx[kVotePerWave][4];
  int nv[kVotePerWave];
#pragma unroll
  for (int q = 0; q < kVotePerWave; ++q) {
    const int k = min(k0 + q, nk - 1);                               // (a slot past nk repeats the last box; not written)
    e[q].x1 = ob[k * 4]; e[q].y1 = ob[k * 4 + 1]; e[q].x2 = ob[k * 4 + 2]; e[q].y2 = ob[k * 4 + 3];
    sw[q] = sx[q][0] = sx[q][1] = sx[q][2] = sx[q][3] = 0.0;
    nv[q] = 0;
  }
  const int r0 = image_rows[img], r1 = image_rows[img + 1];
  for (int t0 = r0; t0 < r1; t0 += 64) {
    const int nrows = min(64, r1 - t0);
    const int my_cnt = lane < nrows ? min(max(count[t0 + lane], 0), k_max) : 0;      // 64 rows' counts, one load
    for (int q = 0; q < nrows; q += kVoteRows) {
      int c[kVoteRows];
      float w[kVoteRows];
      Box b[kVoteRows];
#pragma unroll
      for (int u = 0; u < kVoteRows; ++u) {                          // slot `lane` of kVoteRows rows (rows past nrows: count 0)
        c[u] = __shfl(my_cnt, (q + u) & 63, 64);
        w[u] = 0.f;
        b[u].x1 = b[u].y1 = b[u].x2 = b[u].y2 = 0.0;
        if (lane < c[u]) {
          const size_t at = (size_t)(t0 + q + u) * k_max + lane;
          w[u] = scores[at];
          b[u].x1 = boxes[at * 4]; b[u].y1 = boxes[at * 4 + 1]; b[u].x2 = boxes[at * 4 + 2]; b[u].y2 = boxes[at * 4 + 3];
        }
      }
#pragma unroll
      for (int u = 0; u < kVoteRows; ++u) vote_add(w[u], b[u], e, vthr, sw, sx, nv);      // (w = 0 where there is no slot)
#pragma unroll
      for (int u = 0; u < kVoteRows; ++u) {                          // what a row has beyond 64 candidates
        for (int s = lane + 64; s < c[u]; s += 64) {
          const size_t at = (size_t)(t0 + q + u) * k_max + s;
          Box bb;
          bb.x1 = boxes[at * 4]; bb.y1 = boxes[at * 4 + 1]; bb.x2 = boxes[at * 4 + 2]; bb.y2 = boxes[at * 4 + 3];
          vote_add(scores[at], bb, e, vthr, sw, sx, nv);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kVotePerWave; ++q) {
    const int n = wave_sum(nv[q]);
    const double w = wave_sum(sw[q]);
    const double x1 = wave_sum(sx[q][0]), y1 = wave_sum(sx[q][1]);
    const double x2 = wave_sum(sx[q][2]), y2 = wave_sum(sx[q][3]);
    const int k = k0 + q;
    if (lane == 0 && k < max_det) {
      const bool used = k < nk;
      ov[k] = used ? n : 0;
      if (used && n > 0) { ob[k * 4] = x1 / w; ob[k * 4 + 1] = y1 / w; ob[k * 4 + 2] = x2 / w; ob[k * 4 + 3] = y2 / w; }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- Soft-NMS
// One workgroup of kSoftThreads per image; thread `tid` owns the candidates j = tid + k * kSoftThreads, k < kSoftPer, of
// the image's list (rows in order, slots ascending: j ascending is flat index ascending).  Their working scores t live in
// dynamic LDS, [kMaxCand] float64 = 128 KiB; their offsets from the image's first slot live in kSoftPer registers (the
// 64 KiB a list of them would need do not fit beside the scores), indexed by the loop counter, which is uniform.
constexpr int kSoftThreads = 1024;
constexpr int kSoftWaves = kSoftThreads / 64;
constexpr int kSoftPer = kMaxCand / kSoftThreads;
constexpr int kSoftBatch = 2;                          // candidates whose box loads are issued together
static_assert(kSoftPer * kSoftThreads == kMaxCand && kSoftPer % kSoftBatch == 0, "every candidate has an owner");

// What a wavefront found: the order-preserving image of its best live score, whose that is, and its box.
struct SoftBest { unsigned long long key; unsigned rel; unsigned pad; Box box; };

// (key, rel) of a live candidate is better when its score is larger, of bit-equal scores when its flat index is lower.
// A live t is positive and finite, so its bits order as u64 like the value; key 0 = nobody.
__device__ __forceinline__ bool soft_better(unsigned long long ka, unsigned ra, unsigned long long kb, unsigned rb) {
  return ka > kb || (ka == kb && ra < rb);
}
__device__ __forceinline__ bool soft_live(double t, double min_score) { return t > min_score && t < INFINITY; }

// The weight of the definition (include/mbx.h) for an IoU o: every operation rounded once, in this order.
template <int METHOD>
__device__ __forceinline__ double soft_weight(double o, double thr, double sigma) {
  if (METHOD == MBX_SOFT_LINEAR) return o > thr ? 1.0 - o : 1.0;
  const double q = (o * o) / sigma;
  return exp(-q);
}

//   1. candidate list as merge_kernel 1b, without the sort: offsets to LDS (in the room of the scores, which are not
//      there yet), from there to the owners' registers; t = (double)score where that is live, else 0 (= not live, for
//      good: a picked candidate gets it too).
//   2. per pick: wave argmax by shuffles, the wave's winner writes (key, offset, box) to the wave's slot, ONE barrier,
//      every thread reads the kSoftWaves slots and knows the pick (the slots alternate between two sets, so the next
//      round's writes need no second barrier); thread 0 writes the pick out; then every thread decays its live
//      candidates against the pick's box -- boxes re-read from global memory -- and tracks its best on the way.
//      o == 0 gives the weight exactly 1 under both methods and is skipped.
//   3. unused output slots 0 / 0 / -1.
// t_c is a product over the picks in pick order whoever owns c, so the result is a function of the image's rows only.
template <int METHOD>
__global__ void __launch_bounds__(kSoftThreads)
soft_merge_kernel(const double* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ count,
                  const int32_t* __restrict__ image_rows, int k_max, int max_det, double thr, double sigma, double min_score,
                  double* __restrict__ out_boxes, float* __restrict__ out_scores, int32_t* __restrict__ out_src,
                  int32_t* __restrict__ out_count, int32_t* __restrict__ out_status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char merge_lds[];
  double* ts = reinterpret_cast<double*>(merge_lds);                                  // [kMaxCand]
  unsigned* rel_list = reinterpret_cast<unsigned*>(merge_lds);                        // [kMaxCand], step 1 only
  __shared__ int tile_cnt[kSoftThreads];
  __shared__ int wave_tot[kSoftWaves];
  __shared__ SoftBest wave_best[2][kSoftWaves];

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = image_rows[img], r1 = image_rows[img + 1];
  const long long base = (long long)r0 * k_max;                 // flat index of the image's first slot
  double* ob = out_boxes + (size_t)img * max_det * 4;
  float* os = out_scores + (size_t)img * max_det;
  int32_t* oi = out_src + (size_t)img * max_det;

  // ---- 1a. number of candidates
  int mine = 0;
  for (int r = r0 + tid; r < r1; r += kSoftThreads) mine += min(max(count[r], 0), k_max);
  mine = wave_sum(mine);
  if (lane == 0) wave_tot[wave] = mine;
  __syncthreads();
  int total = 0;
  for (int w = 0; w < kSoftWaves; ++w) total += wave_tot[w];
  const bool too_many = total > kMaxCand;
  if (too_many) total = 0;
  total = __builtin_amdgcn_readfirstlane(total);

  int nk = 0;
  if (total > 0) {
    // ---- 1b. offsets of the candidates, in list order
    int off = 0;
    for (int t0 = r0; t0 < r1; t0 += kSoftThreads) {
      const int nrows = min(kSoftThreads, r1 - t0);
      __syncthreads();                                           // the previous tile's counts have been read
      if (tid < nrows) tile_cnt[tid] = min(max(count[t0 + tid], 0), k_max);
      __syncthreads();
      for (int q = 0; q < nrows; ++q) {
        const int c = tile_cnt[q];
        const unsigned rel0 = (unsigned)(t0 + q - r0) * (unsigned)k_max;
        for (int s = tid; s < c; s += kSoftThreads) rel_list[off + s] = rel0 + (unsigned)s;
        off += c;
      }
    }
    __syncthreads();
    unsigned rel[kSoftPer];
#pragma unroll
    for (int k = 0; k < kSoftPer; ++k) {
      const int j = k * kSoftThreads + tid;
      rel[k] = j < total ? rel_list[j] : 0xffffffffu;
    }
    __syncthreads();                                             // the offsets are in registers: the room is the scores' now

    // ---- 1c. working scores, and the first argmax
    unsigned long long bkey = 0ull;
    unsigned brel = 0xffffffffu;
    Box bbox = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kSoftPer; ++k) {
      const int j = k * kSoftThreads + tid;
      if (k * kSoftThreads < total && j < total) {
        double t = (double)scores[base + rel[k]];
        if (!soft_live(t, min_score)) t = 0.0;
        ts[j] = t;
        const unsigned long long key = (unsigned long long)__double_as_longlong(t);
        if (soft_better(key, rel[k], bkey, brel)) {
          const double* p = boxes + (size_t)(base + rel[k]) * 4;
          bkey = key; brel = rel[k];
          bbox.x1 = p[0]; bbox.y1 = p[1]; bbox.x2 = p[2]; bbox.y2 = p[3];
        }
      }
    }

    // ---- 2. picks
    for (;;) {
      // the wave's best, every lane
      unsigned long long wkey = bkey;
      unsigned wrel = brel;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ok = __shfl_xor(wkey, o, 64);
        const unsigned orl = __shfl_xor(wrel, o, 64);
        if (soft_better(ok, orl, wkey, wrel)) { wkey = ok; wrel = orl; }
      }
      SoftBest* slots = wave_best[nk & 1];
      if (wkey == 0ull) {
        if (lane == 0) { slots[wave].key = 0ull; slots[wave].rel = 0xffffffffu; }
      } else if (brel == wrel) {                                 // one lane: offsets are distinct
        slots[wave].key = wkey; slots[wave].rel = wrel; slots[wave].box = bbox;
      }
      __syncthreads();
      int win = 0;
      unsigned long long pkey = slots[0].key;
      unsigned prel = slots[0].rel;
#pragma unroll
      for (int w = 1; w < kSoftWaves; ++w) {
        const unsigned long long ok = slots[w].key;
        const unsigned orl = slots[w].rel;
        if (soft_better(ok, orl, pkey, prel)) { pkey = ok; prel = orl; win = w; }
      }
      if (pkey == 0ull) break;                                   // nobody is live
      const Box pb = slots[win].box;
      if (tid == 0) {
        const long long flat = base + prel;
        ob[nk * 4] = pb.x1; ob[nk * 4 + 1] = pb.y1; ob[nk * 4 + 2] = pb.x2; ob[nk * 4 + 3] = pb.y2;
        os[nk] = (float)__longlong_as_double((long long)pkey);
        oi[nk] = (int32_t)flat;
      }
      ++nk;
      if (nk >= max_det) break;

      // decay against the pick, and the next argmax
      bkey = 0ull; brel = 0xffffffffu;
      for (int k0 = 0; k0 < kSoftPer && k0 * kSoftThreads < total; k0 += kSoftBatch) {      // (uniform)
        double t[kSoftBatch];
        Box c[kSoftBatch];
        bool live[kSoftBatch];
#pragma unroll
        for (int u = 0; u < kSoftBatch; ++u) {
          const int j = (k0 + u) * kSoftThreads + tid;
          t[u] = j < total ? ts[j] : 0.0;
          live[u] = t[u] > 0.0;
          c[u].x1 = c[u].y1 = c[u].x2 = c[u].y2 = 0.0;
          if (live[u] && rel[k0 + u] == prel) {                  // the pick leaves the live set
            ts[j] = 0.0;
            live[u] = false;
          }
          if (live[u]) {
            const double* p = boxes + (size_t)(base + rel[k0 + u]) * 4;
            c[u].x1 = p[0]; c[u].y1 = p[1]; c[u].x2 = p[2]; c[u].y2 = p[3];
          }
        }
#pragma unroll
        for (int u = 0; u < kSoftBatch; ++u) {
          if (!live[u]) continue;
          const int j = (k0 + u) * kSoftThreads + tid;
          const double o = iou_corners(pb, c[u], box_area(c[u]));
          double tn = t[u];
          if (o != 0.0) {
            tn = tn * soft_weight<METHOD>(o, thr, sigma);
            if (!soft_live(tn, min_score)) tn = 0.0;
            ts[j] = tn;
          }
          const unsigned long long key = (unsigned long long)__double_as_longlong(tn);
          if (soft_better(key, rel[k0 + u], bkey, brel)) { bkey = key; brel = rel[k0 + u]; bbox = c[u]; }
        }
      }
    }
  }

  // ---- 3. count, status and the unused slots
  if (tid == 0) { out_count[img] = nk; out_status[img] = too_many ? 1 : 0; }
  for (int t = nk + tid; t < max_det; t += kSoftThreads) {
    ob[t * 4] = ob[t * 4 + 1] = ob[t * 4 + 2] = ob[t * 4 + 3] = 0.0;
    os[t] = 0.f;
    oi[t] = -1;
  }
}

// The vote launches behind a kernel that has written the kept boxes and out_count (vote_kernel's grid: groups of
// kVotePerBlock kept slots x at most 65 535 images).
int launch_votes(const double* boxes, const float* scores, const int32_t* count, const int32_t* image_rows, int I, int k_max,
                 int max_det, double vote_iou_threshold, double* out_boxes, const int32_t* out_count, int32_t* out_votes,
                 mbx_stream_t stream) {
  MBX_ENTER();
  const int groups = (max_det + kVotePerBlock - 1) / kVotePerBlock;
  for (int i0 = 0; i0 < I;) {
    const int ni = I - i0 < 65535 ? I - i0 : 65535;                     // (the y extent of a grid)
    hipLaunchKernelGGL(vote_kernel, dim3(groups, ni), dim3(kThreads), 0, mbx_s(stream), boxes, scores, count, image_rows,
                       i0, k_max, max_det, vote_iou_threshold, out_boxes, out_count, out_votes);
    MBX_LAUNCH_CHECK();
    i0 += ni;
  }
  return MBX_OK;
}

}  // namespace

extern "C" int mbx_merge_detections(const double* boxes, const float* scores, const int32_t* count,
                                    const int32_t* image_rows, int I, int k_max, int max_det, double iou_threshold,
                                    double* out_boxes, float* out_scores, int32_t* out_src, int32_t* out_count,
                                    int32_t* out_status, mbx_stream_t stream) {
  if (!boxes || !scores || !count || !image_rows || !out_boxes || !out_scores || !out_src || !out_count || !out_status)
    return MBX_ERR_INVALID_ARG;
  if (I < 0 || k_max <= 0 || max_det <= 0) return MBX_ERR_INVALID_ARG;
  if (max_det > kMergeMaxDet) return MBX_ERR_UNSUPPORTED;
  if (I == 0) return MBX_OK;
  const size_t lds = (size_t)kMaxCand * sizeof(unsigned long long) + ((size_t)max_det + kThreads) * sizeof(Box) +
                     (size_t)max_det * sizeof(unsigned);
  const int use_iou = !(isinf(iou_threshold) && iou_threshold > 0.0);
  MBX_ENTER();
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess) return MBX_ERR_LAUNCH;
  hipLaunchKernelGGL(merge_kernel, dim3(I), dim3(kThreads), lds, mbx_s(stream), boxes, scores, count, image_rows, k_max,
                     max_det, iou_threshold, use_iou, out_boxes, out_scores, out_src, out_count, out_status);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_merge_detections_voted(const double* boxes, const float* scores, const int32_t* count,
                                          const int32_t* image_rows, int I, int k_max, int max_det, double iou_threshold,
                                          double vote_iou_threshold, double* out_boxes, float* out_scores,
                                          int32_t* out_src, int32_t* out_count, int32_t* out_status, int32_t* out_votes,
                                          mbx_stream_t stream) {
  if (!out_votes) return MBX_ERR_INVALID_ARG;
  if (!(vote_iou_threshold > 0.0 && vote_iou_threshold <= 1.0)) return MBX_ERR_INVALID_ARG;       // a NaN too
  // the kept list: the plain merge itself, its argument checks included
  const int rc = mbx_merge_detections(boxes, scores, count, image_rows, I, k_max, max_det, iou_threshold, out_boxes,
                                      out_scores, out_src, out_count, out_status, stream);
  if (rc != MBX_OK || I == 0) return rc;
  return launch_votes(boxes, scores, count, image_rows, I, k_max, max_det, vote_iou_threshold, out_boxes, out_count, out_votes,
                      stream);
}

extern "C" int mbx_merge_detections_soft(const double* boxes, const float* scores, const int32_t* count,
                                         const int32_t* image_rows, int I, int k_max, int max_det, int method,
                                         double iou_threshold, double sigma, double min_score, double vote_iou_threshold,
                                         double* out_boxes, float* out_scores, int32_t* out_src, int32_t* out_count,
                                         int32_t* out_status, int32_t* out_votes, mbx_stream_t stream) {
  if (!boxes || !scores || !count || !image_rows || !out_boxes || !out_scores || !out_src || !out_count || !out_status)
    return MBX_ERR_INVALID_ARG;
  if (I < 0 || k_max <= 0 || max_det <= 0) return MBX_ERR_INVALID_ARG;
  if (method == MBX_SOFT_LINEAR) {
    if (isnan(iou_threshold)) return MBX_ERR_INVALID_ARG;
  } else if (method == MBX_SOFT_GAUSSIAN) {
    if (!(sigma > 0.0 && sigma < INFINITY)) return MBX_ERR_INVALID_ARG;                            // a NaN too
  } else {
    return MBX_ERR_INVALID_ARG;
  }
  if (!(min_score >= 0.0 && min_score < INFINITY)) return MBX_ERR_INVALID_ARG;                     // a NaN too
  if (!(vote_iou_threshold >= 0.0 && vote_iou_threshold <= 1.0)) return MBX_ERR_INVALID_ARG;       // a NaN too
  const bool vote = vote_iou_threshold > 0.0;
  if (vote && !out_votes) return MBX_ERR_INVALID_ARG;
  if (max_det > kMergeMaxDet) return MBX_ERR_UNSUPPORTED;
  if (I == 0) return MBX_OK;
  const size_t lds = (size_t)kMaxCand * sizeof(double);
  const auto kernel = method == MBX_SOFT_LINEAR ? soft_merge_kernel<MBX_SOFT_LINEAR> : soft_merge_kernel<MBX_SOFT_GAUSSIAN>;
  MBX_ENTER();
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess) return MBX_ERR_LAUNCH;
  hipLaunchKernelGGL(kernel, dim3(I), dim3(kSoftThreads), lds, mbx_s(stream), boxes, scores, count, image_rows, k_max, max_det,
                     iou_threshold, sigma, min_score, out_boxes, out_scores, out_src, out_count, out_status);
  MBX_LAUNCH_CHECK();
  if (!vote) return MBX_OK;
  return launch_votes(boxes, scores, count, image_rows, I, k_max, max_det, vote_iou_threshold, out_boxes, out_count, out_votes,
                      stream);
}
