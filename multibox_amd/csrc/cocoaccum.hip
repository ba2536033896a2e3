// libmbx: accumulation of the COCO bounding-box metric (pycocotools' COCOeval.accumulate for one category, as
// multibox_amd/cocoeval.py:accumulate_tables restates it) on the outputs of mbx_coco_match: one global stable sort of the
// detections by score, running tp / fp counts per (IoU threshold, area range, maxDets) slice, the running maximum of the
// precision from the right and one lower-bound search per recall threshold.  Everything but the final float64 divisions
// is integer work; built with -ffp-contract=off like cocomatch.hip, the divisions are the host's, bit for bit.
//
// Device-wide steps are separate launches on the caller's stream (no workgroup ever waits on another):
//   sort     tile sort in LDS (bitonic on the unique pair (score key, original index)), then merge passes in which every
//            element finds its place by a binary search in the sibling run
//   gather   per sorted position: its slot within its image and one tp bit and one fp bit per (area range, threshold)
//   count    per chunk of kChunk positions and slice: (tp, fp) totals; then a prefix sum of the totals per slice
//   max      per chunk and slice: the maximum precision; then an exclusive suffix maximum over the chunks per slice
//   search   per (slice, recall threshold): lower bound over the chunk prefixes, then inside the one chunk it lands in
#include "common.h"
#include <math.h>

namespace {

constexpr int kMaxDet = MBX_COCO_MAX_DET;
constexpr int kMaxT = 16;
constexpr int kMaxA = 8;
constexpr int kMaxR = MBX_COCO_ACC_MAX_R;
constexpr int kMaxM = MBX_COCO_ACC_MAX_M;
constexpr int kChunk = MBX_COCO_ACC_CHUNK;            // positions per chunk: one wavefront, kIts rounds of 64
constexpr int kIts = kChunk / 64;
constexpr int kTile = MBX_COCO_ACC_SORT_TILE;         // elements one workgroup sorts in LDS
constexpr int kNoSlot = 255;                          // a position that takes part in no slice
constexpr double kEps = 2.220446049250313e-16;        // np.spacing(1)
static_assert(kChunk == 256 && kTile == 1024 && kMaxDet < kNoSlot, "the kernels below are written for these");

// the HOST arrays of the entry point, by value
struct AccParams { double thr[kMaxR]; int32_t md[kMaxM]; };

struct Layout { size_t key[2], idx[2], tpw, fpw, slot, tot, cmax, npig, total; };

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

Layout layout(long long nd, int T, int A, int M) {
  const size_t n = (size_t)nd, nch = (n + kChunk - 1) / kChunk, P = (size_t)T * A, W = (P + 31) / 32, S = P * M;
  Layout l;
  size_t o = 0;
  l.key[0] = o; o += up256(n * 8);
  l.key[1] = o; o += up256(n * 8);
  l.idx[0] = o; o += up256(n * 4);
  l.idx[1] = o; o += up256(n * 4);
  l.tpw = o; o += up256(W * n * 4);
  l.fpw = o; o += up256(W * n * 4);
  l.slot = o; o += up256(n);
  l.tot = o; o += up256(S * (nch + 1) * 8);
  l.cmax = o; o += up256(S * nch * 8);
  l.npig = o; o += up256((size_t)kMaxA * 8);
  l.total = o;
  return l;
}

// Ascending key = descending score; -0.0 counts as +0.0 (the host compares them as equal).
__device__ __forceinline__ uint64_t score_key(double s) {
  if (s == 0.0) s = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(s);
  const uint64_t asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  return ~asc;
}

__global__ void __launch_bounds__(256) acc_fill_kernel(double* __restrict__ precision, int np, double* __restrict__ recall, int nr) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < np) precision[e] = -1.0;
  if (e < nr) recall[e] = -1.0;
}

// npig[a] = sum over the images of n_gt_counted[i, a]; one workgroup per area range
__global__ void __launch_bounds__(256) acc_npig_kernel(const int32_t* __restrict__ n_gt_counted, int I, int A, long long* __restrict__ npig) {
  __shared__ long long part[256];
  const int a = blockIdx.x, tid = threadIdx.x;
  long long s = 0;
  for (int i = tid; i < I; i += 256) s += n_gt_counted[(size_t)i * A + a];
  part[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  if (tid == 0) npig[a] = part[0];
}

// ---- sort
__global__ void __launch_bounds__(256) acc_tile_sort_kernel(const double* __restrict__ dt, int n, uint64_t* __restrict__ key,
                                                            uint32_t* __restrict__ idx) {
  __shared__ uint64_t sk[kTile];
  __shared__ uint32_t si[kTile];
  const int base = blockIdx.x * kTile, tid = threadIdx.x;
  for (int e = tid; e < kTile; e += 256) {
    const int j = base + e;
    const bool ok = j < n;
    sk[e] = ok ? score_key(dt[(size_t)j * 5 + 4]) : ~0ull;               // padding sorts last: no real index is 2^32 - 1
    si[e] = ok ? (uint32_t)j : 0xFFFFFFFFu;
  }
  __syncthreads();
  for (int k = 2; k <= kTile; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < kTile / 2; i += 256) {
        const int e = ((i & ~(j - 1)) << 1) | (i & (j - 1)), p = e | j;
        const bool up = (e & k) == 0;
        const uint64_t k0 = sk[e], k1 = sk[p];
        const uint32_t i0 = si[e], i1 = si[p];
        const bool gt = k0 > k1 || (k0 == k1 && i0 > i1);
        if (gt == up) { sk[e] = k1; sk[p] = k0; si[e] = i1; si[p] = i0; }
      }
      __syncthreads();
    }
  }
  for (int e = tid; e < kTile; e += 256) {
    const int j = base + e;
    if (j < n) { key[j] = sk[e]; idx[j] = si[e]; }
  }
}

// Runs of w = 1 << lw elements are sorted; merge them in pairs.  An element's place is its offset in its own run plus the
// number of smaller elements in the sibling run (the pairs (key, index) are all different).  Always < n.
__global__ void __launch_bounds__(256) acc_merge_kernel(const uint64_t* __restrict__ ks, const uint32_t* __restrict__ is,
                                                        uint64_t* __restrict__ kd, uint32_t* __restrict__ id, int n, int lw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int w = 1 << lw, run = e >> lw, pair0 = (run & ~1) << lw, mid = pair0 + w;
  const uint64_t k = ks[e];
  const uint32_t ix = is[e];
  int lo, hi;
  if (run & 1) { lo = pair0; hi = mid; } else { lo = min(mid, n); hi = min(mid + w, n); }
  const int sib0 = lo;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    const uint64_t km = ks[m];
    const uint32_t im = is[m];
    if (km < k || (km == k && im < ix)) lo = m + 1; else hi = m;
  }
  const int dest = pair0 + (e - ((run & 1) ? mid : pair0)) + (lo - sib0);
  kd[dest] = k;
  id[dest] = ix;
}

// ---- gather: workgroup y builds word y (pairs q = a * T + t in [32 y, 32 y + 32)) of every position's tp and fp bits
__global__ void __launch_bounds__(256) acc_gather_kernel(const uint32_t* __restrict__ idx, const int32_t* __restrict__ dt_rows, int I,
                                                         int n, const int16_t* __restrict__ match, const uint8_t* __restrict__ ignore,
                                                         int P, uint32_t* __restrict__ tpw, uint32_t* __restrict__ fpw,
                                                         uint8_t* __restrict__ slot) {
  const int p = blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
  if (p >= n) return;
  const uint32_t j = idx[p];
  int lo = 0, hi = I;                                                 // the first image whose rows begin after j
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if ((int64_t)dt_rows[m] <= (int64_t)j) lo = m + 1; else hi = m;
  }
  const int i = lo - 1;
  int s = -1;
  if (i >= 0 && j < (uint32_t)n) {
    const int64_t d = (int64_t)j - dt_rows[i];
    if (d >= 0 && d < kMaxDet && (int64_t)j < (int64_t)dt_rows[i + 1]) s = (int)d;
  }
  uint32_t tp = 0, fp = 0;
  if (s >= 0) {
    const size_t base = ((size_t)i * P + (size_t)w * 32) * kMaxDet + s;
    const int nb = min(32, P - w * 32);
    for (int b = 0; b < nb; ++b) {
      const bool m = match[base + (size_t)b * kMaxDet] >= 0;
      const bool ig = ignore[base + (size_t)b * kMaxDet] != 0;
      tp |= (uint32_t)(m && !ig) << b;
      fp |= (uint32_t)(!m && !ig) << b;
    }
  }
  tpw[(size_t)w * n + p] = tp;
  fpw[(size_t)w * n + p] = fp;
  if (w == 0) slot[p] = (uint8_t)(s < 0 ? kNoSlot : s);
}

// ---- count: one wavefront per (chunk, word); tot[slice][c + 1] = the chunk's (tp, fp), slice = (a * T + t) * M + m
__global__ void __launch_bounds__(256) acc_count_kernel(const uint32_t* __restrict__ tpw, const uint32_t* __restrict__ fpw,
                                                        const uint8_t* __restrict__ slot, int n, int nch, int P, int M, AccParams prm,
                                                        int2* __restrict__ tot) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), w = blockIdx.y;
  if (c >= nch) return;
  uint32_t tw[kIts], fw[kIts];
  int sl[kIts];
#pragma unroll
  for (int it = 0; it < kIts; ++it) {
    const int p = c * kChunk + it * 64 + lane;
    const bool ok = p < n;
    tw[it] = ok ? tpw[(size_t)w * n + p] : 0u;
    fw[it] = ok ? fpw[(size_t)w * n + p] : 0u;
    sl[it] = ok ? (int)slot[p] : kNoSlot;
  }
  const int nb = min(32, P - w * 32);
  for (int m = 0; m < M; ++m) {
    const int md = prm.md[m];
    uint64_t part[kIts];
#pragma unroll
    for (int it = 0; it < kIts; ++it) part[it] = __ballot(sl[it] != kNoSlot && sl[it] < md);
    int mytp = 0, myfp = 0;
    for (int b = 0; b < nb; ++b) {
      int ct = 0, cf = 0;
#pragma unroll
      for (int it = 0; it < kIts; ++it) {
        ct += __popcll(__ballot((tw[it] >> b) & 1u) & part[it]);
        cf += __popcll(__ballot((fw[it] >> b) & 1u) & part[it]);
      }
      if (lane == b) { mytp = ct; myfp = cf; }
    }
    if (lane < nb) {
      int2* row = tot + ((size_t)(w * 32 + lane) * M + m) * (size_t)(nch + 1);
      row[c + 1] = make_int2(mytp, myfp);
      if (c == 0) row[0] = make_int2(0, 0);
    }
  }
}

// inclusive prefix sum of tot[slice][1 .. nch]; one workgroup per slice, every thread a contiguous part
__global__ void __launch_bounds__(256) acc_scan_kernel(int2* __restrict__ tot, int nch) {
  __shared__ int stp[256], sfp[256];
  const int tid = threadIdx.x;
  int2* a = tot + (size_t)blockIdx.x * (size_t)(nch + 1) + 1;
  const int seg = (nch + 255) / 256, b0 = min(tid * seg, nch), b1 = min(b0 + seg, nch);
  int tp = 0, fp = 0;
  for (int k = b0; k < b1; ++k) { tp += a[k].x; fp += a[k].y; }
  stp[tid] = tp;
  sfp[tid] = fp;
  __syncthreads();
  tp = fp = 0;
  for (int u = 0; u < tid; ++u) { tp += stp[u]; fp += sfp[u]; }
  for (int k = b0; k < b1; ++k) {
    tp += a[k].x;
    fp += a[k].y;
    a[k] = make_int2(tp, fp);
  }
}

// ---- max: cmax[slice][c] = the largest tp / ((fp + tp) + eps) among the chunk's positions that take part
__global__ void __launch_bounds__(256) acc_max_kernel(const uint32_t* __restrict__ tpw, const uint32_t* __restrict__ fpw,
                                                      const uint8_t* __restrict__ slot, int n, int nch, int P, int M, AccParams prm,
                                                      const int2* __restrict__ tot, double* __restrict__ cmax) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), w = blockIdx.y;
  if (c >= nch) return;
  uint32_t tw[kIts], fw[kIts];
  int sl[kIts];
#pragma unroll
  for (int it = 0; it < kIts; ++it) {
    const int p = c * kChunk + it * 64 + lane;
    const bool ok = p < n;
    tw[it] = ok ? tpw[(size_t)w * n + p] : 0u;
    fw[it] = ok ? fpw[(size_t)w * n + p] : 0u;
    sl[it] = ok ? (int)slot[p] : kNoSlot;
  }
  const uint64_t le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);  // lanes <= this one
  const int nb = min(32, P - w * 32);
  for (int m = 0; m < M; ++m) {
    const int md = prm.md[m];
    uint64_t part[kIts];
#pragma unroll
    for (int it = 0; it < kIts; ++it) part[it] = __ballot(sl[it] != kNoSlot && sl[it] < md);
    double mine = 0.0;
    for (int b = 0; b < nb; ++b) {
      const size_t s = (size_t)(w * 32 + b) * M + m;
      const int2 base = tot[s * (size_t)(nch + 1) + c];
      int tpc = base.x, fpc = base.y;
      double mx = 0.0;
#pragma unroll
      for (int it = 0; it < kIts; ++it) {
        const uint64_t tm = __ballot((tw[it] >> b) & 1u) & part[it], fm = __ballot((fw[it] >> b) & 1u) & part[it];
        const int tpi = tpc + __popcll(tm & le), fpi = fpc + __popcll(fm & le);
        if ((part[it] >> lane) & 1ull) mx = fmax(mx, (double)tpi / (((double)fpi + (double)tpi) + kEps));
        tpc += __popcll(tm);
        fpc += __popcll(fm);
      }
      mx = wave_max(mx);
      if (lane == b) mine = mx;
    }
    if (lane < nb) cmax[((size_t)(w * 32 + lane) * M + m) * (size_t)nch + c] = mine;
  }
}

// cmax[slice][c] <- max over the chunks after c (0 if none: a precision is never negative); one workgroup per slice
__global__ void __launch_bounds__(256) acc_suffix_kernel(double* __restrict__ cmax, int nch) {
  __shared__ double sm[256];
  const int tid = threadIdx.x;
  double* a = cmax + (size_t)blockIdx.x * (size_t)nch;
  const int seg = (nch + 255) / 256, b0 = min(tid * seg, nch), b1 = min(b0 + seg, nch);
  double mx = 0.0;
  for (int k = b0; k < b1; ++k) mx = fmax(mx, a[k]);
  sm[tid] = mx;
  __syncthreads();
  double o = 0.0;
  for (int u = tid + 1; u < 256; ++u) o = fmax(o, sm[u]);
  for (int k = b1 - 1; k >= b0; --k) {
    const double v = a[k];
    a[k] = o;
    o = fmax(o, v);
  }
}

// ---- search: workgroup (slice, group of 4 recall thresholds), one wavefront per threshold.  rc = tp / npig does not
// decrease with tp, so the first position with rc >= thr is found on the integer prefixes with the host's own division.
__global__ void __launch_bounds__(256) acc_search_kernel(const uint32_t* __restrict__ tpw, const uint32_t* __restrict__ fpw,
                                                         const uint8_t* __restrict__ slot, int n, int nch, int T, int A, int M, int R,
                                                         AccParams prm, const int2* __restrict__ tot, const double* __restrict__ sufmax,
                                                         const long long* __restrict__ npig, double* __restrict__ precision,
                                                         double* __restrict__ recall) {
  const int lane = threadIdx.x & 63, s = blockIdx.x, q = s / M, m = s - q * M, a = q / T, t = q - a * T;
  const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
  const long long np = npig[a];
  if (np == 0) return;                                                // the slice stays -1
  const double dn = (double)np;
  const int2* row = tot + (size_t)s * (size_t)(nch + 1);
  if (blockIdx.y == 0 && threadIdx.x == 0) recall[((size_t)t * A + a) * M + m] = (double)(nch ? row[nch].x : 0) / dn;
  if (r >= R) return;
  const double thr = prm.thr[r];
  const int md = prm.md[m], wq = q >> 5, b = q & 31;
  int lo = 0, hi = nch;                                               // the first chunk by whose end rc >= thr
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((double)row[mid + 1].x / dn >= thr) hi = mid; else lo = mid + 1;
  }
  const uint64_t le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  int c = lo;
  bool found = false;
  double mx = 0.0;
  while (c < nch) {                                                   // (a chunk in which nothing takes part: the next one)
    int tpc = row[c].x, fpc = row[c].y;
#pragma unroll
    for (int it = 0; it < kIts; ++it) {
      const int p = c * kChunk + it * 64 + lane;
      const bool ok = p < n;
      const int sl = ok ? (int)slot[p] : kNoSlot;
      const uint32_t tw = ok ? tpw[(size_t)wq * n + p] : 0u, fw = ok ? fpw[(size_t)wq * n + p] : 0u;
      const uint64_t part = __ballot(sl != kNoSlot && sl < md);
      const uint64_t tm = __ballot((tw >> b) & 1u) & part, fm = __ballot((fw >> b) & 1u) & part;
      const int tpi = tpc + __popcll(tm & le), fpi = fpc + __popcll(fm & le);
      const bool mine = (part >> lane) & 1ull;
      const uint64_t hit = __ballot(mine && (double)tpi / dn >= thr);
      const int first = found ? 0 : (hit ? __ffsll((unsigned long long)hit) - 1 : 64);
      if (hit) found = true;
      if (mine && lane >= first) mx = fmax(mx, (double)tpi / (((double)fpi + (double)tpi) + kEps));
      tpc += __popcll(tm);
      fpc += __popcll(fm);
    }
    if (found) break;
    ++c;
  }
  mx = wave_max(mx);
  if (lane == 0) precision[(((size_t)t * R + r) * A + a) * M + m] = found ? fmax(mx, sufmax[(size_t)s * (size_t)nch + c]) : 0.0;
}

bool sizes_ok(int T, int A, int M) { return T >= 1 && T <= kMaxT && A >= 1 && A <= kMaxA && M >= 1 && M <= kMaxM; }

}  // namespace

extern "C" size_t mbx_coco_accumulate_workspace(long long ND, int T, int A, int M) {
  if (ND < 0 || ND > MBX_COCO_ACC_MAX_ND || !sizes_ok(T, A, M)) return 0;
  return layout(ND, T, A, M).total;
}

extern "C" int mbx_coco_accumulate(const double* dt, const int32_t* dt_rows, int I, const int16_t* match, const uint8_t* ignore,
                                   const int32_t* n_gt_counted, int T, int A, const double* rec_thrs, int R,
                                   const int32_t* max_dets, int M, double* precision, double* recall, void* workspace,
                                   size_t workspace_bytes, mbx_stream_t stream) {
  if (!dt || !dt_rows || !match || !ignore || !n_gt_counted || !rec_thrs || !max_dets || !precision || !recall)
    return MBX_ERR_INVALID_ARG;
  if (I < 0 || !sizes_ok(T, A, M) || R < 1 || R > kMaxR) return MBX_ERR_INVALID_ARG;
  hipStream_t st = mbx_s(stream);
  const int n_prec = T * R * A * M, n_rec = T * A * M;
  MBX_ENTER();
  if (I == 0) {
    hipLaunchKernelGGL(acc_fill_kernel, dim3((n_prec + 255) / 256), dim3(256), 0, st, precision, n_prec, recall, n_rec);
    MBX_LAUNCH_CHECK();
    return MBX_OK;
  }
  int32_t nd32 = 0;                                                   // ND = dt_rows[I]: the grids depend on it
  if (hipMemcpyAsync(&nd32, dt_rows + I, sizeof(nd32), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return MBX_ERR_LAUNCH;
  if (nd32 < 0) return MBX_ERR_INVALID_ARG;
  if (nd32 > MBX_COCO_ACC_MAX_ND) return MBX_ERR_UNSUPPORTED;
  const Layout l = layout(nd32, T, A, M);
  if (!workspace || workspace_bytes < l.total) return MBX_ERR_INVALID_ARG;

  AccParams prm = {};
  for (int r = 0; r < R; ++r) prm.thr[r] = rec_thrs[r];
  for (int m = 0; m < M; ++m) prm.md[m] = max_dets[m];
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  uint64_t* key[2] = {reinterpret_cast<uint64_t*>(ws + l.key[0]), reinterpret_cast<uint64_t*>(ws + l.key[1])};
  uint32_t* idx[2] = {reinterpret_cast<uint32_t*>(ws + l.idx[0]), reinterpret_cast<uint32_t*>(ws + l.idx[1])};
  uint32_t* tpw = reinterpret_cast<uint32_t*>(ws + l.tpw);
  uint32_t* fpw = reinterpret_cast<uint32_t*>(ws + l.fpw);
  uint8_t* slot = ws + l.slot;
  int2* tot = reinterpret_cast<int2*>(ws + l.tot);
  double* cmax = reinterpret_cast<double*>(ws + l.cmax);
  long long* npig = reinterpret_cast<long long*>(ws + l.npig);
  const int n = nd32, nch = (n + kChunk - 1) / kChunk, P = T * A, W = (P + 31) / 32, S = P * M;

  hipLaunchKernelGGL(acc_fill_kernel, dim3((n_prec + 255) / 256), dim3(256), 0, st, precision, n_prec, recall, n_rec);
  MBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(acc_npig_kernel, dim3(A), dim3(256), 0, st, n_gt_counted, I, A, npig);
  MBX_LAUNCH_CHECK();
  if (n > 0) {
    const int nblk = (n + 255) / 256;
    hipLaunchKernelGGL(acc_tile_sort_kernel, dim3((n + kTile - 1) / kTile), dim3(256), 0, st, dt, n, key[0], idx[0]);
    MBX_LAUNCH_CHECK();
    int cur = 0;
    for (int lw = 10; (1 << lw) < n; ++lw) {                          // 1 << 10 == kTile
      hipLaunchKernelGGL(acc_merge_kernel, dim3(nblk), dim3(256), 0, st, key[cur], idx[cur], key[cur ^ 1], idx[cur ^ 1], n, lw);
      MBX_LAUNCH_CHECK();
      cur ^= 1;
    }
    hipLaunchKernelGGL(acc_gather_kernel, dim3(nblk, W), dim3(256), 0, st, idx[cur], dt_rows, I, n, match, ignore, P, tpw, fpw, slot);
    MBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(acc_count_kernel, dim3((nch + 3) / 4, W), dim3(256), 0, st, tpw, fpw, slot, n, nch, P, M, prm, tot);
    MBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(acc_scan_kernel, dim3(S), dim3(256), 0, st, tot, nch);
    MBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(acc_max_kernel, dim3((nch + 3) / 4, W), dim3(256), 0, st, tpw, fpw, slot, n, nch, P, M, prm, tot, cmax);
    MBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(acc_suffix_kernel, dim3(S), dim3(256), 0, st, cmax, nch);
    MBX_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(acc_search_kernel, dim3(S, (R + 3) / 4), dim3(256), 0, st, tpw, fpw, slot, n, nch, T, A, M, R, prm, tot, cmax,
                     npig, precision, recall);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}
