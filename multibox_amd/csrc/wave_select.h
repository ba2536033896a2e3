// Selection inside one wavefront, shared by the matching kernels that run a wavefront per box (loss.hip: match_atss_kernel,
// match_tal.hip: match_tal_kernel): the c smallest (64-bit key, index) pairs of what the 64 lanes offer, found without a sort
// and without LDS traffic.  A strided scan leaves in every lane's registers the kKeepPairs smallest of its own pairs, in
// order (KeepList); each round a 64-lane minimum over the heads of the lists takes the next pair (wave_min_pair) and that
// lane moves on (keep_list_rounds).  Only when a lane has handed out its whole list and had more to offer does the
// wavefront scan again, for the pairs over the last one taken.  The last pair taken is the cut.
#pragma once
#include "common.h"

namespace {

// Lanes of one wavefront hand LDS values to each other without a workgroup barrier (the wavefronts run different numbers
// of boxes): this keeps the compiler from moving LDS accesses across the hand-off; the hardware runs one wavefront's LDS
// instructions in order.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (key, index) pairs in lexicographic order: equal keys go to the lowest index.
__device__ __forceinline__ bool pair_less(unsigned long long ka, int ia, unsigned long long kb, int ib) {
  return ka < kb || (ka == kb && ia < ib);
}

// The smallest (key, index) pair of the wavefront's 64 lanes, in every lane (all 64 active), by data-parallel-primitive
// moves.  A step: every lane takes the value of the lane the control CTRL names and keeps the smaller; a lane the control
// gives no source, or whose row ROW_MASK leaves out, sees the identity (all ones).  A shift scan inside each row of 16
// lanes (row_shr 1, 2, 4, 8), then lane 15 of rows 0 and 2 to rows 1 and 3 (row_bcast15) and lane 31 to rows 2 and 3
// (row_bcast31) leave the minimum in lane 63, which is read out as a wavefront-uniform value.  The 64-bit keys are reduced
// first; one lane holds the smallest key unless keys tie, and only then are the tied lanes' indices reduced too.
// No LDS traffic: the sixteen wavefronts of a workgroup run these rounds at once, and as ds_bpermute shuffles, eighteen a
// round, they all went through the one LDS of the compute unit (539 -> 490 us for ATSS at P = 3199, G = 100; LAB_NOTES).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void dpp_min(unsigned long long& k) {
  const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)(unsigned)k, CTRL, ROW_MASK, 0xf, false);
  const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)(unsigned)(k >> 32), CTRL, ROW_MASK, 0xf, false);
  const unsigned long long ok = ((unsigned long long)ohi << 32) | olo;
  if (ok < k) k = ok;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void dpp_min(int& i) {
  const int oi = __builtin_amdgcn_update_dpp(0x7fffffff, i, CTRL, ROW_MASK, 0xf, false);
  if (oi < i) i = oi;
}
template <typename T>
__device__ __forceinline__ void dpp_min_to_lane63(T& v) {
  dpp_min<0x111, 0xf>(v);
  dpp_min<0x112, 0xf>(v);
  dpp_min<0x114, 0xf>(v);
  dpp_min<0x118, 0xf>(v);
  dpp_min<0x142, 0xa>(v);
  dpp_min<0x143, 0xc>(v);
}

// The smallest key of the 64 lanes, in every lane.
__device__ __forceinline__ unsigned long long wave_min_key(unsigned long long k) {
  dpp_min_to_lane63(k);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ void wave_min_pair(unsigned long long& k, int& i) {
  const unsigned long long mk = wave_min_key(k);
  const unsigned long long tied = __ballot(k == mk);          // never empty: the lane the minimum came from
  int mi;
  if (__popcll(tied) == 1) {
    mi = __builtin_amdgcn_readlane(i, __ffsll((long long)tied) - 1);
  } else {                                                    // equal keys: the lowest index among them
    mi = k == mk ? i : 0x7fffffff;
    dpp_min_to_lane63(mi);
    mi = __builtin_amdgcn_readlane(mi, 63);
  }
  k = mk;
  i = mi;
}

constexpr int kKeepPairs = 4;                                 // pairs a lane keeps from one scan (12 registers)

// One lane's kKeepPairs smallest pairs over the last one taken, ascending; (all ones, INT_MAX) = none.
struct KeepList {
  unsigned long long k[kKeepPairs];
  int i[kKeepPairs];
  int eligible;                                               // how many of the lane's pairs were over the last one taken
  int pops;                                                   // how many it has handed out since the scan

  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int t = 0; t < kKeepPairs; ++t) { k[t] = ~0ull; i[t] = 0x7fffffff; }
    eligible = 0;
    pops = 0;
  }
  // The scan offers every pair of the lane once, in any order; pairs at or under (last_k, last_i) were taken before.
  __device__ __forceinline__ void offer(unsigned long long key, int p, unsigned long long last_k, int last_i) {
    if (!pair_less(last_k, last_i, key, p)) return;
    ++eligible;
    if (!pair_less(key, p, k[kKeepPairs - 1], i[kKeepPairs - 1])) return;
    k[kKeepPairs - 1] = key; i[kKeepPairs - 1] = p;
#pragma unroll
    for (int t = kKeepPairs - 1; t > 0; --t) {
      if (pair_less(k[t], i[t], k[t - 1], i[t - 1])) {
        const unsigned long long sk = k[t]; k[t] = k[t - 1]; k[t - 1] = sk;
        const int si = i[t]; i[t] = i[t - 1]; i[t - 1] = si;
      }
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int t = 0; t + 1 < kKeepPairs; ++t) { k[t] = k[t + 1]; i[t] = i[t + 1]; }
    k[kKeepPairs - 1] = ~0ull; i[kKeepPairs - 1] = 0x7fffffff;
    ++pops;
  }
  // It has handed out its whole list and had more pairs than it could keep: it no longer knows its smallest.
  __device__ __forceinline__ bool spent() const { return pops == kKeepPairs && eligible > kKeepPairs; }
};

// Rounds behind a scan, all 64 lanes: the smallest head of the 64 lists is the next pair, its lane moves on (indices are
// distinct: one lane holds it), until `taken` reaches c or some lane is spent -- then the caller scans again from
// (last_k, last_i).  c is at most the number of pairs on offer, so a round never finds every list empty.
__device__ __forceinline__ void keep_list_rounds(KeepList& list, int c, int& taken, unsigned long long& last_k, int& last_i) {
  while (taken < c) {
    if (__any(list.spent())) break;
    unsigned long long best_k = list.k[0];
    int best_i = list.i[0];
    wave_min_pair(best_k, best_i);
    if (list.i[0] == best_i) list.pop();
    last_k = best_k;
    last_i = best_i;
    ++taken;
  }
}

}  // namespace
