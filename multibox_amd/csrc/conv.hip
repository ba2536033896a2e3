// libmbx: implicit-GEMM convolution on MFMA (gfx950), forward + data gradient in one kernel, and conv_impl, the
// dispatcher to the launch families.  NHWC bf16 views, KRSC bf16 filters, fp32 accumulate.  (The weight gradient is
// its own translation unit, wgrad.hip.)
//
// GEMM view (forward):  Y[m, n] = sum_k P[m, k] * W[n, k]
//   m = (img, oh, ow) output pixel, n = output channel, k = (r, s, c) filter tap x input channel.
// The MFMA is issued with the FILTER tile as the A operand and the PIXEL tile as the B operand
// (v_mfma_f32_16x16x32_bf16: D[row = channel][col = pixel]): each lane holds four consecutive channels
// of one pixel.  The fp32 tile is staged through LDS at the end and written row-wise (16 B per lane).
//
// LDS tiles are [rows][64 k] bf16 = 128-B rows of eight 16-B chunks, XOR-swizzled
// (chunk ^ (row & 7)) so the ds_read_b128 fragment reads are bank-conflict free; a 3-deep ring filled
// by LDS-DMA, one barrier per 64-deep K step, two tiles of global latency in flight.
#include <stdlib.h>

#include "conv_common.h"

namespace {

// EV: epilogue variant fixed at compile time (no per-element branching):
//   0 store, 1 store + BN statistics partials, 2 accumulate into y (+ optional relu mask from `skip`),
//   3 affine (+relu), 4 residual (+relu), 5 float32 store, 6 store + batch-norm BACKWARD statistics (data gradients).
// SH: the stride-2 data gradient (input dilated by 2).  Its own instantiation, so that the parity walk below costs
// the other 400 launches per step nothing (as a run-time branch in one kernel it cost them 0.6 ms per step).
// MODE 1: pointwise (1x1, unit stride, no padding) -- the two-instruction address path, no tap walk: 60 % of the launches.
// NSTG: ring depth.  3 = two tiles in flight; 2 = one, for 64 KB of LDS per 128x128 eight-wave block, so that TWO
// blocks share a CU and one's epilogue (HBM-bound: skip read / accumulate / store) overlaps the other's loop.
// (the body is a device function of (problem, block id, number of blocks) so that conv_igemm3_pair_kernel can run TWO
// problems in one grid; conv_igemm3_kernel passes blockIdx.x / gridDim.x)
template <int BM, int BN, int WNW, int WMW, int EV, int MODE = 0, int NSTG = 3>
__device__ __forceinline__ void conv_igemm3_body(const ConvK& p, const int bid_, const int nblk_) {
  constexpr bool SH = MODE == 2, PW = MODE == 1;
  static_assert(WNW * WMW == 4 || WNW * WMW == 8, "four or eight waves");
  constexpr int NT = 64 * WNW * WMW, RPP = NT / 8;      // threads, tile rows filled per DMA pass
  constexpr int TN = BN / WNW, TM = BM / WMW, NI = TN / 16, MI = TM / 16;
  constexpr int PI = BM / RPP, WI = BN / RPP, NL = PI + WI;
  constexpr int STAGE = (BM + BN) * 8;                 // 16-B slots per stage
  extern __shared__ __attribute__((aligned(16))) u32x4 smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id();
  const int wn = wave % WNW, wm = wave / WNW;
  int lid = xcd_remap(bid_, nblk_);
  int split = 0;                                        // split-K slice of this block (float32 partial tiles only)
  if constexpr (EV == 5) { const int nt = p.tiles_m * p.tiles_n; split = lid / nt; lid -= split * nt; }
  const int tile_n = lid % p.tiles_n, tile_m = lid / p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(p.w, p.w_bytes);
  const int lrow = tid >> 3;
  const int chunk = (tid & 7) ^ (lrow & 7);            // source chunk of this lane's LDS slot (pixel tile)
  // The FILTER tile has its own swizzle: its rows are read by the MFMA A operand in a PERMUTED order (see the epilogue:
  // a lane must end up with 8 consecutive output channels), rows 8 (f >> 2) + (f & 3) + 4 (a & 1) + 32 (a >> 1) for
  // fragment row f of block a, and the key ((row >> 3) & 3) << 1 | (row >> 1) & 1 makes exactly those reads
  // bank-conflict free (the 16 lanes a ds_read_b128 services together hit 16 different 16-byte bank groups).
  const int chunkw = (tid & 7) ^ ((((lrow >> 3) & 3) << 1) | ((lrow >> 1) & 1));
  int hb[PI], wb[PI], ro[PI];
#pragma unroll
  for (int i = 0; i < PI; ++i) {
    const int m = m0 + lrow + RPP * i;
    const bool mv = m < p.M;
    const unsigned mm = mv ? (unsigned)m : 0u;
    int img, oh, ow;
    if (SH && p.parity) decode_pixel_parity(p, mm, img, oh, ow); else decode_pixel(p, mm, img, oh, ow);
    hb[i] = mv ? oh * p.mul - p.pad_t : -(1 << 24);
    wb[i] = ow * p.mul - p.pad_l;
    ro[i] = SH ? img * p.x_img_stride * 2 : (img * p.x_img_stride + (hb[i] * p.W_in + wb[i]) * p.ldx) * 2;
    if (PW && !mv) ro[i] = (int)kOOB;
  }
  int wo[WI];
#pragma unroll
  for (int i = 0; i < WI; ++i) {
    const int n = n0 + lrow + RPP * i;
    wo[i] = n < p.C_out ? n * p.Ktot * 2 : -1;
  }

  f32x4 acc[NI][MI];
#pragma unroll
  for (int a = 0; a < NI; ++a)
#pragma unroll
    for (int b = 0; b < MI; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fch = lane >> 4;
  // fragment read offsets (16-B slots): row*8 + ((kk*4 + fch) ^ (row & 7)); row & 7 == frow & 7
  const int fr0 = frow * 8 + (fch ^ (frow & 7));
  const int fr1 = frow * 8 + ((4 + fch) ^ (frow & 7));
  // filter fragments: block a reads tile rows 32 (a >> 1) + 4 (a & 1) + [8 (frow >> 2) + (frow & 3)]  (slot = row * 8 + chunk ^ key)
  const int fwrow = 8 * (frow >> 2) + (frow & 3), fwkey = ((frow >> 2) << 1) | ((frow >> 1) & 1);
  const int fw0 = fwrow * 8 + (fch ^ fwkey);
  const int fw1 = fwrow * 8 + ((4 + fch) ^ fwkey);
  // stride-2 data gradient, tile inside one parity class: only taps with kr = kr0 (mod 2), ks = ks0 (mod 2) meet
  // non-zero rows of the dilated input -- walk those only (steps of 2), a quarter of the K tiles
  int kr0 = 0, ks0 = 0, kstep = 1, nk = (p.Ktot + 63) >> 6;
  if (SH && p.skip_taps) {
    const int mlast = min(m0 + BM, p.M) - 1;
    const int c0 = pixel_class(p, m0);
    if (c0 == pixel_class(p, mlast)) {
      kr0 = (p.pad_t + (c0 >> 1)) & 1;
      ks0 = (p.pad_l + (c0 & 1)) & 1;
      kstep = 2;
      nk = ((p.R - kr0 + 1) >> 1) * ((p.S - ks0 + 1) >> 1) * (p.C_in >> 6);
    }
  }
  int kt0 = 0;                                          // first K step of this block (split-K slices start later)
  if constexpr (EV == 5) { kt0 = split * p.kps; nk = min(p.kps, nk - kt0); }
  int kc = chunk * 8 + kt0 * 64, kr = kr0, ks = ks0;
  while (kc >= p.C_in) { kc -= p.C_in; if ((ks += kstep) >= p.S) { ks = ks0; kr += kstep; } }
  const int ldx2 = p.ldx * 2;
  int st_issue = 0, st_comp = 0;                        // ring positions
  // LDS-DMA of K tile LT into ring slot st_issue.  (A macro, not a lambda: the three call sites must be
  // straight-line code so that the MFMA accumulators never leave the accumulator registers.)
#define MBX_ISSUE_TILE(LT)                                                                                   \
  do {                                                                                                       \
    u32x4* sp = smem + st_issue * STAGE + wave * 64;                                                         \
    const bool kv = kr < p.R;                                                                                \
    if (PW) {                                                                                                \
      _Pragma("unroll") for (int i = 0; i < PI; ++i)                                                         \
        glds16(xr, sp + i * NT, (kv && ro[i] >= 0) ? (ro[i] + kc * 2) : (int)kOOB);                          \
    } else if (!SH) {                                                                                        \
      const int toff = (kr * p.W_in + ks) * ldx2 + kc * 2;                                                   \
      _Pragma("unroll") for (int i = 0; i < PI; ++i) {                                                       \
        const bool ok = kv && ((unsigned)(hb[i] + kr) < (unsigned)p.H_in) &&                                 \
                        ((unsigned)(wb[i] + ks) < (unsigned)p.W_in);                                         \
        glds16(xr, sp + i * NT, ok ? (ro[i] + toff) : (int)kOOB);                                            \
      }                                                                                                      \
    } else {                                                                                                 \
      _Pragma("unroll") for (int i = 0; i < PI; ++i) {                                                       \
        const int hn = hb[i] + kr, wn_ = wb[i] + ks;                                                         \
        const bool ok = kv && (((hn | wn_) & 1) == 0) && ((unsigned)(hn >> 1) < (unsigned)p.H_in) &&         \
                        ((unsigned)(wn_ >> 1) < (unsigned)p.W_in);                                           \
        glds16(xr, sp + i * NT, ok ? (ro[i] + ((hn >> 1) * p.W_in + (wn_ >> 1)) * ldx2 + kc * 2) : (int)kOOB); \
      }                                                                                                      \
    }                                                                                                        \
    /* the filter lane's own K position (its chunk differs from the pixel lane's): linear in K, except in the     \
       tap-skipping walk, where C_in % 64 == 0 and a K tile lies inside one tap */                             \
    const int kb = (SH && kstep == 2) ? ((kr * p.S + ks) * p.C_in + kc + (chunkw - chunk) * 8) * 2                \
                                      : (((LT) + kt0) * 64 + chunkw * 8) * 2;                                  \
    const bool kvw = (SH && kstep == 2) ? kv : (kb < p.Ktot * 2);                                              \
    u32x4* sw = sp + BM * 8;                                                                                 \
    _Pragma("unroll") for (int i = 0; i < WI; ++i)                                                           \
      glds16(wr, sw + i * NT, (kvw && wo[i] >= 0) ? (wo[i] + kb) : (int)kOOB);                               \
    kc += 64;                                                                                                \
    while (kc >= p.C_in) { kc -= p.C_in; if ((ks += kstep) >= p.S) { ks = ks0; kr += kstep; } }              \
    st_issue = st_issue == NSTG - 1 ? 0 : st_issue + 1;                                                      \
  } while (0)

  static_assert(NSTG == 2 || NSTG == 3, "ring depth");
  // LANDING HAND-OFF (every ring in this file and in conv5.hip).  A K tile staged by LDS-DMA is read by OTHER waves.
  // `s_waitcnt vmcnt` (the issuing wave's DMAs have retired) + `s_barrier` turned out NOT to order those reads behind
  // the DMA's LDS write: with another stream's kernels sharing the CUs (input augmentation on a side stream, RCCL in
  // data-parallel runs) a reader saw a slot's PREVIOUS contents about once in 10^5 launches of the 2-deep tiles
  // (round 2: one wave's 32 pixels x 1 channel NaN, then the whole stem; tools/side_stream_stress.py).  The 3-deep
  // rings had the same wait -> barrier -> read distance and were only protected by their DMA being issued a K step
  // earlier -- a timing margin, not an ordering.  The rule now, everywhere: a wave publishes a tile only after it has
  // READ BACK one of its own DMA destinations of that tile (its last piece) and that read has returned
  // (`lgkmcnt(0)`) -- its LDS-DMA writes drain through the LDS pipe in front of the read -- and only then joins the
  // barrier behind which the other waves read.  In the deep rings the wait + read-back of tile it+1 sit in the MIDDLE of
  // step `it` (behind the first half of its MFMAs / of the loaders' DMA issue) so that the read's round trip is hidden;
  // the 2-deep rings, which wait for the tile they have just issued, pay it at the end of the step (+0.2 ms per step).
  u32x4* const probe_base = smem + (PI + WI - 1) * NT + wave * 64 + lane;   // this lane's slot of the wave's LAST piece
  MBX_ISSUE_TILE(0);
  if (NSTG == 3 && nk > 1) { MBX_ISSUE_TILE(1); wait_vmcnt<NL>(); } else wait_vmcnt<0>();
  lds_readback_wait(lds_readback_issue(probe_base));
  raw_barrier();
  for (int it = 0; it < nk; ++it) {
    const bool more = it + NSTG - 1 < nk;
    if (more) MBX_ISSUE_TILE(it + NSTG - 1);
    st_comp = st_comp == NSTG - 1 ? 0 : st_comp + 1;    // now the slot of tile it+1; tile `it` is in st_prev
    const int st_prev = st_comp == 0 ? NSTG - 1 : st_comp - 1;
#ifndef MBX_NO_PROBE_I3                      // (debug builds only: A/B of what the hand-off costs)
    unsigned probe;
    if constexpr (NSTG == 3) {
      // 3-deep: tile it+1 was issued a whole step ago: wait for it HERE (tile it+2 is in flight meanwhile) and start
      // the read-back; it returns while this step's fragments are read and multiplied.  (No control flow may sit
      // inside the MFMA block below: the accumulators would leave the accumulator registers.)
      if (more) wait_vmcnt<NL>(); else wait_vmcnt<0>();
      probe = lds_readback_issue(probe_base + st_comp * STAGE);
    }
#endif
    {                                                   // MFMA on tile `it`
      const u32x4* cP = smem + st_prev * STAGE + (wm * TM) * 8;
      const u32x4* cW = smem + st_prev * STAGE + BM * 8 + (wn * TN) * 8;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int fr = kk ? fr1 : fr0, fw = kk ? fw1 : fw0;
        bf16x8 wf[NI], pf[MI];
#pragma unroll
        for (int a = 0; a < NI; ++a) wf[a] = __builtin_bit_cast(bf16x8, cW[(a >> 1) * 256 + (a & 1) * 32 + fw]);
#pragma unroll
        for (int b = 0; b < MI; ++b) pf[b] = __builtin_bit_cast(bf16x8, cP[b * 128 + fr]);
#pragma unroll
        for (int a = 0; a < NI; ++a)
#pragma unroll
          for (int b = 0; b < MI; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[a], pf[b], acc[a][b], 0, 0, 0);
      }
    }
#ifndef MBX_NO_PROBE_I3
    if constexpr (NSTG == 2) {
      wait_vmcnt<0>();                                  // tile it+1 (issued at the top of this step) has retired
      probe = lds_readback_issue(probe_base + st_comp * STAGE);
    }
    lds_readback_wait(probe);                           // the read-back has returned: publish
#else
    if (NSTG == 3 && more) wait_vmcnt<NL>(); else wait_vmcnt<0>();
#endif
    raw_barrier();
  }
#undef MBX_ISSUE_TILE
  wait_vmcnt<0>();
  // ---------------------------------------------------------------- epilogue: straight from the accumulators
  // acc[a][b][r] = output channel  wn TN + 32 (a >> 1) + 8 fch + 4 (a & 1) + r  of pixel  wm TM + 16 b + frow  (the filter rows
  // were fed to the MFMA in that order): blocks 2A and 2A + 1 together give a lane EIGHT CONSECUTIVE channels of one pixel
  // = one 16-byte bf16 store, and the four lanes of a pixel cover 64 contiguous bytes.  No LDS staging, no barrier, the
  // ring is not needed any more: every global read of the epilogue (residual skip, accumulate source, ReLU mask) is an
  // independent 16-byte load that can be in flight with all the others of the lane (round 2 staged the tile through
  // LDS and walked it row-wise in 16-32 passes, each behind a barrier and each stalled on its own loads -- as long as
  // the K loop on the K <= 448 layers).
  static_assert(NI % 2 == 0, "wave tile: a multiple of 32 output channels");
  constexpr int NA = NI / 2;
  const int cl0 = wn * TN + fch * 8;                           // + 32 A: first of this lane's 8 channels inside the tile
  if constexpr (EV == 5) {
    // float32 head outputs (tiny launches): scalar stores
#pragma unroll
    for (int b = 0; b < MI; ++b) {
      const int m = m0 + wm * TM + b * 16 + frow;
      if (m >= p.M) continue;
      const int img = (int)fast_div((unsigned)m, p.mg_hw, p.sh_hw), pix = m - img * p.HW_out;
      float* yrow = reinterpret_cast<float*>(p.y) + split * p.y_split_stride + img * p.y_img_stride + pix * p.ldy;
#pragma unroll
      for (int a = 0; a < NI; ++a) {
        const int c0 = n0 + cl0 + 32 * (a >> 1) + 4 * (a & 1);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (c0 + r < p.C_out) yrow[c0 + r] = acc[a][b][r];
      }
    }
  } else {
    float s1[NA][8], s2[NA][8];
    // (reads in flight per lane: all of the tile's, or two pixel blocks at a time where that would take > 64 registers)
    conv_epilogue_direct<EV, SH, NI, MI, ((EV == 2 || EV == 6) && MI * NA >= 8 && MI % 2 == 0) ? 2 : MI>(p, acc, m0 + wm * TM + frow, n0 + cl0, s1, s2);
    if constexpr (EV == 1 || EV == 6) {
      // batch-norm statistics partials of this tile (of the STORED, bf16-rounded values), in a fixed order: the lane's
      // MI pixels (above) -> the 16 lanes that share its channels (DPP row sums) -> the WMW waves along the pixel
      // dimension through LDS (the ring is idle: every wave is past the last barrier of the K loop)
      float* red = reinterpret_cast<float*>(smem);             // [WMW][BN][2]
#pragma unroll
      for (int A = 0; A < NA; ++A) { row_sum16_x8(s1[A]); row_sum16_x8(s2[A]); }
#pragma unroll
      for (int A = 0; A < NA; ++A)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float x1 = s1[A][j], x2 = s2[A][j];
          if (frow == 0) {
            red[((wm * BN) + cl0 + 32 * A + j) * 2] = x1;
            red[((wm * BN) + cl0 + 32 * A + j) * 2 + 1] = x2;
          }
        }
      __syncthreads();
      if (tid < BN && n0 + tid < p.C_out) {
        float x1 = 0.f, x2 = 0.f;
#pragma unroll
        for (int w = 0; w < WMW; ++w) { x1 += red[(w * BN + tid) * 2]; x2 += red[(w * BN + tid) * 2 + 1]; }
        if constexpr (EV == 6) bw_stats_write(p, tile_m, n0 + tid, x1, x2); else stats_write(p, tile_m, n0 + tid, x1, x2);
      }
    }
  }
}

template <int BM, int BN, int WNW, int WMW, int EV, int MODE = 0, int NSTG = 3>
__global__ void __launch_bounds__(64 * WNW * WMW)
conv_igemm3_kernel(const ConvK p) {
  conv_igemm3_body<BM, BN, WNW, WMW, EV, MODE, NSTG>(p, (int)blockIdx.x, (int)gridDim.x);
}

// TWO independent problems of the same instantiation in one grid (blocks [0, n0) run p0, the rest p1): the sibling
// convolutions of a batch-norm group (block35's two 3x3 branches, forward and data gradient) are 9-11 us launches that do
// not fill the chip; a kernel costs >= 4.4 us whatever it does.  Same code per block: results bit-identical to two launches.
template <int BM, int BN, int WNW, int WMW, int EV, int MODE = 0, int NSTG = 3>
__global__ void __launch_bounds__(64 * WNW * WMW)
conv_igemm3_pair_kernel(const ConvK p0, const ConvK p1, const int n0) {
  if ((int)blockIdx.x < n0) conv_igemm3_body<BM, BN, WNW, WMW, EV, MODE, NSTG>(p0, (int)blockIdx.x, n0);
  else conv_igemm3_body<BM, BN, WNW, WMW, EV, MODE, NSTG>(p1, (int)blockIdx.x - n0, (int)gridDim.x - n0);
}

// ------------------------------------------------------------------------------------------ split-K reduce
// Long-K convolutions with few output tiles (the 3x3 head convolutions on the 1536-channel feature map: K = 13 824, at most
// 64 tiles of 128 x 64 on 256 CUs) run as `ksplit` K slices per tile -- float32 partial tiles [slice][M][ldp] from the
// float32-store instantiation of conv_igemm3_kernel -- and this kernel adds the slices IN SLICE ORDER (deterministic),
// rounds to bf16, stores y and writes the batch-norm statistics partials of the stored values (one row of [C][2] per 64
// pixels), i.e. everything the EV = 1 epilogue does.  One workgroup per 64 pixels; lane = one 4-channel group of one row.
constexpr int kSplitRows = 16;                        // pixels per workgroup of the reduce launch = per statistics row
__global__ void __launch_bounds__(256)
splitk_reduce_kernel(const float* __restrict__ part, int ksplit, long long slice_stride, int M, int C, int ldp,
                     unsigned short* __restrict__ y, int HW_out, long long y_img_stride, int ldy, float* __restrict__ stats,
                     int stats_mod, int stats_ld, float stats_cap) {
  __shared__ float red[kSplitRows][256][2];             // [row][channel][value | value^2] of the STORED values (C <= 256 per pass)
  const int m0 = blockIdx.x * kSplitRows, tid = threadIdx.x;
  for (int cb = 0; cb < C; cb += 256) {
    const int cw = min(256, C - cb), c4 = (cw + 3) >> 2;     // 4-channel groups of this pass
    if (cb) __syncthreads();                            // (red is reused per pass)
    for (int item = tid; item < kSplitRows * c4; item += 256) {
      const int r = item / c4, gq = item - r * c4, m = m0 + r, c = cb + 4 * gq;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m < M) {
        const float* src = part + (size_t)m * ldp + c;
        a = *reinterpret_cast<const float4*>(src);
        int sl = 1;
        for (; sl + 3 < ksplit; sl += 4) {              // four slices' loads in flight, added in slice order
          const float4 b0 = *reinterpret_cast<const float4*>(src + (sl + 0) * slice_stride);
          const float4 b1 = *reinterpret_cast<const float4*>(src + (sl + 1) * slice_stride);
          const float4 b2 = *reinterpret_cast<const float4*>(src + (sl + 2) * slice_stride);
          const float4 b3 = *reinterpret_cast<const float4*>(src + (sl + 3) * slice_stride);
          a.x = (((a.x + b0.x) + b1.x) + b2.x) + b3.x; a.y = (((a.y + b0.y) + b1.y) + b2.y) + b3.y;
          a.z = (((a.z + b0.z) + b1.z) + b2.z) + b3.z; a.w = (((a.w + b0.w) + b1.w) + b2.w) + b3.w;
        }
        for (; sl < ksplit; ++sl) {
          const float4 b = *reinterpret_cast<const float4*>(src + sl * slice_stride);
          a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
      }
      const float v[4] = {a.x, a.y, a.z, a.w};
      const unsigned q2[2] = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
      const unsigned q[4] = {q2[0] & 0xffffu, q2[0] >> 16, q2[1] & 0xffffu, q2[1] >> 16};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float f = (m < M && c + j < C) ? bf2f((unsigned short)q[j]) : 0.f;
        if (4 * gq + j < 256) { red[r][4 * gq + j][0] = f; red[r][4 * gq + j][1] = f * f; }
      }
      if (m < M) {
        const int img = m / HW_out, pix = m - img * HW_out;
        unsigned short* dst = y + img * y_img_stride + (long long)pix * ldy + c;
        if (c + 3 < C) *reinterpret_cast<u32x2*>(dst) = u32x2{q2[0], q2[1]};
        else for (int j = 0; j < 4; ++j) if (c + j < C) dst[j] = (unsigned short)q[j];
      }
    }
    if (stats) {
      __syncthreads();
      if (tid < cw) {
        float x1 = 0.f, x2 = 0.f;
#pragma unroll
        for (int r = 0; r < kSplitRows; ++r) { x1 += red[r][tid][0]; x2 += red[r][tid][1]; }
        if (stats_mod) {                              // (fixed-point integer adds: stats_write, conv_common.h)
          unsigned long long* o = reinterpret_cast<unsigned long long*>(stats) + ((size_t)((int)blockIdx.x % stats_mod) * stats_ld + cb + tid) * 2;
          stats_add_fixed(o, x1, x2, stats_cap);
        } else {
          float* o = stats + ((size_t)blockIdx.x * stats_ld + cb + tid) * 2;
          o[0] = x1;
          o[1] = x2;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------- host side
struct TileCfg { int BM, BN; float eff; };
const TileCfg kCfgs[] = {{128, 128, 1.00f}, {128, 64, 0.85f}, {64, 128, 0.85f}, {128, 32, 0.60f}, {64, 64, 0.70f},
                          {256, 128, 1.30f}, {128, 128, 1.10f}, {256, 64, 1.0f},    // 5-7: eight-wave blocks
                          {128, 128, 1.10f},                                       // 8: eight waves, 2-deep ring, two blocks per CU
                          {128, 64, 0.85f}, {64, 64, 0.70f},                       // 9, 10: four waves, 2-deep ring (3+ blocks per CU)
                          {128, 64, 0.85f}, {256, 64, 1.0f}, {128, 128, 1.0f}};    // 11-13: 2-deep: 8w 128x64, 8w 256x64, 4w 128x128

int pick_cfg(long M, int C_out) {
  int best = 0;
  double best_t = 1e300;
  for (int i = 0; i < (int)(sizeof(kCfgs) / sizeof(kCfgs[0])); ++i) {
    if (i >= 5) continue;                        // eight-wave tiles are opt-in (MBX_FORCE_CFG / chooser below)
    const TileCfg& c = kCfgs[i];
    const long tiles = ((M + c.BM - 1) / c.BM) * ((C_out + c.BN - 1) / c.BN);
    const long lds = 3L * (c.BM + c.BN) * 128;
    long per_cu = (160 * 1024) / lds;
    if (per_cu > 2) per_cu = 2;
    const long rounds = (tiles + 256 * per_cu - 1) / (256 * per_cu);
    const double t = (double)rounds * c.BM * c.BN / c.eff;
    if (t < best_t) { best_t = t; best = i; }
  }
  return best;
}



constexpr int kNumCfgs = MBX_CONV_TILE_CONFIGS;
static_assert(kGbCtlWords * 4 == MBX_GRID_BARRIER_BYTES && kFbSlots == MBX_BN_BWD_SLOTS, "include/mbx.h and csrc/grid_barrier.h agree");
// mbx_conv_desc.tile_config beyond the igemm3 tiles 1..kNumCfgs: the launch families (include/mbx.h)
constexpr int kI5Flag = MBX_TILE_I5_BASE;         // + t + 1: igemm5 tile t (conv5.hip), persistent launch
constexpr int kI7Cfg = MBX_TILE_I7;               // igemm7 (conv7.hip), persistent pointwise launch with the filter panel in LDS
constexpr int kDirectCfg = MBX_TILE_DIRECT3;      // the direct 3x3 launch (convd.hip)
constexpr int kDirectWCfg = MBX_TILE_DIRECTW;     // the whole-width direct 3x3 launch for narrow maps (convd.hip)
constexpr int kResidentCfg = MBX_TILE_RESIDENT;   // the resident-image launch for 1x7 / 7x1 layers on small maps (convr.hip)
constexpr int kPwResCfg = MBX_TILE_PWRES;         // the pixel-resident pointwise launch for the epilogue-bound 1x1 layers (convr.hip)
constexpr int kSplitFlag = MBX_TILE_SPLITK_BASE;  // + S: split-K in S slices (float32 partials + reduce launch)
constexpr int kSplitMax = MBX_TILE_SPLITK_MAX;
// slices really used and K steps per slice for a request of S slices over nk K steps (no empty slice)
inline void splitk_geom(int nk, int S, int& ksplit, int& kps) {
  if (S > nk) S = nk;
  if (S < 1) S = 1;
  kps = (nk + S - 1) / S;
  ksplit = (nk + kps - 1) / kps;
}
int choose_cfg(long M, int C_out, int desc_cfg) {
  static const int force = mbx_env_int("MBX_FORCE_CFG", -1);
  if (force >= 0) return force;
  if (desc_cfg > 0 && desc_cfg <= kNumCfgs) return desc_cfg - 1;       // the caller measured (mbx_conv_desc.tile_config)
  // measured on MI355X (tools/kbench.py, all B=64 layer shapes, plain / residual / accumulate epilogues): the
  // eight-wave 128x128 tile with the 2-deep ring (two blocks per CU: one's epilogue and prologue overlap the
  // other's loop) wins wherever its blocks fill both slots of most CUs and the 128-wide column tile is not
  // mostly padding; then the eight-wave 256x128 tile (one block per CU); otherwise the model.
  {
    const long cols = (C_out + 127) / 128, tiles8 = ((M + 127) / 128) * cols;
    if (tiles8 >= 384 && (double)C_out >= 0.6 * (double)(cols * 128)) return 8;
  }
  if (C_out >= 256) {
    const long tiles5 = ((M + 255) / 256) * ((C_out + 127) / 128);
    const long rounds5 = (tiles5 + 255) / 256;              // one 8-wave block per CU
    if (tiles5 >= 128 && (double)tiles5 / (double)(rounds5 * 256) >= 0.7) return 5;
  }
  return pick_cfg(M, C_out);
}

// mbx_conv_pair: the first pass over each descriptor runs in CAPTURE mode (ConvK.dry == 2): the launcher records what it
// would have launched instead of launching it
struct PairCapture { ConvK k; int bm, bn, wnw, wmw, nstg, ev, mode, valid; };
thread_local PairCapture g_capture;

template <int BM, int BN, int WNW, int WMW, int EV, int NSTG>
int launch_pair_inst(const ConvK& a, const ConvK& b, hipStream_t s) {
  static bool attr = false;
  const size_t lds = NSTG * (size_t)(BM + BN) * 128;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_igemm3_pair_kernel<BM, BN, WNW, WMW, EV, 0, NSTG>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr = true;
  }
  const int n0 = a.tiles_m * a.tiles_n, n1 = b.tiles_m * b.tiles_n;
  hipLaunchKernelGGL((conv_igemm3_pair_kernel<BM, BN, WNW, WMW, EV, 0, NSTG>), dim3(n0 + n1), dim3(64 * WNW * WMW), lds, s, a, b, n0);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

template <int BM, int BN, int WNW, int WMW, int NSTG = 3>
int launch_igemm(ConvK& k, hipStream_t s) {
  k.tiles_m = (k.M + BM - 1) / BM;
  k.tiles_n = (k.C_out + BN - 1) / BN;
  k.stats_cap = stats_cap_for(k.tiles_m);               // one add per pixel tile and channel
  if (k.dry == 2) {
    g_capture.k = k; g_capture.bm = BM; g_capture.bn = BN; g_capture.wnw = WNW; g_capture.wmw = WMW; g_capture.nstg = NSTG;
    g_capture.ev = k.epi == MBX_EPI_STORE_F32 ? 5 : k.epi == MBX_EPI_RESIDUAL ? 4 : k.epi == MBX_EPI_AFFINE ? 3
                   : k.bw_n ? 6 : k.stats ? 1 : (k.accumulate || k.skip || k.bits) ? 2 : 0;
    g_capture.mode = k.shift ? 2 : k.pw ? 1 : 0;
    g_capture.valid = 1;
    return MBX_OK;
  }
  {
    const size_t lds = NSTG * (size_t)(BM + BN) * 128;          // the ring; the epilogue works out of the accumulators
    const int ev = k.epi == MBX_EPI_STORE_F32 ? 5 : k.epi == MBX_EPI_RESIDUAL ? 4 : k.epi == MBX_EPI_AFFINE ? 3
                   : k.bw_n ? 6 : k.stats ? 1 : (k.accumulate || k.skip || k.bits) ? 2 : 0;
    static bool attr_set3[7] = {false, false, false, false, false, false, false};
#define MBX_LAUNCH_EV(EV)                                                                                     \
    case EV:                                                                                                  \
      if (!attr_set3[EV]) {                                                                                   \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_igemm3_kernel<BM, BN, WNW, WMW, EV, 0, NSTG>), \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                      \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_igemm3_kernel<BM, BN, WNW, WMW, EV, 1, NSTG>), \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                      \
        attr_set3[EV] = true;                                                                                 \
      }                                                                                                       \
      if (k.pw)                                                                                               \
        hipLaunchKernelGGL((conv_igemm3_kernel<BM, BN, WNW, WMW, EV, 1, NSTG>), dim3(k.tiles_m * k.tiles_n * (EV == 5 ? k.ksplit : 1)), \
                           dim3(64 * WNW * WMW), lds, s, k);                                                  \
      else                                                                                                    \
        hipLaunchKernelGGL((conv_igemm3_kernel<BM, BN, WNW, WMW, EV, 0, NSTG>), dim3(k.tiles_m * k.tiles_n * (EV == 5 ? k.ksplit : 1)), \
                           dim3(64 * WNW * WMW), lds, s, k);                                                  \
      break;
    static bool attr_sh[2] = {false, false};
#define MBX_LAUNCH_SH(EV, SLOT)                                                                               \
    do {                                                                                                      \
      if (!attr_sh[SLOT]) {                                                                                   \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_igemm3_kernel<BM, BN, WNW, WMW, EV, 2, NSTG>), \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                      \
        attr_sh[SLOT] = true;                                                                                 \
      }                                                                                                       \
      hipLaunchKernelGGL((conv_igemm3_kernel<BM, BN, WNW, WMW, EV, 2, NSTG>), dim3(k.tiles_m * k.tiles_n),      \
                         dim3(64 * WNW * WMW), lds, s, k);                                                    \
    } while (0)
    if (k.dry) return (k.shift && ev != 0 && ev != 2) ? MBX_ERR_UNSUPPORTED : MBX_OK;       // (the stride-2 walk: store / accumulate only)
    if (k.shift) {                               // stride-2 data gradient: its own instantiations (store / accumulate)
      if (ev == 0) MBX_LAUNCH_SH(0, 0);
      else if (ev == 2) MBX_LAUNCH_SH(2, 1);
      else return MBX_ERR_UNSUPPORTED;
    } else
    switch (ev) {
      MBX_LAUNCH_EV(0) MBX_LAUNCH_EV(1) MBX_LAUNCH_EV(2) MBX_LAUNCH_EV(3) MBX_LAUNCH_EV(4) MBX_LAUNCH_EV(5) MBX_LAUNCH_EV(6)
    }
#undef MBX_LAUNCH_SH
#undef MBX_LAUNCH_EV
  }
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

}  // namespace

extern "C" int mbx_conv_stats_rows(const mbx_conv_desc* d) {
  if (!d) return MBX_ERR_INVALID_ARG;
  if (d->stats_rows_mod > 0) return d->stats_rows_mod;                 // atomic mode: R rows whatever the tiles
  const long M = (long)d->N * d->H_out * d->W_out;
  if (d->tile_config > kSplitFlag) return (int)((M + kSplitRows - 1) / kSplitRows);   // split-K: the reduce launch writes a row per 16 pixels
  if (d->tile_config == kDirectCfg) return mbx_direct3_grid(d->N, d->H_out, d->W_out);        // a row per workgroup
  if (d->tile_config == kDirectWCfg) { const int g = mbx_directw_grid(d->N, d->H_out, d->W_out); return g > 0 ? g : MBX_ERR_UNSUPPORTED; }
  if (d->tile_config == kResidentCfg) return mbx_resident_rows(d->N);                        // a row per image
  if (d->tile_config == kI7Cfg) return (int)((M + 127) / 128);
  if (d->tile_config > kI5Flag) {
    const int i = d->tile_config - kI5Flag - 1;
    if (i >= mbx_i5_num_tiles) return MBX_ERR_INVALID_ARG;
    return (int)((M + mbx_i5_tiles[i][0] - 1) / mbx_i5_tiles[i][0]);
  }
  const TileCfg& c = kCfgs[choose_cfg(M, d->C_out, d->tile_config)];
  return (int)((M + c.BM - 1) / c.BM);
}

static int conv_impl(const mbx_conv_desc* d, mbx_stream_t stream, int dry);
extern "C" int mbx_conv(const mbx_conv_desc* d, mbx_stream_t stream) { return conv_impl(d, stream, 0); }
extern "C" int mbx_conv_supported(const mbx_conv_desc* d) { return conv_impl(d, nullptr, 1); }
extern "C" int mbx_conv_pair(const mbx_conv_desc* a, const mbx_conv_desc* b, mbx_stream_t stream) {
  // both descriptors through every check of mbx_conv in capture mode; one grid if they resolved to the SAME instantiation
  // of one of the pair kernels (4-wave 128x64 / 64x64 tiles, store or store + statistics epilogue, general addressing)
  PairCapture ca, cb;
  g_capture.valid = 0;
  int st = conv_impl(a, stream, 2);
  if (st != MBX_OK) return st;
  if (!g_capture.valid) return MBX_ERR_UNSUPPORTED;       // (a persistent or split-K configuration)
  ca = g_capture;
  g_capture.valid = 0;
  st = conv_impl(b, stream, 2);
  if (st != MBX_OK) return st;
  if (!g_capture.valid) return MBX_ERR_UNSUPPORTED;
  cb = g_capture;
  if (ca.bm != cb.bm || ca.bn != cb.bn || ca.wnw != cb.wnw || ca.wmw != cb.wmw || ca.nstg != cb.nstg || ca.ev != cb.ev ||
      ca.mode != 0 || cb.mode != 0 || (ca.ev != 0 && ca.ev != 1 && ca.ev != 6) || ca.wnw != 2 || ca.wmw != 2 || ca.bn != 64)
    return MBX_ERR_UNSUPPORTED;
  ca.k.dry = cb.k.dry = 0;
  hipStream_t s = mbx_s(stream);
#define MBX_PAIR(BM_, NSTG_)                                                                                      \
  if (ca.bm == BM_ && ca.nstg == NSTG_)                                                                           \
    return ca.ev == 6 ? launch_pair_inst<BM_, 64, 2, 2, 6, NSTG_>(ca.k, cb.k, s)                                    \
           : ca.ev ? launch_pair_inst<BM_, 64, 2, 2, 1, NSTG_>(ca.k, cb.k, s) : launch_pair_inst<BM_, 64, 2, 2, 0, NSTG_>(ca.k, cb.k, s);
  MBX_PAIR(128, 2) MBX_PAIR(128, 3) MBX_PAIR(64, 2) MBX_PAIR(64, 3)
#undef MBX_PAIR
  return MBX_ERR_UNSUPPORTED;
}

extern "C" size_t mbx_conv_splitk_workspace_bytes(const mbx_conv_desc* d) {
  if (!d || d->tile_config <= kSplitFlag || d->tile_config > kSplitFlag + kSplitMax) return 0;
  int ksplit, kps;
  splitk_geom((d->R * d->S * d->C_in + 63) >> 6, d->tile_config - kSplitFlag, ksplit, kps);
  return (size_t)4 * d->N * d->H_out * d->W_out * (((d->C_out + 7) / 8) * 8) * ksplit;
}

static int conv_impl(const mbx_conv_desc* d, mbx_stream_t stream, int dry) {
  int st = check_desc(d);
  if (st != MBX_OK) return st;
  if (!d->w || !d->y) return MBX_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(d->w) & 15)) return MBX_ERR_INVALID_ARG;
  const bool f32 = d->epilogue == MBX_EPI_STORE_F32;
  if (!f32 && (d->C_out % 8 || d->ldy % 8 || (reinterpret_cast<uintptr_t>(d->y) & 15))) return MBX_ERR_INVALID_ARG;
  if (d->epilogue == MBX_EPI_RESIDUAL && (!d->skip || d->ld_skip % 8 || (reinterpret_cast<uintptr_t>(d->skip) & 15)))
    return MBX_ERR_INVALID_ARG;
  if ((long long)d->N * d->y_img_stride >= (1LL << 31)) return MBX_ERR_UNSUPPORTED;
  if (d->stats_partial && (d->epilogue != MBX_EPI_STORE || d->accumulate || d->skip)) return MBX_ERR_INVALID_ARG;
  if (d->epilogue == MBX_EPI_STORE && d->skip && (d->ld_skip % 8 || (reinterpret_cast<uintptr_t>(d->skip) & 15))) return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  ConvK k;
  k.x = reinterpret_cast<const unsigned short*>(d->x);
  k.x_img_stride = (int)d->x_img_stride; k.ldx = d->ldx; k.H_in = d->H_in; k.W_in = d->W_in; k.C_in = d->C_in;
  k.w = reinterpret_cast<const unsigned short*>(d->w);
  k.C_out = d->C_out; k.R = d->R; k.S = d->S; k.Ktot = d->R * d->S * d->C_in;
  k.x_bytes = (unsigned)(2 * ((long long)(d->N - 1) * d->x_img_stride + ((long long)d->H_in * d->W_in - 1) * d->ldx + d->C_in));
  k.w_bytes = (unsigned)(2LL * d->C_out * k.Ktot);
  if (d->transposed) { k.mul = 1; k.shift = d->stride == 2 ? 1 : 0; } else { k.mul = d->stride; k.shift = 0; }
  k.pad_t = d->pad_t; k.pad_l = d->pad_l; k.W_out = d->W_out; k.HW_out = d->H_out * d->W_out;
  k.M = d->N * k.HW_out;
  k.y = d->y; k.y_img_stride = (int)d->y_img_stride; k.ldy = d->ldy;
  k.epi = d->epilogue; k.relu = d->relu; k.accumulate = d->accumulate;
  k.scale = d->scale; k.shiftv = d->shift;
  k.skip = reinterpret_cast<const unsigned short*>(d->skip);
  k.skip_img_stride = (int)d->skip_img_stride; k.ld_skip = d->ld_skip; k.rscale = d->rscale;
  k.bits = nullptr; k.bits_ld = 0; k.bits_bytes = 0;
  if (d->relu_bits) {
    // sign bits of a residual output: written by RESIDUAL + relu, read as the mask of a plain STORE (see mbx.h)
    const bool wr = d->epilogue == MBX_EPI_RESIDUAL && d->relu, rd = d->epilogue == MBX_EPI_STORE && !d->skip;
    if ((!wr && !rd) || d->ld_bits % 4 || d->ld_bits < 4 * ((d->C_out + 31) / 32) || (reinterpret_cast<uintptr_t>(d->relu_bits) & 3)) return MBX_ERR_INVALID_ARG;
    if (d->stats_partial || d->bn_bwd_stats) return MBX_ERR_UNSUPPORTED;
    const long long bb = (long long)d->N * d->H_out * d->W_out * d->ld_bits;
    if (bb >= (1LL << 31)) return MBX_ERR_UNSUPPORTED;
    k.bits = reinterpret_cast<unsigned char*>(d->relu_bits); k.bits_ld = d->ld_bits; k.bits_bytes = (unsigned)bb;
  }
  k.stats = d->stats_partial;
  if (d->stats_rows_mod < 0 || d->stats_rows_mod > 1024 || d->stats_ld < 0 || (d->stats_ld && d->stats_ld < d->C_out)) return MBX_ERR_INVALID_ARG;
  k.stats_mod = d->stats_rows_mod; k.stats_ld = d->stats_ld ? d->stats_ld : d->C_out;
  k.stats_cap = 0.f;                                   // (set by the launcher that knows its adders per channel: stats_cap_for)
  k.fa = FusedApply{};
  k.fa.bar = nullptr;
  k.fb = FusedBwd{};
  k.fb.bar = nullptr;
  if (d->bn_bwd) {
    // the BN backward of the layers this data gradient feeds as the tail of the launch (fused_bn.h)
    const mbx_bn_bwd_fused* b = d->bn_bwd;
    if (!b->barrier || (reinterpret_cast<uintptr_t>(b->barrier) & 127) || b->n < 1 || b->n > 4 || b->c_begin[0] != 0) return MBX_ERR_INVALID_ARG;
    if (d->epilogue != MBX_EPI_STORE || d->accumulate || d->skip || d->relu_bits || d->stats_partial || d->bn_bwd_stats || d->bn_apply ||
        d->stride != 1 || d->C_out > 2048 || d->y_img_stride != (int64_t)d->H_out * d->W_out * d->ldy)
      return MBX_ERR_UNSUPPORTED;
    const int tc = d->tile_config;
    if (!((tc > kI5Flag && tc <= kI5Flag + 7) || tc == kDirectWCfg || tc == kResidentCfg)) return MBX_ERR_UNSUPPORTED;
    const long long Mll = (long long)d->N * d->H_out * d->W_out;
    for (int i = 0; i < 4; ++i) k.fb.cb[i] = 1 << 30;
    for (int i = 0; i < b->n; ++i) {
      if (!b->y[i] || !b->dy[i] || !b->mean[i] || !b->rstd[i] || (b->relu[i] && !b->beta[i]) || !b->acc[i] ||
          (reinterpret_cast<uintptr_t>(b->y[i]) & 15) || (reinterpret_cast<uintptr_t>(b->dy[i]) & 15) || b->ld_y[i] % 8 || b->ld_dy[i] % 8 ||
          b->c_begin[i] % 8 || b->c_begin[i] >= d->C_out || (i && b->c_begin[i] <= b->c_begin[i - 1]) || b->acc_ld[i] <= 0)
        return MBX_ERR_INVALID_ARG;
      if (Mll * b->ld_y[i] >= (1LL << 31) || Mll * b->ld_dy[i] >= (1LL << 31)) return MBX_ERR_UNSUPPORTED;
      k.fb.cb[i] = b->c_begin[i];
      k.fb.y[i] = reinterpret_cast<const unsigned short*>(b->y[i]); k.fb.ldy[i] = b->ld_y[i];
      k.fb.dy[i] = reinterpret_cast<unsigned short*>(b->dy[i]); k.fb.lddy[i] = b->ld_dy[i];
      k.fb.mean[i] = b->mean[i]; k.fb.rstd[i] = b->rstd[i]; k.fb.beta[i] = b->beta[i]; k.fb.dbeta[i] = b->dbeta[i];
      k.fb.acc[i] = b->acc[i]; k.fb.acc_ld[i] = b->acc_ld[i]; k.fb.relu[i] = b->relu[i];
    }
    const int fault = mbx_barrier_fault() == '3';             // '3': the fused BACKWARD barriers
    k.fb.n = b->n;
    k.fb.bar = reinterpret_cast<unsigned*>(b->barrier);
    static const int probe = mbx_env_int("MBX_FUSED_PROBE", 0) & ~1;
    k.fb.spin_limit = fault ? (1u << 10) : (1u << 22); k.fb.fault = fault | probe; k.fb.step_poison = b->step_poison;
    k.fb.inv_M = (float)(1.0 / (double)Mll);
  }
  if (d->bn_apply) {
    // the layer's BN apply as the tail of this launch (fused_bn.h): fixed-point statistics rows, plain bf16 store, rows of y
    // contiguous over the images; only the launches whose workgroups are all resident (checked per family below)
    const mbx_bn_apply_desc* b = d->bn_apply;
    if (!b->barrier || !b->a || !b->beta || !b->mean || !b->rstd || (reinterpret_cast<uintptr_t>(b->barrier) & 127) ||
        (reinterpret_cast<uintptr_t>(b->a) & 15) || b->ld_a % 8 || b->ld_a < d->C_out)
      return MBX_ERR_INVALID_ARG;
    if (!d->stats_partial || d->stats_rows_mod < 1 || d->stats_rows_mod > 16 || d->epilogue != MBX_EPI_STORE || d->accumulate || d->skip ||
        d->transposed || d->rscale != 0.f || d->C_out > 2048 || d->y_img_stride != (int64_t)d->H_out * d->W_out * d->ldy ||
        (long long)d->N * d->H_out * d->W_out * b->ld_a >= (1LL << 31))
      return MBX_ERR_UNSUPPORTED;
    const int tc = d->tile_config;
    if (!((tc > kI5Flag && tc <= kI5Flag + 7) || tc == kDirectWCfg || tc == kResidentCfg)) return MBX_ERR_UNSUPPORTED;
    const int fault = mbx_barrier_fault() == '2';             // '2': the FORWARD barriers
    k.fa.bar = reinterpret_cast<unsigned*>(b->barrier);
    static const int probe = mbx_env_int("MBX_FUSED_PROBE", 0) & ~1;      // timing probes of tools/fused_probe.py (WRONG results)
    k.fa.spin_limit = fault ? (1u << 10) : (1u << 22); k.fa.fault = fault | probe; k.fa.step_poison = b->step_poison;
    k.fa.a = reinterpret_cast<unsigned short*>(b->a); k.fa.ld_a = b->ld_a; k.fa.beta = b->beta;
    k.fa.mean = b->mean; k.fa.rstd = b->rstd; k.fa.mmean = b->moving_mean; k.fa.mvar = b->moving_var; k.fa.thr = b->relu_thr;
    k.fa.relu = b->relu; k.fa.eps = b->eps; k.fa.decay = b->decay;
    k.fa.inv_count = 1.0 / (double)((long long)d->N * d->H_out * d->W_out);
  }
  k.bw_n = 0; k.bw_mod = 1;
  for (int i = 0; i < 4; ++i) { k.bw_cb[i] = 1 << 30; k.bw_ldy[i] = 0; k.bw_sld[i] = 0; k.bw_y[i] = nullptr; k.bw_thr[i] = nullptr; k.bw_stats[i] = nullptr; }
  if (d->bn_bwd_stats) {
    // BN-backward statistics epilogue: plain bf16 store only (a scale is fine), never with the forward statistics
    const mbx_bn_bwd_stats* b = d->bn_bwd_stats;
    if (d->epilogue != MBX_EPI_STORE || d->accumulate || d->skip || d->stats_partial || b->n < 1 || b->n > 4 || b->rows_mod < 1 ||
        b->rows_mod > 1024 || b->c_begin[0] != 0)
      return MBX_ERR_INVALID_ARG;
    for (int i = 0; i < b->n; ++i) {
      if (!b->y[i] || !b->relu_thr[i] || !b->stats[i] || (reinterpret_cast<uintptr_t>(b->y[i]) & 15) || b->ld_y[i] % 8 || b->c_begin[i] % 32 ||
          b->c_begin[i] >= d->C_out || (i && b->c_begin[i] <= b->c_begin[i - 1]) || b->stats_ld[i] <= 0)
        return MBX_ERR_INVALID_ARG;
      k.bw_cb[i] = b->c_begin[i]; k.bw_ldy[i] = b->ld_y[i]; k.bw_sld[i] = b->stats_ld[i];
      k.bw_y[i] = reinterpret_cast<const unsigned short*>(b->y[i]); k.bw_thr[i] = b->relu_thr[i]; k.bw_stats[i] = b->stats[i];
    }
    k.bw_n = b->n; k.bw_mod = b->rows_mod;
  }
  if (d->accumulate && d->acc_src) {
    if (d->ld_acc % 8 || (reinterpret_cast<uintptr_t>(d->acc_src) & 15) || (long long)d->N * d->acc_img_stride >= (1LL << 31))
      return MBX_ERR_INVALID_ARG;
    k.acc_src = reinterpret_cast<const unsigned short*>(d->acc_src); k.acc_img_stride = (int)d->acc_img_stride; k.ld_acc = d->ld_acc;
  } else {
    k.acc_src = reinterpret_cast<const unsigned short*>(d->y); k.acc_img_stride = (int)d->y_img_stride; k.ld_acc = d->ldy;
  }
  {  // ranges of the epilogue's buffer descriptors: last pixel of the last image + the channels of the view
    const long long last_pix = (long long)k.HW_out - 1, span = ((d->C_out + 7) / 8) * 8;
    const long long yb = 2 * ((long long)(d->N - 1) * d->y_img_stride + last_pix * d->ldy + span);
    const long long sb = d->skip ? 2 * ((long long)(d->N - 1) * d->skip_img_stride + last_pix * d->ld_skip + span) : 0;
    const long long ab = 2 * ((long long)(d->N - 1) * k.acc_img_stride + last_pix * k.ld_acc + span);
    if (!f32 && (yb >= (1LL << 31) || sb >= (1LL << 31) || ab >= (1LL << 31))) return MBX_ERR_UNSUPPORTED;
    k.y_bytes = (unsigned)yb; k.skip_bytes = (unsigned)sb; k.acc_bytes = (unsigned)ab;
  }
  set_magic((unsigned)k.HW_out, k.mg_hw, k.sh_hw);
  set_magic((unsigned)k.W_out, k.mg_w, k.sh_w);
  k.pw = (d->R == 1 && d->S == 1 && d->pad_t == 0 && d->pad_l == 0 && d->stride == 1) ? 1 : 0;
  k.skip_taps = 0; k.parity = 0;
  k.work_counter = d->work_counter;
  k.max_wg = d->max_workgroups;
  k.dry = dry;
  k.ksplit = 1; k.kps = 1 << 30; k.y_split_stride = 0;
#ifdef MBX_I5_STAMPS
  {  // debug build (MBX_BUILD_DEFS=-DMBX_I5_STAMPS): MBX_I5_STAMP_PTR = device address of 64 x 8 x 4 uint64 (tools/i5_stamps.py)
    static const unsigned long long sp = getenv("MBX_I5_STAMP_PTR") ? strtoull(getenv("MBX_I5_STAMP_PTR"), nullptr, 10) : 0ull;
    k.stamps = reinterpret_cast<unsigned long long*>(sp);
    k.dbg = mbx_env_int("MBX_I5_DBG", 0);                // (read per call: tools switch it between launches)
    k.stagger = mbx_env_int("MBX_STAGGER", 0);
  }
#endif
  for (int c = 0; c < 4; ++c) { k.cls_m0[c] = 0; k.cls_hw[c] = 1; k.cls_w[c] = 1; }
  static const bool notap = mbx_env_char("MBX_NO_TAP_SKIP") == '1';
  if (k.shift && d->C_in % 64 == 0 && !notap) {  // K tiles never straddle filter taps: whole taps can be skipped
    // parity classes of the output pixels (class = (oh & 1) * 2 + (ow & 1)); an empty class has the start of the
    // next one, so pixel_class() steps over it
    int m0 = 0;
    for (int c = 0; c < 4; ++c) {
      const int hc = (d->H_out - (c >> 1) + 1) / 2, wc = (d->W_out - (c & 1) + 1) / 2;
      k.cls_m0[c] = m0;
      k.cls_hw[c] = hc * wc > 0 ? hc * wc : 1;
      k.cls_w[c] = wc > 0 ? wc : 1;
      m0 += d->N * hc * wc;
    }
    k.skip_taps = k.parity = 1;
  }
  if (k.bits && k.shift) return MBX_ERR_UNSUPPORTED;      // (the sign bits are indexed by the raster pixel index)
  hipStream_t s = mbx_s(stream);
  if (d->tile_config > kSplitFlag) {
    // split-K: forward convolutions with a bf16 store (+ statistics) epilogue only; partials in the caller's workspace
    const int S = d->tile_config - kSplitFlag;
    if (S < 2 || S > kSplitMax || d->transposed || d->bn_bwd_stats || d->relu_bits || d->epilogue != MBX_EPI_STORE || d->accumulate || d->skip || d->rscale != 0.f)
      return MBX_ERR_UNSUPPORTED;
    const int ldp = ((d->C_out + 7) / 8) * 8;
    int ksplit, kps;
    splitk_geom((k.Ktot + 63) >> 6, S, ksplit, kps);
    const long long slice = (long long)k.M * ldp;
    if (!d->splitk_ws || (reinterpret_cast<uintptr_t>(d->splitk_ws) & 15) || d->splitk_ws_bytes < (int64_t)(4 * slice * ksplit) ||
        slice * ksplit >= (1LL << 31))
      return MBX_ERR_WORKSPACE;
    ConvK g = k;
    g.epi = MBX_EPI_STORE_F32; g.stats = nullptr; g.relu = 0;
    g.y = d->splitk_ws; g.ldy = ldp; g.y_img_stride = k.HW_out * ldp;
    g.ksplit = ksplit; g.kps = kps; g.y_split_stride = slice;
    st = launch_igemm<128, 64, 2, 2>(g, s);
    if (st != MBX_OK || dry) return st;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((k.M + kSplitRows - 1) / kSplitRows), dim3(256), 0, s, reinterpret_cast<const float*>(d->splitk_ws),
                       ksplit, slice, k.M, k.C_out, ldp, reinterpret_cast<unsigned short*>(k.y), k.HW_out,
                       (long long)k.y_img_stride, k.ldy, k.stats, k.stats_mod, k.stats_ld, stats_cap_for((k.M + kSplitRows - 1) / kSplitRows));
    MBX_LAUNCH_CHECK();
    return MBX_OK;
  }
  if (d->tile_config == kDirectCfg) return mbx_launch_direct3(k, d->N, d->H_out, s);
  if (d->tile_config == kDirectWCfg) return mbx_launch_directw(k, d->N, d->H_out, s);
  if (d->tile_config == kResidentCfg) return mbx_launch_resident(k, d->N, d->H_out, s);
  if (d->tile_config == kPwResCfg) return mbx_launch_pwres(k, s);
  if (d->tile_config == kI7Cfg) return mbx_launch_igemm7(k, s);
  if (d->tile_config > kI5Flag) return mbx_launch_igemm5(k, d->tile_config - kI5Flag - 1, s);
  switch (choose_cfg(k.M, k.C_out, d->tile_config)) {
    case 0: return launch_igemm<128, 128, 2, 2>(k, s);
    case 1: return launch_igemm<128, 64, 2, 2>(k, s);
    case 2: return launch_igemm<64, 128, 2, 2>(k, s);
    case 3: return launch_igemm<128, 32, 1, 4>(k, s);
    case 5: return launch_igemm<256, 128, 2, 4>(k, s);
    case 6: return launch_igemm<128, 128, 2, 4>(k, s);
    case 7: return launch_igemm<256, 64, 1, 8>(k, s);
    case 8: return launch_igemm<128, 128, 2, 4, 2>(k, s);
    case 9: return launch_igemm<128, 64, 2, 2, 2>(k, s);
    case 10: return launch_igemm<64, 64, 2, 2, 2>(k, s);
    case 11: return launch_igemm<128, 64, 2, 4, 2>(k, s);
    case 12: return launch_igemm<256, 64, 1, 8, 2>(k, s);
    case 13: return launch_igemm<128, 128, 2, 2, 2>(k, s);
    default: return launch_igemm<64, 64, 2, 2>(k, s);
  }
}
