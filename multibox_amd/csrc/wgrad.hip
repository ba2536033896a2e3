// libmbx: the weight gradient of the convolutions (gfx950) -- the single-layer kernel (mbx_conv_wgrad[_scaled]), the
// grouped launch of a whole backward segment (mbx_conv_wgrad_grouped) and its host-side planner (mbx_wgrad_plan).
// NHWC bf16 views, KRSC float32 filter gradients.  The forward / data-gradient kernels are in conv.hip.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "conv_common.h"

namespace {

// ------------------------------------------------------------------------- weight gradient
// dW[n][kc] += sum_m dY[m][n] * P[m][kc]; GEMM whose reduction runs over PIXELS, the slow NHWC
// dimension of both operands: tiles are staged [pixel][channel] exactly as they lie in HBM and
// the MFMA fragments (8 consecutive pixels of one channel) come out of LDS through the gfx950
// transpose read ds_read_b64_tr_b16.  Split over pixels across blockIdx.y, fp32 atomics.
struct WgradK {
  const unsigned short* x; int x_img_stride, ldx, H_in, W_in, C_in;
  const unsigned short* dy; int dy_img_stride, ld_dy;
  int C_out, S, Ktot, stride, pad_t, pad_l, W_out, HW_out, M;
  float* dw; float* db; float scale;
  unsigned x_bytes, dy_bytes;
  unsigned mg_hw, sh_hw, mg_w, sh_w;     // magic-number division by HW_out and W_out
  int H_out;
  int tiles_n, tiles_k, m_per_split;
};

// chunk swizzle of a staged [64 pixels][channels] tile by pixel row: 256-byte rows (16 chunks) | 128-byte rows (8 chunks)
__device__ __forceinline__ int wg_swz(int row) { return ((row & 3) | (((row >> 3) & 1) << 2)) << 1; }
__device__ __forceinline__ int wg_swz64(int row) { return (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1; }

// ------------------------------------------------------------------------------------------
// The kernel: 128 x 128 output tile, 64 pixels per step, tiles staged by LDS-DMA into an NST-deep ring.
// One DMA wave-instruction fills 4 rows x 16 chunks; the swizzle moves to the source chunk
// (chunk = slot ^ swz(row), constant per lane because row & 3 and row bit 3 are lane constants).
// Pixel rows advance by 16 per instruction: decoded once, then stepped incrementally; 1x1 convs
// (contiguous pixel rows) take a two-instruction address path.  Fragment addresses are per-lane
// constants + immediates.
struct WgradK2 {
  WgradK b;
  int pw;            // x rows contiguous: offset = m * ldx (1x1, stride 1, no padding, dense images)
  int ydense;        // dy rows contiguous: offset = m * ld_dy
  int dbg;           // MBX_WG_DBG ablation switches (diagnosis only): 1 no DMA after the prologue, 2 no LDS reads / MFMA
};

// NG = 2: eight waves; the two 4-wave groups reduce disjoint halves of the block's pixel range into the
// SAME (n, k) tile and are summed through LDS before the atomics -> half the atomic bytes per FLOP
// (the fp32 atomics ran at the chip-wide atomic rate and cost ~35 % of the 1x1 weight gradients).
// LIN: x and dy rows are both contiguous in the pixel index (1x1 convs on dense views): offsets are m * ld, no
// (image, row, column) bookkeeping -- compile-time, like the pointwise mode of the igemm kernel.
// BIAS: the bias gradient (column sums of dy) rides along -- only the residual "up" convs have a bias.
// The block's work is given by the caller: output tile (tile_n, tile_k) and pixel range [blk_begin, blk_end) -- from
// blockIdx for the one-layer launch, from a work-item table for the grouped launch (conv_wgrad_grouped_kernel).
// NYF: 16-channel dy fragments per wave, i.e. the width of the tile.  4 is the WIDE tile above.  2 is the NARROW tile:
// 64 output channels x 128 filter columns per block (dy rows of 128 B in LDS, their own swizzle).
// Half the tile for the same grid means every block covers twice the pixels: half the fp32 atomics per launch, and
// channel counts like 32 / 48 / 64 / 160 / 192 / 320 / 1088 stop padding a 128-wide tile.  dy must be pixel-dense.
constexpr int kWg2Stages = 2;                                     // ring depth 2: one step in flight
constexpr int wg2_stage_slots(int nyf) { return 64 * 4 * nyf + 64 * 16; }   // 16-byte slots: [Y 64 x 4 NYF | X 64 x 16]
template <int NYF>
__device__ __forceinline__ int wg2_yswz(int row) { if constexpr (NYF == 4) return wg_swz(row); else return wg_swz64(row); }

template <int NYF, int NST, int NG, bool LIN, bool BIAS>
__device__ __forceinline__ void wgrad2_body(const WgradK2& q, u32x4* smem, const int tile_n, const int tile_k,
                                            const int blk_begin, const int blk_end) {
  static_assert(NYF == 4 || NYF == 2, "wide or narrow tile");
  const WgradK& p = q.b;
  // ---- the geometry of the dy tile: all that differs between the two widths (wide | narrow)
  constexpr int YROW = 64 * NYF;                       // bytes of a dy row in LDS: 256 | 128
  constexpr int YCH = YROW / 16, YRPI = 64 / YCH;      // a dy DMA wave-instruction fills YRPI rows x YCH chunks: 4 x 16 | 8 x 8
  constexpr int YDMA = 64 / (4 * YRPI);                // dy DMA instructions per wave and step: 4 | 2 (x: always 4)
  constexpr int XSLOT = 64 * YCH;                      // 16-byte slot of the x tile inside a stage: behind the dy tile
  constexpr int STAGE = wg2_stage_slots(NYF);          // smem: [NST][Y 64 x YCH | X 64x16] slots
  constexpr int YKK = 32 * YROW, YHI = 4 * YROW;       // dy transposing reads: bytes to pixel rows + 32 (kk) and + 4 (upper half)
  constexpr int NB = 32 * NYF, NW = 16 * NYF;          // output channels per block (= bf16 elements of a dy row) and per wave
  const int lane = threadIdx.x & 63;
  const int wave8 = wave_id();
  const int grp = NG == 2 ? (wave8 >> 2) : 0, wave = wave8 & 3;
  const int tid = threadIdx.x & 255;                   // thread index inside its 4-wave group
  const int wn = wave & 1, wk = wave >> 1;
  const int n0 = tile_n * NB, k0 = tile_k * 128;
  // group 0 takes the first half of the block's pixels (rounded up to 64), group 1 the rest
  const int half = NG == 2 ? ((((blk_end - blk_begin) + 1) / 2 + 63) & ~63) : (blk_end - blk_begin);
  const int m_begin = blk_begin + grp * half;
  const int m_end = NG == 2 ? (grp == 0 ? min(blk_end, blk_begin + half) : blk_end) : blk_end;
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t yr = make_rsrc(p.dy, p.dy_bytes);

  // ---- DMA lane constants
  const int r4 = lane >> 4;                                   // row within the 4-row piece
  const int swz = wg_swz(4 * wave + r4);                      // swz(row) for rows 16*i + 4*wave + r4
  const int lc = (lane & 15) ^ swz;                           // logical chunk this lane fetches
  const int kcol = k0 + lc * 8;
  const bool kvalid = kcol < p.Ktot;
  const int tap = (kvalid ? kcol : 0) / p.C_in, tc = (kvalid ? kcol : 0) - tap * p.C_in;
  const int tr = kvalid ? tap / p.S : (1 << 24), ts = tap - (tap / p.S) * p.S;
  const int toff = ((tr * p.W_in + ts) * p.ldx + tc) * 2;
  // dy rows 4 * YRPI * i + YRPI * wave + ry: their swizzle is a lane constant like that of the x rows
  const int ry = lane / YCH;
  const int lcy = (lane & (YCH - 1)) ^ wg2_yswz<NYF>(YRPI * wave + ry);
  const int ycol = (n0 + lcy * 8 < p.C_out) ? (n0 + lcy * 8) * 2 : -1;
  const int ldx2 = p.ldx * 2, ldy2 = p.ld_dy * 2;
  // narrow: next dy row of this lane (advances by 32 per instruction); the wide tile's dy rows are its x rows (m_run)
  [[maybe_unused]] int my_run = m_begin + wave * YRPI + ry;
  // running pixel = next row this lane will fetch (advances by 16 per DMA instruction)
  int m_run = m_begin + wave * 4 + r4;
  int img = 0, oh = 0, ow = 0;
  {
    const unsigned mm = (unsigned)min(m_run, p.M - 1);
    img = (int)fast_div(mm, p.mg_hw, p.sh_hw);
    const int pix = (int)mm - img * p.HW_out;
    oh = (int)fast_div((unsigned)pix, p.mg_w, p.sh_w);
    ow = pix - oh * p.W_out;
  }

  // ---- fragment (transpose-read) lane constants, byte offsets inside a stage
  const int g = lane >> 4, t = lane & 15, fq = t >> 2, pp = t & 3;
  const int lb = (8 * g + fq) * 256 + (pp & 1) * 8;
  const int sx = wg_swz(8 * g + fq);
  const int lby = (8 * g + fq) * YROW + (pp & 1) * 8;
  const int sxy = wg2_yswz<NYF>(8 * g + fq);
  int yo[NYF], xo[4];
#pragma unroll
  for (int a = 0; a < NYF; ++a) yo[a] = lby + (((2 * (wn * NYF + a) + (pp >> 1)) ^ sxy) << 4);
#pragma unroll
  for (int b = 0; b < 4; ++b) xo[b] = lb + (((2 * (wk * 4 + b) + (pp >> 1)) ^ sx) << 4) + XSLOT * 16;

  f32x4 acc[NYF][4];
#pragma unroll
  for (int a = 0; a < NYF; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  const bool do_bias = BIAS && p.db != nullptr && tile_k == 0 && tid < NB && n0 + tid < p.C_out;

  const int nsteps = (half + 63) >> 6;                   // same trip count for both groups (barriers are block-wide)
  int st_issue = 0, st_comp = 0;
  typedef s16x4 __attribute__((address_space(3))) * lds_tr;
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  // DMA of pixel step LT into ring slot st_issue (macro: straight-line call sites, see igemm)
#define MBX_ISSUE_STEP()                                                                                      \
  do {                                                                                                        \
    u32x4* sp = smem + (grp * NST + st_issue) * STAGE + wave * 64;                                            \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                           \
      const bool mv = m_run < m_end;                                                                          \
      int xoff, yoff;                                                                                         \
      if (LIN || q.pw) xoff = (mv && kvalid) ? (m_run * ldx2 + kcol * 2) : (int)kOOB;                         \
      else {                                                                                                  \
        const int hb = oh * p.stride - p.pad_t + tr, wb = ow * p.stride - p.pad_l + ts;                       \
        const bool ok = mv && ((unsigned)hb < (unsigned)p.H_in) && ((unsigned)wb < (unsigned)p.W_in);         \
        xoff = ok ? ((img * p.x_img_stride + ((oh * p.stride - p.pad_t) * p.W_in + ow * p.stride - p.pad_l) * p.ldx) * 2 + toff) \
                  : (int)kOOB;                                                                                \
      }                                                                                                       \
      if (i < YDMA) {                                                                                         \
        if constexpr (NYF == 2) {                                                                             \
          yoff = (my_run < m_end && ycol >= 0) ? (my_run * ldy2 + ycol) : (int)kOOB;                          \
          my_run += 32;                                                                                       \
        } else if (LIN || q.ydense) yoff = (mv && ycol >= 0) ? (m_run * ldy2 + ycol) : (int)kOOB;             \
        else yoff = (mv && ycol >= 0) ? ((img * p.dy_img_stride + (oh * p.W_out + ow) * p.ld_dy) * 2 + ycol) : (int)kOOB; \
        glds16(yr, sp + i * 256, yoff);                                                                       \
      }                                                                                                       \
      glds16(xr, sp + XSLOT + i * 256, xoff);                                                                 \
      m_run += 16;                                                                                            \
      if (!LIN && !(q.pw && q.ydense)) {                                                                      \
        ow += 16;                                                                                             \
        while (ow >= p.W_out) { ow -= p.W_out; ++oh; }                                                        \
        while (oh >= p.H_out) { oh -= p.H_out; ++img; }                                                       \
      }                                                                                                       \
    }                                                                                                         \
    st_issue = st_issue == NST - 1 ? 0 : st_issue + 1;                                                        \
  } while (0)

  static_assert(NST == kWg2Stages, "ring depth 2: one step in flight");
  if (nsteps > 0) MBX_ISSUE_STEP();
  wait_vmcnt<0>();
  raw_barrier();
  for (int it = 0; it < nsteps; ++it) {
    if (it + 1 < nsteps) MBX_ISSUE_STEP();
    {
      const char* base = reinterpret_cast<const char*>(smem + (grp * NST + st_comp) * STAGE);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 yf[NYF], xf[4];
#pragma unroll
        for (int a = 0; a < NYF; ++a) {
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(base + yo[a] + kk * YKK));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(base + yo[a] + kk * YKK + YHI));
          const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          yf[a] = __builtin_bit_cast(bf16x8, v);
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(base + xo[b] + kk * 8192));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(base + xo[b] + kk * 8192 + 1024));
          const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          xf[b] = __builtin_bit_cast(bf16x8, v);
        }
#pragma unroll
        for (int a = 0; a < NYF; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[a], xf[b], acc[a][b], 0, 0, 0);
      }
      if (do_bias) {
        const unsigned short* cY = reinterpret_cast<const unsigned short*>(base);
        const int ch = tid >> 3, e = tid & 7;
        for (int r = 0; r < 64; ++r) bsum += bf2f(cY[r * NB + ((ch ^ wg2_yswz<NYF>(r)) << 3) + e]);
      }
      st_comp = st_comp == NST - 1 ? 0 : st_comp + 1;
    }
    wait_vmcnt<0>();
    if (it + 1 < nsteps) {            // 2-deep ring: landing probe, as in conv_igemm3_kernel (NSTG == 2)
      lds_readback_wait(lds_readback_issue(smem + (grp * NST + (st_issue ^ 1)) * STAGE + wave * 64 + lane));
    }
    raw_barrier();
  }
#undef MBX_ISSUE_STEP
  wait_vmcnt<0>();
  if (NG == 2) {                                        // group 1 -> LDS -> group 0 (rings are idle now)
    float* xch = reinterpret_cast<float*>(smem);
    if (grp == 1) {
#pragma unroll
      for (int a = 0; a < NYF; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) xch[((a * 4 + b) * 4 + r) * 256 + tid] = acc[a][b][r];
    }
    __syncthreads();
    if (grp == 1) {
      if (do_bias) atomicAdd(p.db + n0 + tid, bsum * p.scale);
      return;
    }
#pragma unroll
    for (int a = 0; a < NYF; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[a][b][r] += xch[((a * 4 + b) * 4 + r) * 256 + tid];
  }
#pragma unroll
  for (int a = 0; a < NYF; ++a) {
    const int nb = n0 + wn * NW + a * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int kc = k0 + wk * 64 + b * 16 + (lane & 15);
      if (kc >= p.Ktot) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (nb + r < p.C_out) atomicAdd(p.dw + (size_t)(nb + r) * p.Ktot + kc, acc[a][b][r] * p.scale);
    }
  }
  if (do_bias) atomicAdd(p.db + n0 + tid, bsum * p.scale);
}

template <int NYF, int NST, int NG, bool LIN, bool BIAS>
__global__ void __launch_bounds__(kThreads * NG)
conv_wgrad2_kernel(const WgradK2 q) {
  extern __shared__ __attribute__((aligned(16))) u32x4 smem[];
  const WgradK& p = q.b;
  const int ntiles = p.tiles_n * p.tiles_k;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile = lid % ntiles, split = lid / ntiles;
  const int blk_begin = split * p.m_per_split;
  wgrad2_body<NYF, NST, NG, LIN, BIAS>(q, smem, tile % p.tiles_n, tile / p.tiles_n, blk_begin, min(p.M, blk_begin + p.m_per_split));
}

// ------------------------------------------------------------------------------------------
// wgrad5: the body of the grouped launch.  SIXTEEN waves with fixed roles: waves 0-7 COMPUTE a (64 NY channels) x
// (64 NX filter columns) output tile, waves 8-15 LOAD.
//  * Roles.  Measured on the all-waves-do-both form (MBX_WG_DBG ablations of the round-2 wgrad3 body): the LDS-DMA
//    issue of a 64-pixel step (~0.5 us of the CU's address path) and its LDS reads + MFMAs (~0.8 us) ADD UP when every
//    wave does first the one and then the other behind a common barrier -- the matrix pipes idle while the block
//    issues loads.  With loader waves the two run side by side: the compute waves issue no vector-memory instruction
//    in the loop and never wait on vmcnt.  Eight loaders beat four by 9 % (a wave issues one DMA per ~100 cycles).
//  * Tile shapes.  The launch is bound by the bytes the CUs pull through the L2 -> LDS path (~45 GB/s per CU), so the
//    planner picks, per layer, the (NY, NX) that moves the fewest bytes: a stage is NY + NX sub-images of
//    [64 pixels][64 channels] (8 KB, 128-byte rows, the transposing-read swizzle of the old narrow dy tile), so
//    channel counts like 160 / 192 / 320 / 1088 and filter widths like 384 / 896 / 1120 stop padding a fixed 128 x 256
//    tile (32 % of the MFMAs and a quarter of the bytes of the step were padding).
//  * Three stages, two steps of global latency in flight (counted vmcnt in the loaders only).  Loader lw fills rows
//    8 lw .. 8 lw + 7 of every sub-image: ONE pixel row per lane and step.
//  * The bias gradient (column sums of dy) is summed by the loaders out of the landed dy sub-images.
//  * single != 0: this block is the only adder of its dw tile (the pixel range is the whole layer) -> plain stores.
constexpr int kWgLoaders = 8;
static_assert(kWgLoaders * 8 == 64, "wgrad5: one 8-row piece of every 64-row sub-image per loader wave");
constexpr int kWgStageSlots = 6 * 512;                            // 16-byte slots per stage: up to six 8 KB sub-images

template <int NY, int NX>
__device__ __forceinline__ void wgrad5_body(const WgradK2& q, u32x4* smem, const int tile_n, const int tile_k,
                                            const int blk_begin, const int blk_end, const int single) {
  static_assert(NY + NX <= 6 && NY >= 1 && NX >= 1, "stage = at most six sub-images (48 KB)");
  const WgradK& p = q.b;
  constexpr int NSUB = NY + NX, STAGE = kWgStageSlots, NST = 3;
  const int lane = threadIdx.x & 63;
  const int wave = wave_id();                                     // 0..15
  const int n0 = tile_n * 64 * NY, k0 = tile_k * 64 * NX;
  const int nsteps = (blk_end - blk_begin + 63) >> 6;
  const bool bias = p.db != nullptr && tile_k == 0;               // block-uniform

  if (wave >= 8) {
    // ------------------------------------------------------------------------------------------ loader waves
    const int lw = wave - 8;
    const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t yr = make_rsrc(p.dy, p.dy_bytes);
    const int r8 = lane >> 3;                                     // this lane's row inside the 8-row piece
    const int lc = (lane & 7) ^ wg_swz64(8 * lw + r8);            // logical chunk fetched into physical slot lane & 7
    int toff[NX], tr[NX], ts[NX], ycol[NY];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const int kcol = k0 + j * 64 + lc * 8;
      const bool kv = kcol < p.Ktot;
      const int kc = kv ? kcol : 0;
      const int tap = kc / p.C_in, tc = kc - tap * p.C_in;
      tr[j] = kv ? tap / p.S : (1 << 24);                         // an invalid column fails the row bound check below
      ts[j] = tap - (tap / p.S) * p.S;
      toff[j] = ((tr[j] * p.W_in + ts[j]) * p.ldx + tc) * 2;
    }
#pragma unroll
    for (int j = 0; j < NY; ++j) ycol[j] = (n0 + j * 64 + lc * 8 < p.C_out) ? (n0 + j * 64 + lc * 8) * 2 : -1;
    const int ldy2 = p.ld_dy * 2;
    int m_run = blk_begin + 8 * lw + r8;                          // + 64 per step
    int img, oh, ow;
    {
      const unsigned mm = (unsigned)min(m_run, p.M - 1);
      img = (int)fast_div(mm, p.mg_hw, p.sh_hw);
      const int pix = (int)mm - img * p.HW_out;
      oh = (int)fast_div((unsigned)pix, p.mg_w, p.sh_w);
      ow = pix - oh * p.W_out;
    }
    int st_issue = 0, st_bias = 0;
// one pixel step's LDS-DMA in two halves (dy sub-images; x sub-images + cursor advance): the landing hand-off of the
// NEXT step (wait + read-back, see conv_igemm3_kernel) sits between them, its LDS round trip covered by the second half
#define MBX_ISSUE_STEP5_Y()                                                                                    \
  do {                                                                                                         \
    u32x4* d = smem + st_issue * STAGE + lw * 64;                                                              \
    const bool mv = m_run < blk_end;                                                                           \
    const int yb = q.ydense ? m_run * ldy2 : (img * p.dy_img_stride + (oh * p.W_out + ow) * p.ld_dy) * 2;      \
    _Pragma("unroll") for (int j = 0; j < NY; ++j)                                                             \
      glds16(yr, d + j * 512, (mv && ycol[j] >= 0) ? yb + ycol[j] : (int)kOOB);                                \
  } while (0)
#define MBX_ISSUE_STEP5_X()                                                                                    \
  do {                                                                                                         \
    u32x4* d = smem + st_issue * STAGE + lw * 64;                                                              \
    const bool mv = m_run < blk_end;                                                                           \
    const int h0 = oh * p.stride - p.pad_t, w0 = ow * p.stride - p.pad_l;                                      \
    const int rb = (img * p.x_img_stride + (h0 * p.W_in + w0) * p.ldx) * 2;                                    \
    _Pragma("unroll") for (int j = 0; j < NX; ++j) {                                                           \
      const bool ok = mv && ((unsigned)(h0 + tr[j]) < (unsigned)p.H_in) && ((unsigned)(w0 + ts[j]) < (unsigned)p.W_in); \
      glds16(xr, d + (NY + j) * 512, ok ? rb + toff[j] : (int)kOOB);                                           \
    }                                                                                                          \
    m_run += 64;                                                                                               \
    ow += 64;                                                                                                  \
    while (ow >= p.W_out) { ow -= p.W_out; ++oh; }                                                             \
    while (oh >= p.H_out) { oh -= p.H_out; ++img; }                                                            \
    st_issue = st_issue == NST - 1 ? 0 : st_issue + 1;                                                         \
  } while (0)
#define MBX_ISSUE_STEP5() do { MBX_ISSUE_STEP5_Y(); MBX_ISSUE_STEP5_X(); } while (0)

    if (nsteps > 0) MBX_ISSUE_STEP5();
    if (nsteps > 1) { MBX_ISSUE_STEP5(); wait_vmcnt<NSUB>(); } else wait_vmcnt<0>();
    int st_pub = 0;                                       // ring slot of the step published next
    lds_readback_wait(lds_readback_issue(smem + (NSUB - 1) * 512 + lw * 64 + lane));   // this lane's slot of the wave's last piece
    raw_barrier();                                        // step 0 has landed
    const int lt = threadIdx.x - 512;                     // 0..511: bias sums of slot lt (row lt >> 3) of every dy image
    float bs[NY][8];
#pragma unroll
    for (int j = 0; j < NY; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) bs[j][e] = 0.f;
    for (int it = 0; it < nsteps; ++it) {
      const bool more = it + 2 < nsteps;
      st_pub = st_pub == NST - 1 ? 0 : st_pub + 1;        // slot of step it+1
#ifndef MBX_NO_PROBE_WG
      if (more) { MBX_ISSUE_STEP5_Y(); wait_vmcnt<NY>(); } else wait_vmcnt<0>();   // step it+1 has retired (this wave's share)
      const unsigned probe = lds_readback_issue(smem + st_pub * STAGE + (NSUB - 1) * 512 + lw * 64 + lane);
      if (more) MBX_ISSUE_STEP5_X();
#else                                                 // (debug builds only: A/B of what the hand-off costs)
      const unsigned probe = 0;
      if (more) { MBX_ISSUE_STEP5(); wait_vmcnt<NSUB>(); } else wait_vmcnt<0>();
#endif
      if (bias) {                                         // dy images of the step being multiplied (landed, read-only now)
        const u32x4* img_y = smem + st_bias * STAGE;
#pragma unroll
        for (int j = 0; j < NY; ++j) {
          const u32x4 v = img_y[j * 512 + lt];
          const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) { bs[j][2 * e] += bf2f(w[e] & 0xffffu); bs[j][2 * e + 1] += bf2f(w[e] >> 16); }
        }
        st_bias = st_bias == NST - 1 ? 0 : st_bias + 1;
      }
#ifndef MBX_NO_PROBE_WG
      lds_readback_wait(probe);                           // read-back returned: publish step it+1
#else
      (void)probe;
#endif
      raw_barrier();
    }
#undef MBX_ISSUE_STEP5_X
#undef MBX_ISSUE_STEP5_Y
#undef MBX_ISSUE_STEP5
    if (bias) {                                           // 64 rows per channel -> LDS -> one adder per channel
      lds_barrier();                                      // (the compute waves are past their last LDS read)
      float* red = reinterpret_cast<float*>(smem);        // [NY][64 rows][64 channels]
      const int row = lt >> 3, cg = (lt & 7) ^ wg_swz64(lt >> 3);     // logical chunk of this thread's slot
#pragma unroll
      for (int j = 0; j < NY; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) red[(j * 64 + row) * 64 + cg * 8 + e] = bs[j][e];
      lds_barrier();
      if (lt < 64 * NY && n0 + lt < p.C_out) {
        const int j = lt >> 6, c = lt & 63;
        float t = 0.f;
        for (int r = 0; r < 64; ++r) t += red[(j * 64 + r) * 64 + c];
        atomicAdd(p.db + n0 + lt, t * p.scale);
      }
    }
    return;
  }

  // ---------------------------------------------------------------------------------------------- compute waves
  // 2 (channels) x 4 (columns) waves; a wave owns A = 2 NY channel blocks x NX column blocks of 16 x 16
  constexpr int A = 2 * NY;
  const int wn = wave & 1, wk = wave >> 1;
  // fragment (transpose-read) lane constants, byte offsets inside a stage
  const int g = lane >> 4, t = lane & 15, fq = t >> 2, pp = t & 3;
  const int lby = (8 * g + fq) * 128 + (pp & 1) * 8;
  const int sxy = ((((fq >> 1) & 1) | ((g & 1) << 1)) << 1);
  int yo[A], xo[NX];
#pragma unroll
  for (int a = 0; a < A; ++a) {
    const int nb = wn * A + a;                                    // channel block 0 .. 4 NY - 1 of the tile
    yo[a] = (nb >> 2) * 8192 + lby + (((2 * (nb & 3) + (pp >> 1)) ^ sxy) << 4);
  }
#pragma unroll
  for (int b = 0; b < NX; ++b) {
    const int kb = wk * NX + b;                                   // column block 0 .. 4 NX - 1
    xo[b] = (NY + (kb >> 2)) * 8192 + lby + (((2 * (kb & 3) + (pp >> 1)) ^ sxy) << 4);
  }
  f32x4 acc[A][NX];
#pragma unroll
  for (int a = 0; a < A; ++a)
#pragma unroll
    for (int b = 0; b < NX; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  int st_comp = 0;
  typedef s16x4 __attribute__((address_space(3))) * lds_tr;
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  raw_barrier();                                          // step 0 has landed
  for (int it = 0; it < nsteps; ++it) {
    if (!(q.dbg & 2)) {
      const char* base = reinterpret_cast<const char*>(smem + st_comp * STAGE);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 yf[A], xf[NX];
        // 192 x 192 tiles: 72 accumulator + 36 fragment registers leave no room for nine loop-invariant fragment
        // addresses under the 128-register budget of a 16-wave block (they spilled: the launch then needs scratch,
        // which costs a ~0.1 ms stall per step when the queue sets it up) -- recompute them from lby instead
        int lby_v = lby;
        if constexpr (A * NX >= 18) asm volatile("" : "+v"(lby_v));
        auto yoff = [&](int a) {
          if constexpr (A * NX >= 18) { const int nb = wn * A + a; return (nb >> 2) * 8192 + lby_v + (((2 * (nb & 3) + (pp >> 1)) ^ sxy) << 4); }
          else return yo[a];
        };
        auto xoff = [&](int b) {
          if constexpr (A * NX >= 18) { const int kb = wk * NX + b; return (NY + (kb >> 2)) * 8192 + lby_v + (((2 * (kb & 3) + (pp >> 1)) ^ sxy) << 4); }
          else return xo[b];
        };
#pragma unroll
        for (int a = 0; a < A; ++a) {
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(base + yoff(a) + kk * 4096));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(base + yoff(a) + kk * 4096 + 512));
          const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          yf[a] = __builtin_bit_cast(bf16x8, v);
        }
#pragma unroll
        for (int b = 0; b < NX; ++b) {
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(base + xoff(b) + kk * 4096));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(base + xoff(b) + kk * 4096 + 512));
          const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          xf[b] = __builtin_bit_cast(bf16x8, v);
        }
#pragma unroll
        for (int a = 0; a < A; ++a)
#pragma unroll
          for (int b = 0; b < NX; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[a], xf[b], acc[a][b], 0, 0, 0);
      }
    }
    st_comp = st_comp == NST - 1 ? 0 : st_comp + 1;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // this wave's LDS reads are done before the stage is reused
    raw_barrier();
  }
  if (bias) { lds_barrier(); lds_barrier(); }             // the loaders reduce the bias sums through LDS meanwhile
#pragma unroll
  for (int a = 0; a < A; ++a) {
    const int nb = n0 + (wn * A + a) * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int b = 0; b < NX; ++b) {
      const int kc = k0 + (wk * NX + b) * 16 + (lane & 15);
      if (kc >= p.Ktot) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (nb + r >= p.C_out) continue;
        float* dst = p.dw + (size_t)(nb + r) * p.Ktot + kc;
        if (single) *dst = acc[a][b][r] * p.scale;        // dw is zero before the launch and this block is its only adder
        else atomicAdd(dst, acc[a][b][r] * p.scale);
      }
    }
  }
}


// ------------------------------------------------------------------------------------------
// GROUPED weight gradient: ONE launch for the weight gradients of many layers (a whole backward segment).
// The weight gradient is off the critical path of the backward pass (only the optimiser consumes dW), so the engine
// keeps every layer's dy and runs them together: the grid is a table of work items (layer, output tile, pixel
// range), longest first.  With hundreds of tiles from dozens of layers in flight, a tile's pixel reduction is
// split across blocks only when it is longer than a fair share of one CU's work: most tiles have ONE adder
// (no atomic traffic to speak of, bit-reproducible), loops run for hundreds of steps instead of a dozen, and
// there is one launch tail per segment instead of one per layer.
struct WgradLayer { WgradK2 q; int narrow, lin, pad0, pad1; };
struct WgradItem { int layer, tile_n, tile_k, m_begin, m_end, single, cfg, pad2; };   // single: the only adder of its dw tile;
                                                                                         // cfg: tile shape, index into kWgCfgs
constexpr int kWgradLds = 3 * 3 * 16384;               // wgrad5: three stages x up to six 8 KB sub-images (NY dy + NX x) = 144 KB
constexpr int kQueues = 8;                             // one work queue per XCD
constexpr int kCounterStride = 32;                     // ints: every queue head on its own 128-byte line

// PERSISTENT: one 1024-thread block per CU (8 MFMA + 8 loader waves, 144 KB + 16 B of LDS); a block reads the id of the XCD it runs on and pulls items from THAT
// XCD's queue (one returning atomic per item), then steals from the other queues.  The host deals whole panel groups
// -- all output tiles of one (layer, pixel range), which stream the same dy / x rows -- to one queue, so the ~32
// blocks that share an L2 walk the same pixels at the same time and all but the first read of a row is an L2 hit
// (LDS-DMA from the XCD's L2 runs at twice the rate of the Infinity Cache, MI355X_MICROARCH.md "Indexed rows").
// Placement is for speed only: any block may run any item.
// tile shapes (NY, NX) the grouped launch is instantiated for: index = WgradItem.cfg
constexpr int kWgCfgs[][2] = {{1, 4}, {1, 5}, {2, 2}, {2, 3}, {2, 4}, {3, 2}, {3, 3}};
constexpr int kNumWgCfgs = sizeof(kWgCfgs) / sizeof(kWgCfgs[0]);

__global__ void __launch_bounds__(64 * (8 + kWgLoaders))
conv_wgrad_grouped_kernel(const WgradLayer* __restrict__ layers, const WgradItem* __restrict__ items,
                          const int* __restrict__ qrange /*[2][kQueues]: begin | end*/, int* __restrict__ heads) {
  extern __shared__ __attribute__((aligned(16))) u32x4 smem[];
  volatile int* s_idx = reinterpret_cast<volatile int*>(smem + kWgradLds / 16);     // one word past the rings
  const int xcd = __builtin_amdgcn_s_getreg((3 << 11) | 20) & (kQueues - 1);         // HW_REG_XCC_ID[3:0]
  int n_done = 0;                                        // work items this block has processed (block-uniform)
  for (int q = 0; q < kQueues; ++q) {
    const int qx = (xcd + q) & (kQueues - 1);
    const int qb = qrange[qx], qe = qrange[kQueues + qx];
    if (qb >= qe) continue;
    for (;;) {
      lds_barrier();                                     // everyone is done with the previous item (LDS, s_idx)
      // dequeue by a LOADER lane: its wave has nothing in flight, while a compute wave's returning atomic would queue
      // behind the dw atomics it has just fired (vmcnt retires in order)
      if (threadIdx.x == 512) *s_idx = qb + atomicAdd(heads + qx * kCounterStride, 1);
      lds_barrier();
      const int idx = __builtin_amdgcn_readfirstlane(*s_idx);
      if (idx >= qe) break;
      const WgradItem it = items[idx];                   // block-uniform: scalar loads
      const WgradK2 q2 = layers[it.layer].q;
#define MBX_WG_CASE(I)                                                                                         \
      case I: wgrad5_body<kWgCfgs[I][0], kWgCfgs[I][1]>(q2, smem, it.tile_n, it.tile_k, it.m_begin, it.m_end, it.single); break;
      switch (it.cfg) {
        MBX_WG_CASE(0) MBX_WG_CASE(1) MBX_WG_CASE(2) MBX_WG_CASE(3) MBX_WG_CASE(4) MBX_WG_CASE(5) MBX_WG_CASE(6)
        default: break;
      }
#undef MBX_WG_CASE
      ++n_done;
    }
  }
  // Leave the queue heads at zero for the next launch: the LAST block to get here (every other block has left its
  // dequeue loops) resets them.  (A hipMemsetAsync in front of the kernel did this first; as a memset NODE of a captured
  // graph replayed hundreds of times with the host far ahead it ended in GPU memory-access faults, 4 of 10 400-step
  // runs -- the launch now carries no memset.)
  // The tally line behind the counters is never reset: [0] work items processed, [1] launches completed, both cumulative.
  // The host checks items == launches x n_items at its health checks (ops.WgradGroup.completed_ok): a launch that found
  // stale heads (after an aborted launch) would otherwise compute nothing -- dW all zeros -- without any error.
  lds_barrier();
  if (threadIdx.x == 0) {
    unsigned long long* tally = reinterpret_cast<unsigned long long*>(heads + (kQueues + 1) * kCounterStride);
    if (n_done) atomicAdd(tally, (unsigned long long)n_done);
    int* exits = heads + kQueues * kCounterStride;
    if (atomicAdd(exits, 1) == (int)gridDim.x - 1) {
      for (int q = 0; q < kQueues; ++q) atomicExch(heads + q * kCounterStride, 0);
      atomicExch(exits, 0);
      atomicAdd(tally + 1, 1ull);
    }
  }
}

// ------------------------------------------------------------------------------- host side
// One instantiation of the single-layer kernel: its dynamic-LDS limit is raised once, at the first launch.
template <int NYF, int NG, bool LIN, bool BIAS>
void launch_wgrad2(const WgradK2& k2, const dim3 grid, hipStream_t s) {
  constexpr int kLds = NG * kWg2Stages * wg2_stage_slots(NYF) * 16;     // per 4-wave group: two stages of 32 KB | 24 KB
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wgrad2_kernel<NYF, kWg2Stages, NG, LIN, BIAS>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
  (void)attr;
  hipLaunchKernelGGL((conv_wgrad2_kernel<NYF, kWg2Stages, NG, LIN, BIAS>), grid, dim3(NG * kThreads), kLds, s, k2);
}

// mbx_conv_desc.tile_config selects the block shape for the weight gradient too: 0 library default (eight waves,
// 256 blocks: one per CU), 1 eight waves / 256, 2 four waves / 512 (two per CU), 3 eight waves / 192, 4 four waves / 384,
// 5 eight waves / 128, 6 eight waves / 224; 7 - 10: the narrow tile (64 output channels per block; needs dense dy, the
// wide tile otherwise) with eight waves / 256, eight / 192, four / 512, four / 768; 11 eight waves, un-split: one block
// per tile, every dw element has ONE adder (bit-reproducible)
struct Wg2Cfg { int ng, target; bool narrow; };       // 4-wave groups per block, blocks to split the pixels for, tile
constexpr Wg2Cfg kWg2Cfgs[] = {{2, 256, false}, {1, 512, false}, {2, 192, false}, {1, 384, false}, {2, 128, false}, {2, 224, false},
                               {2, 256, true}, {2, 192, true}, {1, 512, true}, {1, 768, true}, {2, 1, false}};   // tile_config 1..11
constexpr int kNumWg2Cfgs = sizeof(kWg2Cfgs) / sizeof(kWg2Cfgs[0]);

}  // namespace

// Geometry / pointers of one layer's weight gradient (shared by the one-layer launch and the grouped plan).
static int fill_wgrad(const mbx_conv_desc* d, const void* dy, int64_t dy_img_stride, int32_t ld_dy, float scale,
                      float* dw, float* db, WgradK2& k2) {
  int st = check_desc(d);
  if (st != MBX_OK) return st;
  if (!dy || !dw || d->transposed) return MBX_ERR_INVALID_ARG;
  if (ld_dy % 8 || ld_dy < ((d->C_out + 7) / 8) * 8 || (reinterpret_cast<uintptr_t>(dy) & 15)) return MBX_ERR_INVALID_ARG;
  if ((long long)d->N * dy_img_stride >= (1LL << 30)) return MBX_ERR_UNSUPPORTED;
  WgradK& k = k2.b;
  k.x = reinterpret_cast<const unsigned short*>(d->x);
  k.x_img_stride = (int)d->x_img_stride; k.ldx = d->ldx; k.H_in = d->H_in; k.W_in = d->W_in; k.C_in = d->C_in;
  k.dy = reinterpret_cast<const unsigned short*>(dy); k.dy_img_stride = (int)dy_img_stride; k.ld_dy = ld_dy;
  k.C_out = d->C_out; k.S = d->S; k.Ktot = d->R * d->S * d->C_in;
  k.stride = d->stride; k.pad_t = d->pad_t; k.pad_l = d->pad_l; k.W_out = d->W_out; k.HW_out = d->H_out * d->W_out;
  k.M = d->N * k.HW_out;
  k.dw = dw; k.db = db; k.scale = scale;
  set_magic((unsigned)k.HW_out, k.mg_hw, k.sh_hw);
  set_magic((unsigned)k.W_out, k.mg_w, k.sh_w);
  k.H_out = d->H_out;
  k.x_bytes = (unsigned)(2 * ((long long)(d->N - 1) * d->x_img_stride + ((long long)d->H_in * d->W_in - 1) * d->ldx + d->C_in));
  k.dy_bytes = (unsigned)(2 * ((long long)(d->N - 1) * dy_img_stride + ((long long)k.HW_out - 1) * ld_dy + ((d->C_out + 7) / 8) * 8));
  k.tiles_n = (k.C_out + 127) / 128;
  k.tiles_k = (k.Ktot + 127) / 128;
  k.m_per_split = k.M;
  k2.pw = (d->R == 1 && d->S == 1 && d->pad_t == 0 && d->pad_l == 0 && d->stride == 1 &&
           d->x_img_stride == (int64_t)d->H_in * d->W_in * d->ldx) ? 1 : 0;
  k2.ydense = (dy_img_stride == (int64_t)k.HW_out * ld_dy) ? 1 : 0;
  static const int dbg = mbx_env_int("MBX_WG_DBG", 0);
  k2.dbg = dbg;
  return MBX_OK;
}

extern "C" int mbx_conv_wgrad_scaled(const mbx_conv_desc* d, const void* dy, int64_t dy_img_stride, int32_t ld_dy,
                                     float scale, float* dw, float* db, mbx_stream_t stream) {
  WgradK2 k2;
  int st = fill_wgrad(d, dy, dy_img_stride, ld_dy, scale, dw, db, k2);
  if (st != MBX_OK) return st;
  MBX_ENTER();
  WgradK& k = k2.b;
  // the block shape: mbx_conv_desc.tile_config (kWg2Cfgs), or the library default (which the environment may change)
  static const int env_ng = mbx_env_char("MBX_WGRAD_NG") == '1' ? 1 : 2, env_target = mbx_env_int("MBX_WGRAD_TARGET", -1);
  const Wg2Cfg cfg = (d->tile_config >= 1 && d->tile_config <= kNumWg2Cfgs)
                         ? kWg2Cfgs[d->tile_config - 1]
                         : Wg2Cfg{env_ng, env_target > 0 ? env_target : (env_ng == 1 ? 512 : 256), false};
  const int ng = cfg.ng, target = cfg.target;
  const bool narrow = cfg.narrow && k2.ydense;
  k.tiles_n = narrow ? (k.C_out + 63) / 64 : (k.C_out + 127) / 128;
  const int tiles = k.tiles_n * k.tiles_k;
  // split the pixel reduction so that ~2 blocks per CU exist, at least 256 pixels per split
  int splits = target / tiles;                 // floor: all blocks resident in one round
  const int max_splits = (k.M + 511) / 512;
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  int mps = (k.M + splits - 1) / splits;
  mps = ((mps + 63) / 64) * 64;
  splits = (k.M + mps - 1) / mps;
  k.m_per_split = mps;
  const bool lin = k2.pw && k2.ydense, bias = db != nullptr;
  const dim3 grid(tiles * splits);
  hipStream_t s = mbx_s(stream);
  switch ((narrow ? 8 : 0) | (ng == 2 ? 4 : 0) | (lin ? 2 : 0) | (bias ? 1 : 0)) {
#define MBX_WG2(I) case I: launch_wgrad2<((I) & 8) ? 2 : 4, ((I) & 4) ? 2 : 1, ((I) & 2) != 0, ((I) & 1) != 0>(k2, grid, s); break;
    MBX_WG2(0) MBX_WG2(1) MBX_WG2(2) MBX_WG2(3) MBX_WG2(4) MBX_WG2(5) MBX_WG2(6) MBX_WG2(7)
    MBX_WG2(8) MBX_WG2(9) MBX_WG2(10) MBX_WG2(11) MBX_WG2(12) MBX_WG2(13) MBX_WG2(14) MBX_WG2(15)
#undef MBX_WG2
  }
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

// ------------------------------------------------------------------------------------ grouped weight gradient
// Host-side plan: [WgradLayer x n_jobs | WgradItem x n_items] image that the caller copies to device memory once.
struct PlanJob { int cfg, ny, nx, tiles_n, tiles_k, steps, splits; double step_cost; };
struct PlanGroup { int job, m_begin, m_end, tiles; double len; };     // all output tiles of one (layer, pixel range)

static void plan_jobs(const mbx_wgrad_job* jobs, int n_jobs, int flags, std::vector<PlanJob>& pj) {
  // Tile shape per layer: the launch is bound by the bytes a CU pulls through the L2 -> LDS path (8 KB per sub-image and
  // 64-pixel step, ~390 cycles at the measured ~45 GB/s per CU) unless the MFMAs of the step take longer (128 NY NX
  // cycles: 4 NY NX per wave, 16 cycles each, two compute waves per SIMD) -- take the shape with the smallest total.
  // Work unit for splitting: one 64-pixel step of one tile, weighted by that cost.  A tile is split only when it is
  // longer than a quarter of a CU's fair share of the whole group (and never below 16 steps per piece): most tiles keep
  // a single adder.
  double total = 0.0;
  pj.resize(n_jobs);
  for (int j = 0; j < n_jobs; ++j) {
    const mbx_conv_desc& d = jobs[j].desc;
    const long long M = (long long)d.N * d.H_out * d.W_out;
    const int Ktot = d.R * d.S * d.C_in;
    double best = 1e300;
    static const int max_cfg = mbx_env_int("MBX_WG_MAXCFG", kNumWgCfgs);       // bisecting aid
    for (int c = 0; c < kNumWgCfgs && c < max_cfg; ++c) {
      const int ny = kWgCfgs[c][0], nx = kWgCfgs[c][1];
      const int tn = (d.C_out + 64 * ny - 1) / (64 * ny), tk = (Ktot + 64 * nx - 1) / (64 * nx);
      const double dma = 390.0 * (ny + nx), mfma = 128.0 * ny * nx;
      const double step = dma > mfma ? dma : mfma;
      const double cost = (double)tn * tk * step;
      if (cost < best) { best = cost; pj[j].cfg = c; pj[j].ny = ny; pj[j].nx = nx; pj[j].tiles_n = tn; pj[j].tiles_k = tk; pj[j].step_cost = step / (390.0 * 6); }
    }
    pj[j].steps = (int)((M + 63) / 64);
    total += (double)pj[j].tiles_n * pj[j].tiles_k * pj[j].steps * pj[j].step_cost;
  }
  const double share = total / conv_cus();
  static double wdiv = 0.0;
  if (wdiv == 0.0) { const char* e = getenv("MBX_WG_WMAX_DIV"); wdiv = e ? atof(e) : 4.0; if (wdiv <= 0.0) wdiv = 4.0; }   // (A/B knob)
  double wmax = share / wdiv;
  if (wmax < 16.0) wmax = 16.0;
  for (int j = 0; j < n_jobs; ++j) {
    int splits = (flags & MBX_WGRAD_DETERMINISTIC) ? 1 : (int)((pj[j].steps * pj[j].step_cost + wmax - 1) / wmax);
    const int max_splits = (pj[j].steps + 15) / 16;
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    pj[j].splits = splits;
  }
}

// Panel groups dealt to the XCD queues: longest items first (the short ones fill the tail), each group to the queue
// with the least work so far; a queue keeps that order.  MBX_WGRAD_SCATTER (A/B knob) deals single items instead.
static void plan_queues(const mbx_wgrad_job* jobs, int n_jobs, int flags, const std::vector<PlanJob>& pj,
                        std::vector<WgradItem>& items, int* qrange) {
  std::vector<PlanGroup> groups;
  for (int j = 0; j < n_jobs; ++j) {
    const mbx_conv_desc& d = jobs[j].desc;
    const long long M = (long long)d.N * d.H_out * d.W_out;
    long long mps = (M + pj[j].splits - 1) / pj[j].splits;
    mps = ((mps + 63) / 64) * 64;
    for (long long b = 0; b < M; b += mps) {
      PlanGroup g;
      g.job = j; g.m_begin = (int)b; g.m_end = (int)(b + mps < M ? b + mps : M);
      g.tiles = pj[j].tiles_n * pj[j].tiles_k;
      g.len = (double)((g.m_end - g.m_begin + 63) / 64) * pj[j].step_cost;
      groups.push_back(g);
    }
  }
  std::stable_sort(groups.begin(), groups.end(), [](const PlanGroup& a, const PlanGroup& b) {
    return a.len != b.len ? a.len > b.len : a.tiles > b.tiles;
  });
  std::vector<WgradItem> q[kQueues];
  double load[kQueues] = {0};
  int rr = 0;
  for (const PlanGroup& g : groups) {
    for (int tk = 0; tk < pj[g.job].tiles_k; ++tk)
      for (int tn = 0; tn < pj[g.job].tiles_n; ++tn) {
        int best = 0;
        if (flags & MBX_WGRAD_SCATTER) best = rr++ % kQueues;
        else if (tk == 0 && tn == 0) { for (int x = 1; x < kQueues; ++x) if (load[x] < load[best]) best = x; rr = best; }
        else best = rr;
        WgradItem I;
        memset(&I, 0, sizeof(I));
        I.layer = g.job; I.tile_n = tn; I.tile_k = tk; I.m_begin = g.m_begin; I.m_end = g.m_end;
        I.single = pj[g.job].splits == 1 ? 1 : 0;
        I.cfg = pj[g.job].cfg;
        q[best].push_back(I);
        load[best] += g.len;
      }
  }
  items.clear();
  for (int x = 0; x < kQueues; ++x) {
    qrange[x] = (int)items.size();
    items.insert(items.end(), q[x].begin(), q[x].end());
    qrange[kQueues + x] = (int)items.size();
  }
}

static size_t plan_image_bytes(int n_jobs, size_t n_items, int64_t* items_off, int64_t* queues_off, int64_t* heads_off,
                               int64_t* tally_off = nullptr) {
  size_t o = sizeof(WgradLayer) * (size_t)n_jobs;
  if (items_off) *items_off = (int64_t)o;
  o += sizeof(WgradItem) * n_items;
  o = (o + 127) / 128 * 128;
  if (queues_off) *queues_off = (int64_t)o;
  o += 128;                                            // qrange: 2 x kQueues ints
  if (heads_off) *heads_off = (int64_t)o;
  o += (size_t)(kQueues + 1) * kCounterStride * sizeof(int);            // queue heads + the exit counter, a line each
  if (tally_off) *tally_off = (int64_t)o;
  o += (size_t)kCounterStride * sizeof(int);                            // tally line: items processed | launches completed (uint64)
  return o;
}

extern "C" size_t mbx_wgrad_plan_bytes(const mbx_wgrad_job* jobs, int n_jobs, int flags) {
  if (!jobs || n_jobs <= 0) return 0;
  std::vector<PlanJob> pj;
  std::vector<WgradItem> items;
  int qrange[2 * kQueues];
  plan_jobs(jobs, n_jobs, flags, pj);
  plan_queues(jobs, n_jobs, flags, pj, items, qrange);
  return plan_image_bytes(n_jobs, items.size(), nullptr, nullptr, nullptr);
}

extern "C" int mbx_wgrad_plan(const mbx_wgrad_job* jobs, int n_jobs, int flags, void* host_image, size_t bytes,
                              mbx_wgrad_plan_info* info) {
  if (!jobs || n_jobs <= 0 || !host_image || !info) return MBX_ERR_INVALID_ARG;
  std::vector<PlanJob> pj;
  std::vector<WgradItem> items;
  int qrange[2 * kQueues];
  plan_jobs(jobs, n_jobs, flags, pj);
  plan_queues(jobs, n_jobs, flags, pj, items, qrange);
  int64_t items_off, queues_off, heads_off, tally_off;
  const size_t need = plan_image_bytes(n_jobs, items.size(), &items_off, &queues_off, &heads_off, &tally_off);
  if (bytes < need || items.size() >= (1ull << 30)) return MBX_ERR_WORKSPACE;
  memset(host_image, 0, need);
  char* base = reinterpret_cast<char*>(host_image);
  WgradLayer* layers = reinterpret_cast<WgradLayer*>(base);
  double flops = 0.0;
  for (int j = 0; j < n_jobs; ++j) {
    const mbx_wgrad_job& J = jobs[j];
    WgradLayer& L = layers[j];
    const int status = fill_wgrad(&J.desc, J.dy, J.dy_img_stride, J.ld_dy, J.scale, J.dw, J.db, L.q);
    if (status != MBX_OK) return status;
    L.narrow = 0;
    L.lin = (L.q.pw && L.q.ydense) ? 1 : 0;
    L.q.b.tiles_n = pj[j].tiles_n;
    flops += 2.0 * L.q.b.M * (double)L.q.b.C_out * L.q.b.Ktot;
  }
  memcpy(base + items_off, items.data(), sizeof(WgradItem) * items.size());
  memcpy(base + queues_off, qrange, sizeof(qrange));
  info->n_layers = n_jobs;
  info->n_items = (int32_t)items.size();
  info->layers_off = 0;
  info->items_off = items_off;
  info->queues_off = queues_off;
  info->heads_off = heads_off;
  info->tally_off = tally_off;
  info->flops = flops;
  return MBX_OK;
}

extern "C" int mbx_conv_wgrad_grouped(void* device_image, const mbx_wgrad_plan_info* info, mbx_stream_t stream) {
  return mbx_conv_wgrad_grouped_capped(device_image, info, 0, stream);
}

extern "C" int mbx_conv_wgrad_grouped_capped(void* device_image, const mbx_wgrad_plan_info* info, int max_workgroups,
                                             mbx_stream_t stream) {
  if (!device_image || !info || info->n_items <= 0 || info->n_layers <= 0) return MBX_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(device_image) & 15) return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  static bool attr = false;
  constexpr int kLds = kWgradLds + 16;                 // + the broadcast word of the item index
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wgrad_grouped_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
    attr = true;
  }
  char* base = reinterpret_cast<char*>(device_image);
  hipStream_t s = mbx_s(stream);
  // (queue heads: zero in the plan image, and reset by the kernel's last block at the end of every launch)
  int blocks = info->n_items < conv_cus() ? info->n_items : conv_cus();            // one persistent block per CU
  if (max_workgroups > 0 && blocks > max_workgroups) blocks = max_workgroups;     // (the queues are drained by any number)
  hipLaunchKernelGGL(conv_wgrad_grouped_kernel, dim3(blocks), dim3(64 * (8 + kWgLoaders)), kLds, s,
                     reinterpret_cast<const WgradLayer*>(base + info->layers_off),
                     reinterpret_cast<const WgradItem*>(base + info->items_off),
                     reinterpret_cast<const int*>(base + info->queues_off),
                     reinterpret_cast<int*>(base + info->heads_off));
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_conv_wgrad(const mbx_conv_desc* d, const void* dy, int64_t dy_img_stride, int32_t ld_dy,
                              float* dw, float* db, mbx_stream_t stream) {
  return mbx_conv_wgrad_scaled(d, dy, dy_img_stride, ld_dy, 1.0f, dw, db, stream);
}
