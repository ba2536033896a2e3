// libmbx: pooling (fwd/bwd), relu mask, head gather/scatter, input packing, step begin and filter preparation (batch norm:
// bn.hip; the optimiser step and global-norm clipping: optim.hip).  All HBM-bound: 16-byte (8 x bf16) accesses per lane along
// the NHWC channel axis (vec8.h), grid-stride loops capped at 2048 blocks.
#include "vec8.h"

namespace {

// ------------------------------------------------------------------------------- pooling
// KK / SS: window and stride fixed at compile time (3 / 2: every max pool of the network) so that the nine loads of
// a window are independent and in flight together; 0 = run-time values.
template <int KK, int SS>
__global__ void __launch_bounds__(kT)
maxpool_fwd_kernel(const unsigned short* __restrict__ x, long long xs, int ldx, int N, int H, int W, int C, int k_,
                   int stride_, unsigned short* __restrict__ y, long long ys, int ldy, int Ho, int Wo,
                   unsigned char* __restrict__ argmax) {
  const int k = KK ? KK : k_, stride = SS ? SS : stride_;
  const int C8 = C >> 3;
  const unsigned total = (unsigned)N * Ho * Wo * C8;            // < 2^31 (checked on the host): 32-bit index math
  for (unsigned i = blockIdx.x * kT + threadIdx.x; i < total; i += gridDim.x * kT) {
    unsigned t = i / (unsigned)C8;
    const int c = (int)(i - t * C8) << 3;
    const unsigned t2 = t / (unsigned)Wo;
    const int ow = (int)(t - t2 * Wo);
    const int n = (int)(t2 / (unsigned)Ho);
    const int oh = (int)(t2 - (unsigned)n * Ho);
    float best[8];
    unsigned arg[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; arg[j] = 0; }
    if constexpr (KK > 0) {
      u32x4 v[KK * KK];
#pragma unroll
      for (int r = 0; r < KK; ++r)
#pragma unroll
        for (int s = 0; s < KK; ++s) {
          const int h = oh * stride + r, w = ow * stride + s;
          v[r * KK + s] = (h < H && w < W) ? ld8(x + n * xs + ((long long)h * W + w) * ldx + c) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
      for (int r = 0; r < KK; ++r)
#pragma unroll
        for (int s = 0; s < KK; ++s) {
          const int h = oh * stride + r, w = ow * stride + s;
          if (h >= H || w >= W) continue;
          float f[8];
          unpack8(v[r * KK + s], f);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (f[j] > best[j]) { best[j] = f[j]; arg[j] = r * KK + s; }
        }
    } else {
      for (int r = 0; r < k; ++r)
        for (int s = 0; s < k; ++s) {
          const int h = oh * stride + r, w = ow * stride + s;
          if (h >= H || w >= W) continue;
          float f[8];
          unpack8(ld8(x + n * xs + ((long long)h * W + w) * ldx + c), f);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (f[j] > best[j]) { best[j] = f[j]; arg[j] = r * k + s; }
        }
    }
    st8(y + n * ys + ((long long)oh * Wo + ow) * ldy + c, pack8(best));
    if (argmax) {
      u32x2 av;
      av.x = arg[0] | (arg[1] << 8) | (arg[2] << 16) | (arg[3] << 24);
      av.y = arg[4] | (arg[5] << 8) | (arg[6] << 16) | (arg[7] << 24);
      *reinterpret_cast<u32x2*>(argmax + (((long long)n * Ho + oh) * Wo + ow) * C + c) = av;
    }
  }
}

template <int KK, int SS>
__global__ void __launch_bounds__(kT)
maxpool_bwd_kernel(const unsigned short* __restrict__ dy, long long dys, int ld_dy,
                   const unsigned char* __restrict__ argmax, int N, int H, int W, int C, int k_, int stride_, int Ho,
                   int Wo, unsigned short* __restrict__ dx, long long dxs, int ld_dx, int accumulate) {
  const int k = KK ? KK : k_, stride = SS ? SS : stride_;
  const int C8 = C >> 3;
  const unsigned total = (unsigned)N * H * W * C8;              // < 2^31 (checked on the host): 32-bit index math
  for (unsigned i = blockIdx.x * kT + threadIdx.x; i < total; i += gridDim.x * kT) {
    unsigned t = i / (unsigned)C8;
    const int c = (int)(i - t * C8) << 3;
    const unsigned t2 = t / (unsigned)W;
    const int w = (int)(t - t2 * W);
    const int n = (int)(t2 / (unsigned)H);
    const int h = (int)(t2 - (unsigned)n * H);
    float acc[8];
    unsigned short* dst = dx + n * dxs + ((long long)h * W + w) * ld_dx + c;
    if (accumulate) unpack8(ld8(dst), acc);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    }
    if constexpr (KK > 0) {
      // the (at most NW x NW) windows covering (h, w), ascending like the run-time loops: all loads first
      constexpr int NW = (KK + SS - 1) / SS;
      const int ohb = h / SS, owb = w / SS;
      u32x4 gv[NW * NW];
      u32x2 av[NW * NW];
      bool ok[NW * NW];
#pragma unroll
      for (int a = 0; a < NW; ++a)
#pragma unroll
        for (int b = 0; b < NW; ++b) {
          const int oh = ohb - (NW - 1 - a), ow = owb - (NW - 1 - b);
          const bool v = oh >= 0 && oh < Ho && ow >= 0 && ow < Wo && h - oh * SS < KK && w - ow * SS < KK;
          ok[a * NW + b] = v;
          const long long o = ((long long)n * Ho + (v ? oh : 0)) * Wo + (v ? ow : 0);
          av[a * NW + b] = v ? *reinterpret_cast<const u32x2*>(argmax + o * C + c) : u32x2{0u, 0u};
          gv[a * NW + b] = v ? ld8(dy + n * dys + ((long long)oh * Wo + ow) * ld_dy + c) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
      for (int a = 0; a < NW; ++a)
#pragma unroll
        for (int b = 0; b < NW; ++b) {
          if (!ok[a * NW + b]) continue;
          const int oh = ohb - (NW - 1 - a), ow = owb - (NW - 1 - b);
          const unsigned tap = (h - oh * SS) * KK + (w - ow * SS);
          float g[8];
          unpack8(gv[a * NW + b], g);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const unsigned aj = ((j < 4 ? av[a * NW + b].x : av[a * NW + b].y) >> (8 * (j & 3))) & 0xffu;
            if (aj == tap) acc[j] += g[j];
          }
        }
    } else {
      int oh0 = (h - k + stride) / stride;          // ceil((h-k+1)/stride) for h-k+1 > -stride
      if (h - k + 1 <= 0) oh0 = 0;
      int ow0 = (w - k + stride) / stride;
      if (w - k + 1 <= 0) ow0 = 0;
      const int oh1 = min(h / stride, Ho - 1), ow1 = min(w / stride, Wo - 1);
      for (int oh = oh0; oh <= oh1; ++oh)
        for (int ow = ow0; ow <= ow1; ++ow) {
          const unsigned tap = (h - oh * stride) * k + (w - ow * stride);
          const long long o = ((long long)n * Ho + oh) * Wo + ow;
          const u32x2 av = *reinterpret_cast<const u32x2*>(argmax + o * C + c);
          float g[8];
          unpack8(ld8(dy + n * dys + ((long long)oh * Wo + ow) * ld_dy + c), g);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const unsigned aj = ((j < 4 ? av.x : av.y) >> (8 * (j & 3))) & 0xffu;
            if (aj == tap) acc[j] += g[j];
          }
        }
    }
    st8(dst, pack8(acc));
  }
}

__global__ void __launch_bounds__(kT)
avgpool_fwd_kernel(const unsigned short* __restrict__ x, long long xs, int ldx, int N, int H, int W, int C, int k,
                   int pad, unsigned short* __restrict__ y, long long ys, int ldy, int Ho, int Wo) {
  const int C8 = C >> 3;
  const unsigned total = (unsigned)N * Ho * Wo * C8;            // < 2^31 (checked on the host): 32-bit index math
  for (unsigned i = blockIdx.x * kT + threadIdx.x; i < total; i += gridDim.x * kT) {
    unsigned t = i / (unsigned)C8;
    const int c = (int)(i - t * C8) << 3;
    const unsigned t2 = t / (unsigned)Wo;
    const int ow = (int)(t - t2 * Wo);
    const int n = (int)(t2 / (unsigned)Ho);
    const int oh = (int)(t2 - (unsigned)n * Ho);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    int cnt = 0;
    if (k == 3) {
      // the 3x3 pool of Mixed_5b (model.py:134): ALL nine taps' loads in flight, added in tap order (as the loop below adds
      // them: same values).  Row by row the launch was three dependent round trips per output: 19 us for 15 MB.
      u32x4 v[9];
      bool ok[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int h = oh - pad + r, w = ow - pad + q;
          ok[r * 3 + q] = (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
          v[r * 3 + q] = ok[r * 3 + q] ? ld8(x + n * xs + ((long long)h * W + w) * ldx + c) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
      for (int tq = 0; tq < 9; ++tq) {
        if (!ok[tq]) continue;
        float f[8];
        unpack8(v[tq], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += f[j];
        ++cnt;
      }
    } else
    // eight taps' loads in flight at a time, added in tap order (the 8x8 head pool read its 64 taps one dependent load after
    // the other: 24 us for 12 MB)
    for (int r = 0; r < k; ++r) {
      const int h = oh - pad + r;
      if ((unsigned)h >= (unsigned)H) continue;
      const unsigned short* row = x + n * xs + (long long)h * W * ldx + c;
      for (int s0 = 0; s0 < k; s0 += 8) {                 // (eight: a whole row of the 8x8 head pool, model.py:285)
        u32x4 v[8];
        bool ok[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int w = ow - pad + s0 + q;
          ok[q] = s0 + q < k && (unsigned)w < (unsigned)W;
          v[q] = ok[q] ? ld8(row + (long long)w * ldx) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          if (!ok[q]) continue;
          float f[8];
          unpack8(v[q], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += f[j];
          ++cnt;
        }
      }
    }
    const float inv = 1.0f / (float)cnt;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= inv;
    st8(y + n * ys + ((long long)oh * Wo + ow) * ldy + c, pack8(acc));
  }
}

__global__ void __launch_bounds__(kT)
avgpool_bwd_kernel(const unsigned short* __restrict__ dy, long long dys, int ld_dy, int N, int H, int W, int C, int k,
                   int pad, int Ho, int Wo, unsigned short* __restrict__ dx, long long dxs, int ld_dx,
                   int accumulate) {
  const int C8 = C >> 3;
  const unsigned total = (unsigned)N * H * W * C8;              // < 2^31 (checked on the host): 32-bit index math
  for (unsigned i = blockIdx.x * kT + threadIdx.x; i < total; i += gridDim.x * kT) {
    unsigned t = i / (unsigned)C8;
    const int c = (int)(i - t * C8) << 3;
    const unsigned t2 = t / (unsigned)W;
    const int w = (int)(t - t2 * W);
    const int n = (int)(t2 / (unsigned)H);
    const int h = (int)(t2 - (unsigned)n * H);
    float acc[8];
    unsigned short* dst = dx + n * dxs + ((long long)h * W + w) * ld_dx + c;
    if (accumulate) unpack8(ld8(dst), acc);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    }
    const int oh0 = max(h + pad - k + 1, 0), oh1 = min(h + pad, Ho - 1);
    const int ow0 = max(w + pad - k + 1, 0), ow1 = min(w + pad, Wo - 1);
    if (k == 3) {
      // all (at most nine) windows' loads in flight, added in the order of the loops below (same values): as dependent
      // loads the launch took ten round trips per element (35 us for 45 MB)
      u32x4 v[9];
      float inv[9];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const int oh = oh0 + a, ow = ow0 + b;
          const bool ok = oh <= oh1 && ow <= ow1;
          const int nh = min(oh - pad + 3, H) - max(oh - pad, 0), nw = min(ow - pad + 3, W) - max(ow - pad, 0);
          inv[a * 3 + b] = ok ? 1.0f / (float)(nh * nw) : 0.f;
          v[a * 3 + b] = ok ? ld8(dy + n * dys + ((long long)oh * Wo + ow) * ld_dy + c) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
      for (int tq = 0; tq < 9; ++tq) {
        if (inv[tq] == 0.f) continue;
        float g[8];
        unpack8(v[tq], g);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += g[j] * inv[tq];
      }
    } else
    for (int oh = oh0; oh <= oh1; ++oh) {
      const int nh = min(oh - pad + k, H) - max(oh - pad, 0);
      for (int ow = ow0; ow <= ow1; ++ow) {
        const int nw = min(ow - pad + k, W) - max(ow - pad, 0);
        const float inv = 1.0f / (float)(nh * nw);
        float g[8];
        unpack8(ld8(dy + n * dys + ((long long)oh * Wo + ow) * ld_dy + c), g);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += g[j] * inv;
      }
    }
    st8(dst, pack8(acc));
  }
}

// ------------------------------------------------------------------------- glue kernels
__global__ void __launch_bounds__(kT)
relu_mask_kernel(unsigned short* __restrict__ g, int ld_g, const unsigned short* __restrict__ a, int ld_a,
                 long long M, int C) {
  const int C8 = C >> 3;
  const long long total = M * C8;
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < total; i += (long long)gridDim.x * kT) {
    const long long m = i / C8;
    const int c = (int)(i - m * C8) << 3;
    float gg[8], aa[8];
    unpack8(ld8(g + m * ld_g + c), gg);
    unpack8(ld8(a + m * ld_a + c), aa);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (!(aa[j] > 0.f)) gg[j] = 0.f;
    st8(g + m * ld_g + c, pack8(gg));
  }
}

__global__ void __launch_bounds__(kT)
pack_input_kernel(const float* __restrict__ img, long long pixels, unsigned short* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < pixels; i += (long long)gridDim.x * kT) {
    float f[8] = {img[3 * i], img[3 * i + 1], img[3 * i + 2], 0.f, 0.f, 0.f, 0.f, 0.f};
    st8(out + 8 * i, pack8(f));
  }
}

__global__ void __launch_bounds__(kT)
head_gather_kernel(const float* __restrict__ h, int ld_h, int N, int cells, int k, int P, int off,
                   float* __restrict__ locs, float* __restrict__ logits) {
  const int total = N * cells * k;
  for (int i = blockIdx.x * kT + threadIdx.x; i < total; i += gridDim.x * kT) {
    const int a = i % k, t = i / k, cell = t % cells, n = t / cells;
    const float* row = h + (size_t)(n * cells + cell) * ld_h;
    const size_t p = (size_t)n * P + off + cell * k + a;
    *reinterpret_cast<float4*>(locs + p * 4) = make_float4(row[a * 4], row[a * 4 + 1], row[a * 4 + 2], row[a * 4 + 3]);
    logits[p] = row[4 * k + a];
  }
}

__global__ void __launch_bounds__(kT)
head_scatter_kernel(const float* __restrict__ d_locs, const float* __restrict__ d_logits, int N, int cells, int k,
                    int P, int off, unsigned short* __restrict__ g, int ld_g) {
  const int total = N * cells * ld_g;
  for (int i = blockIdx.x * kT + threadIdx.x; i < total; i += gridDim.x * kT) {
    const int ch = i % ld_g, t = i / ld_g, cell = t % cells, n = t / cells;
    const size_t p = (size_t)n * P + off + cell * k;
    float v = 0.f;
    if (ch < 4 * k) v = d_locs[(p + ch / 4) * 4 + (ch & 3)];
    else if (ch < 5 * k) v = d_logits[p + (ch - 4 * k)];
    g[i] = (unsigned short)f2bf(v);
  }
}

// every detection head of the network in ONE launch (a kernel costs >= 4.4 us in the replayed step whatever it does: six
// gathers behind six tiny head convolutions were 26 us of launches for 160 KB of data)
constexpr int kMaxHeads = 8;
struct HeadTable {
  const float* h[kMaxHeads]; unsigned short* g[kMaxHeads];
  int ld_h[kMaxHeads], ld_g[kMaxHeads], cells[kMaxHeads], k[kMaxHeads], off[kMaxHeads];
  int start[kMaxHeads + 1];                  // prefix sums of the per-head element counts
  int n;
};

__global__ void __launch_bounds__(kT)
head_gather_all_kernel(const HeadTable t, int P, float* __restrict__ locs, float* __restrict__ logits) {
  const int total = t.start[t.n];
  for (int i = blockIdx.x * kT + threadIdx.x; i < total; i += gridDim.x * kT) {
    int j = 0;
    while (j + 1 < t.n && i >= t.start[j + 1]) ++j;
    const int e = i - t.start[j], k = t.k[j], cells = t.cells[j];
    const int a = e % k, q = e / k, cell = q % cells, n = q / cells;
    const float* row = t.h[j] + (size_t)(n * cells + cell) * t.ld_h[j];
    const size_t p = (size_t)n * P + t.off[j] + cell * k + a;
    *reinterpret_cast<float4*>(locs + p * 4) = make_float4(row[a * 4], row[a * 4 + 1], row[a * 4 + 2], row[a * 4 + 3]);
    logits[p] = row[4 * k + a];
  }
}

__global__ void __launch_bounds__(kT)
head_scatter_all_kernel(const HeadTable t, int P, const float* __restrict__ d_locs, const float* __restrict__ d_logits) {
  const int total = t.start[t.n];
  for (int i = blockIdx.x * kT + threadIdx.x; i < total; i += gridDim.x * kT) {
    int j = 0;
    while (j + 1 < t.n && i >= t.start[j + 1]) ++j;
    const int e = i - t.start[j], k = t.k[j], cells = t.cells[j], ld = t.ld_g[j];
    const int ch = e % ld, q = e / ld, cell = q % cells, n = q / cells;
    const size_t p = (size_t)n * P + t.off[j] + cell * k;
    float v = 0.f;
    if (ch < 4 * k) v = d_locs[(p + ch / 4) * 4 + (ch & 3)];
    else if (ch < 5 * k) v = d_logits[p + (ch - 4 * k)];
    t.g[j][e] = (unsigned short)f2bf(v);
  }
}

// start of a step's backward pass in ONE launch: the gradient buffer and the BN-backward workspace cleared (two fills),
// and the grid-barrier time-outs of the PREVIOUS step -- word `ctl` of the gradient buffer, which this launch clears --
// added to a running total first (was: five small torch kernels over the per-layer flags)
__global__ void __launch_bounds__(kT)
step_begin_kernel(float* __restrict__ G, long long nG, float* __restrict__ ws, long long nws, long long ctl,
                  unsigned long long* __restrict__ timeouts_total, float* __restrict__ scalar) {
  if (scalar && blockIdx.x == 0 && threadIdx.x == 0) *scalar = 0.f;      // (the regularisation-loss accumulator of the optimiser)
  const long long n4 = nG >> 2, w4 = nws >> 2;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n4 + w4; i += (long long)gridDim.x * kT) {
    if (i < n4) {
      if (timeouts_total && i == (ctl >> 2)) {         // this lane is the one that clears the control word: read it first
        const float t = G[ctl];
        if (t > 0.f) *timeouts_total += (unsigned long long)t;
      }
      reinterpret_cast<float4*>(G)[i] = z;
    } else {
      reinterpret_cast<float4*>(ws)[i - n4] = z;
    }
  }
}

// ---------------------------------------------------------------------- filter prepare
// dst[c][r'][s'][kq] = src[kq][R-1-r'][S-1-s'][c]: a [K] x [C] transpose per tap.  Each workgroup moves a
// 64(k) x 32(c) patch of one tap through LDS so that both the reads (contiguous in c) and the writes
// (contiguous in k) are coalesced (the first version gathered 2-byte elements: 3.5 GB of fetches for 120 MB).
__global__ void __launch_bounds__(kT)
filter_prepare_kernel(const unsigned short* __restrict__ w, unsigned short* __restrict__ wd,
                      const mbx_filter_entry* __restrict__ table, int n_entries) {
  __shared__ __attribute__((aligned(16))) unsigned short tile[64][40];     // 80-byte rows: 16-byte aligned chunks
  int lo = 0, hi = n_entries - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const mbx_filter_entry e = table[lo];
  const int kt = (e.Kpad + 63) / 64, ct = (e.C + 31) / 32;
  int b = blockIdx.x - e.first_block;
  const int ck = b % kt; b /= kt;
  const int cc = b % ct; b /= ct;
  const int s = b % e.S, r = b / e.S;                       // destination tap (r', s')
  const unsigned short* src = w + e.src_off;
  unsigned short* dst = wd + e.dst_off;
  const int k0 = ck * 64, c0 = cc * 32;
  const long long tap_src = ((long long)(e.R - 1 - r) * e.S + (e.S - 1 - s)) * e.C;
  if (((e.C | e.Kpad) & 7) == 0 && ((e.src_off | e.dst_off) & 7) == 0) {
    // 16 bytes per lane both ways: one load of 8 channels of one filter, one store of 8 filters of one channel
    static_assert(kT == 256, "one 16-byte chunk per thread");
    {
      const int kk = threadIdx.x >> 2, c = (threadIdx.x & 3) << 3;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (k0 + kk < e.K && c0 + c < e.C)
        v = *reinterpret_cast<const uint4*>(src + (long long)(k0 + kk) * e.R * e.S * e.C + tap_src + c0 + c);
      *reinterpret_cast<uint4*>(&tile[kk][c]) = v;
    }
    __syncthreads();
    {
      const int c = threadIdx.x >> 3, kk = (threadIdx.x & 7) << 3;
      if (k0 + kk < e.Kpad && c0 + c < e.C) {
        unsigned q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = (unsigned)tile[kk + 2 * j][c] | ((unsigned)tile[kk + 2 * j + 1][c] << 16);
        *reinterpret_cast<uint4*>(dst + (((long long)(c0 + c) * e.R + r) * e.S + s) * e.Kpad + k0 + kk) =
            make_uint4(q[0], q[1], q[2], q[3]);
      }
    }
    return;
  }
  for (int i = threadIdx.x; i < 64 * 32; i += kT) {         // read: c fastest
    const int kk = i >> 5, c = i & 31;
    unsigned short v = 0;
    if (k0 + kk < e.K && c0 + c < e.C) v = src[(long long)(k0 + kk) * e.R * e.S * e.C + tap_src + c0 + c];
    tile[kk][c] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * 32; i += kT) {         // write: k fastest
    const int c = i >> 6, kk = i & 63;
    if (k0 + kk < e.Kpad && c0 + c < e.C)
      dst[(((long long)(c0 + c) * e.R + r) * e.S + s) * e.Kpad + k0 + kk] = tile[kk][c];
  }
}

}  // namespace

// ================================================================================== C ABI
static int pool_args_ok(const void* x, int ldx, const void* y, int ldy, int N, int H, int W, int C, int k, int Ho, int Wo) {
  return x && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 && k > 0 && k < 16 &&
         Ho > 0 && Wo > 0 && al16(x) && al16(y) && (long long)N * H * W * (C / 8) < (1LL << 31) &&
         (long long)N * Ho * Wo * (C / 8) < (1LL << 31);
}

extern "C" int mbx_maxpool_fwd(const void* x, int64_t xs, int ldx, int N, int H, int W, int C, int k, int stride, void* y,
                               int64_t ys, int ldy, int Ho, int Wo, uint8_t* argmax, mbx_stream_t stream) {
  if (!pool_args_ok(x, ldx, y, ldy, N, H, W, C, k, Ho, Wo) || stride < 1) return MBX_ERR_INVALID_ARG;
  if ((Ho - 1) * stride + k > H || (Wo - 1) * stride + k > W) return MBX_ERR_INVALID_ARG;   // VALID only
  MBX_ENTER();
  if (k == 3 && stride == 2)
    hipLaunchKernelGGL((maxpool_fwd_kernel<3, 2>), dim3(grid_for((long long)N * Ho * Wo * (C / 8))), dim3(kT), 0, mbx_s(stream),
                       (cus)x, (long long)xs, ldx, N, H, W, C, k, stride, (us)y, (long long)ys, ldy, Ho, Wo, argmax);
  else
    hipLaunchKernelGGL((maxpool_fwd_kernel<0, 0>), dim3(grid_for((long long)N * Ho * Wo * (C / 8))), dim3(kT), 0, mbx_s(stream),
                       (cus)x, (long long)xs, ldx, N, H, W, C, k, stride, (us)y, (long long)ys, ldy, Ho, Wo, argmax);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_maxpool_bwd(const void* dy, int64_t dys, int ld_dy, const uint8_t* argmax, int N, int H, int W, int C,
                               int k, int stride, int Ho, int Wo, void* dx, int64_t dxs, int ld_dx, int accumulate,
                               mbx_stream_t stream) {
  if (!pool_args_ok(dy, ld_dy, dx, ld_dx, N, H, W, C, k, Ho, Wo) || !argmax || stride < 1) return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  if (k == 3 && stride == 2)
    hipLaunchKernelGGL((maxpool_bwd_kernel<3, 2>), dim3(grid_for((long long)N * H * W * (C / 8))), dim3(kT), 0, mbx_s(stream),
                       (cus)dy, (long long)dys, ld_dy, argmax, N, H, W, C, k, stride, Ho, Wo, (us)dx, (long long)dxs, ld_dx,
                       accumulate);
  else
    hipLaunchKernelGGL((maxpool_bwd_kernel<0, 0>), dim3(grid_for((long long)N * H * W * (C / 8))), dim3(kT), 0, mbx_s(stream),
                       (cus)dy, (long long)dys, ld_dy, argmax, N, H, W, C, k, stride, Ho, Wo, (us)dx, (long long)dxs, ld_dx,
                       accumulate);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_avgpool_fwd(const void* x, int64_t xs, int ldx, int N, int H, int W, int C, int k, int pad, void* y,
                               int64_t ys, int ldy, int Ho, int Wo, mbx_stream_t stream) {
  if (!pool_args_ok(x, ldx, y, ldy, N, H, W, C, k, Ho, Wo) || pad < 0 || pad >= k) return MBX_ERR_INVALID_ARG;
  if (Ho != H + 2 * pad - k + 1 || Wo != W + 2 * pad - k + 1) return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(grid_for((long long)N * Ho * Wo * (C / 8))), dim3(kT), 0, mbx_s(stream),
                     (cus)x, (long long)xs, ldx, N, H, W, C, k, pad, (us)y, (long long)ys, ldy, Ho, Wo);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_avgpool_bwd(const void* dy, int64_t dys, int ld_dy, int N, int H, int W, int C, int k, int pad, int Ho,
                               int Wo, void* dx, int64_t dxs, int ld_dx, int accumulate, mbx_stream_t stream) {
  if (!pool_args_ok(dy, ld_dy, dx, ld_dx, N, H, W, C, k, Ho, Wo) || pad < 0 || pad >= k) return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(grid_for((long long)N * H * W * (C / 8))), dim3(kT), 0, mbx_s(stream),
                     (cus)dy, (long long)dys, ld_dy, N, H, W, C, k, pad, Ho, Wo, (us)dx, (long long)dxs, ld_dx, accumulate);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_relu_mask(void* g, int ld_g, const void* a, int ld_a, int64_t M, int C, mbx_stream_t stream) {
  if (!g || !a || M <= 0 || C <= 0 || C % 8 || ld_g % 8 || ld_a % 8 || !al16(g) || !al16(a)) return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  hipLaunchKernelGGL(relu_mask_kernel, dim3(grid_for(M * (C / 8))), dim3(kT), 0, mbx_s(stream), (us)g, ld_g, (cus)a, ld_a,
                     (long long)M, C);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_pack_input(const float* img, int64_t pixels, void* out, mbx_stream_t stream) {
  if (!img || !out || pixels <= 0 || !al16(out)) return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  hipLaunchKernelGGL(pack_input_kernel, dim3(grid_for(pixels)), dim3(kT), 0, mbx_s(stream), img, (long long)pixels, (us)out);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_head_gather(const float* h, int ld_h, int N, int cells, int k, int P, int off, float* locs,
                               float* logits, mbx_stream_t stream) {
  if (!h || !locs || !logits || N <= 0 || cells <= 0 || k <= 0 || ld_h < 5 * k || off < 0 || off + cells * k > P)
    return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  hipLaunchKernelGGL(head_gather_kernel, dim3(grid_for((long long)N * cells * k)), dim3(kT), 0, mbx_s(stream), h, ld_h, N,
                     cells, k, P, off, locs, logits);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_head_scatter(const float* d_locs, const float* d_logits, int N, int cells, int k, int P, int off, void* g,
                                int ld_g, mbx_stream_t stream) {
  if (!d_locs || !d_logits || !g || N <= 0 || cells <= 0 || k <= 0 || ld_g < 5 * k || off < 0 || off + cells * k > P)
    return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  hipLaunchKernelGGL(head_scatter_kernel, dim3(grid_for((long long)N * cells * ld_g)), dim3(kT), 0, mbx_s(stream), d_locs,
                     d_logits, N, cells, k, P, off, (us)g, ld_g);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

static int fill_head_table(const mbx_head* heads, int n_heads, int N, int P, bool scatter, HeadTable& t) {
  if (!heads || n_heads <= 0 || n_heads > kMaxHeads || N <= 0 || P <= 0) return MBX_ERR_INVALID_ARG;
  long long acc = 0;
  t.n = n_heads;
  for (int j = 0; j < n_heads; ++j) {
    const mbx_head& H = heads[j];
    if (H.cells <= 0 || H.k <= 0 || H.off < 0 || H.off + H.cells * H.k > P) return MBX_ERR_INVALID_ARG;
    if (scatter ? (!H.g || H.ld_g < 5 * H.k) : (!H.h || H.ld_h < 5 * H.k)) return MBX_ERR_INVALID_ARG;
    t.h[j] = H.h; t.g[j] = reinterpret_cast<unsigned short*>(H.g);
    t.ld_h[j] = H.ld_h; t.ld_g[j] = H.ld_g; t.cells[j] = H.cells; t.k[j] = H.k; t.off[j] = H.off;
    t.start[j] = (int)acc;
    acc += (long long)N * H.cells * (scatter ? H.ld_g : H.k);
    if (acc >= (1LL << 31)) return MBX_ERR_UNSUPPORTED;
  }
  for (int j = n_heads; j <= kMaxHeads; ++j) t.start[j] = (int)acc;
  return MBX_OK;
}

extern "C" int mbx_head_gather_all(const mbx_head* heads, int n_heads, int N, int P, float* locs, float* logits,
                                   mbx_stream_t stream) {
  if (!locs || !logits) return MBX_ERR_INVALID_ARG;
  HeadTable t;
  const int st = fill_head_table(heads, n_heads, N, P, false, t);
  if (st != MBX_OK) return st;
  MBX_ENTER();
  hipLaunchKernelGGL(head_gather_all_kernel, dim3(grid_for(t.start[t.n])), dim3(kT), 0, mbx_s(stream), t, P, locs, logits);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_head_scatter_all(const float* d_locs, const float* d_logits, const mbx_head* heads, int n_heads, int N,
                                    int P, mbx_stream_t stream) {
  if (!d_locs || !d_logits) return MBX_ERR_INVALID_ARG;
  HeadTable t;
  const int st = fill_head_table(heads, n_heads, N, P, true, t);
  if (st != MBX_OK) return st;
  MBX_ENTER();
  hipLaunchKernelGGL(head_scatter_all_kernel, dim3(grid_for(t.start[t.n])), dim3(kT), 0, mbx_s(stream), t, P, d_locs, d_logits);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_step_begin(float* grads, int64_t n_grads, float* bn_ws, int64_t n_ws, int64_t ctl_index,
                              uint64_t* timeouts_total, float* zero_scalar, mbx_stream_t stream) {
  if (!grads || n_grads <= 0 || n_grads % 4 || n_ws < 0 || n_ws % 4 || (n_ws && !bn_ws) || !al16(grads) || (bn_ws && !al16(bn_ws)) ||
      (timeouts_total && (ctl_index < 0 || ctl_index >= n_grads)))
    return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  hipLaunchKernelGGL(step_begin_kernel, dim3(grid_for((n_grads + n_ws) / 4)), dim3(kT), 0, mbx_s(stream), grads,
                     (long long)n_grads, bn_ws, (long long)n_ws, (long long)ctl_index,
                     reinterpret_cast<unsigned long long*>(timeouts_total), zero_scalar);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}

extern "C" int mbx_filter_prepare(const void* w_bf16, void* w_dgrad, const mbx_filter_entry* table, int n_entries,
                                  int total_blocks, mbx_stream_t stream) {
  if (!w_bf16 || !w_dgrad || !table || n_entries <= 0 || total_blocks <= 0) return MBX_ERR_INVALID_ARG;
  MBX_ENTER();
  hipLaunchKernelGGL(filter_prepare_kernel, dim3(total_blocks), dim3(kT), 0, mbx_s(stream), (cus)w_bf16, (us)w_dgrad, table,
                     n_entries);
  MBX_LAUNCH_CHECK();
  return MBX_OK;
}
