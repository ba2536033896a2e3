// The store epilogue of the kernels that multiply out of LDS with the filter rows as the A operand in the PERMUTED order:
// conv_direct3_kernel, conv_stem_kernel (convd.hip) and conv_resident_kernel (convr.hip).  (conv_directw_kernel takes the
// permutation from here and keeps its own text of the epilogue: convd.hip.)
#pragma once
#include "conv_common.h"

namespace {

// Filter rows are fed to the MFMA in a PERMUTED order (as in conv_igemm3_kernel): LDS row 16 a + f of a tap holds output
// channel dperm<CO>(a, f) (of the tile's CO = 16 NA channels), so that blocks 2A and 2A + 1 leave a lane EIGHT consecutive
// channels of one pixel = one 16-byte store (four lanes cover 64 contiguous bytes; with the plain order a 128-byte pixel row
// went out as four 32-byte pieces and the 32 -> 64 layer ran at 2.4x its HBM time).  A trailing unpaired block (C_out 48:
// channels 32..47) keeps the plain order.
template <int CO>
__device__ __forceinline__ int dperm(int a, int f) {
  return (a < (CO / 32) * 2) ? 32 * (a >> 1) + 8 * (f >> 2) + 4 * (a & 1) + (f & 3) : 16 * a + f;
}

// EV = 3 (folded batch norm of the inference / --fine_tune forward, detect.py:313-326): y = act(acc * scale[c] + shift[c]), the
// expression of the implicit-GEMM kernels' affine epilogue.  The lane's channels of a tile that starts at channel cb and ends
// before ce: eight per paired block (cb + 32 A + 8 fch ..), four of an unpaired last block (cb + 16 (NA - 1) + 4 fch ..).
template <int NA>
struct DirAffine {
  static constexpr int NP = NA / 2;                       // paired blocks
  float sc8[NP > 0 ? NP : 1][8], sh8[NP > 0 ? NP : 1][8], sc4[4], sh4[4];
};
template <int EV, int NA>
__device__ __forceinline__ void direct_affine_load(const ConvK& p, const int cb, const int ce, const int fch, DirAffine<NA>& af) {
  constexpr int NP = NA / 2;
  if constexpr (EV == 3) {
#pragma unroll
    for (int A = 0; A < NP; ++A)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = cb + 32 * A + 8 * fch + j;
        af.sc8[A][j] = (p.scale && c < ce) ? p.scale[c] : 1.f;
        af.sh8[A][j] = (p.shiftv && c < ce) ? p.shiftv[c] : 0.f;
      }
    if constexpr (NA > 2 * NP) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = cb + 32 * NP + 4 * fch + j;
        af.sc4[j] = (p.scale && c < ce) ? p.scale[c] : 1.f;
        af.sh4[j] = (p.shiftv && c < ce) ? p.shiftv[c] : 0.f;
      }
    }
  }
}

// One pixel block of a tile: acc[a][b][r] holds channel cb + dperm(a, 4 fch + r) of the lane's pixel (valid: pv; its channel 0
// is element pix_off of y); the tile's channels end before ce.  Blocks 2A, 2A + 1 -> 8 consecutive channels: 16-byte stores; an unpaired last
// block: 4 consecutive channels, 8-byte stores.  EV = 3: affine (+ ReLU; relu_f reads the affine's VALU result, never an
// accumulator); EV = 1: s1 / s2 += the STORED, bf16-rounded values and their squares.
template <int EV, int NA, int MI>
__device__ __forceinline__ void direct_store_pixel(const ConvK& p, const __amdgpu_buffer_rsrc_t yr, const f32x4 (&acc)[NA][MI], const int b,
                                                   const bool pv, const int pix_off, const int cb, const int ce, const int fch,
                                                   const DirAffine<NA>& af, float (&s1)[NA][4], float (&s2)[NA][4]) {
  constexpr int NP = NA / 2;
#pragma unroll
  for (int A = 0; A < NP; ++A) {
    const int c0 = cb + 32 * A + 8 * fch;
    const bool ok = pv && c0 < ce;                        // channel counts are multiples of 8: a group of eight is all in or all out
    float v8[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) { v8[r] = acc[2 * A][b][r]; v8[4 + r] = acc[2 * A + 1][b][r]; }
    if constexpr (EV == 3) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v8[j] = v8[j] * af.sc8[A][j] + af.sh8[A][j];
      if (p.relu) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v8[j] = relu_f(v8[j]);
      }
    }
    unsigned h2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) h2[j] = pack2bf(v8[2 * j], v8[2 * j + 1]);
    __builtin_amdgcn_raw_buffer_store_b128(u32x4{h2[0], h2[1], h2[2], h2[3]}, yr, ok ? (int)((pix_off + c0) * 2) : (int)kOOB, 0, 0);
    if constexpr (EV == 1) {
      if (ok) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const unsigned w0 = h2[r >> 1], w1 = h2[2 + (r >> 1)];
          const float f0 = (r & 1) ? bf_hi(w0) : bf_lo(w0), f1 = (r & 1) ? bf_hi(w1) : bf_lo(w1);
          s1[2 * A][r] += f0; s2[2 * A][r] += f0 * f0;
          s1[2 * A + 1][r] += f1; s2[2 * A + 1][r] += f1 * f1;
        }
      }
    }
  }
  if constexpr (NA > 2 * NP) {
    constexpr int a = 2 * NP;
    const int c0 = cb + 16 * a + 4 * fch;
    const bool ok = pv && c0 < ce;
    float v4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[a][b][r];
      if constexpr (EV == 3) { v = v * af.sc4[r] + af.sh4[r]; if (p.relu) v = relu_f(v); }
      v4[r] = v;
    }
    const unsigned g2[2] = {pack2bf(v4[0], v4[1]), pack2bf(v4[2], v4[3])};
    __builtin_amdgcn_raw_buffer_store_b64(u32x2{g2[0], g2[1]}, yr, ok ? (int)((pix_off + c0) * 2) : (int)kOOB, 0, 0);
    if constexpr (EV == 1) {
      if (ok) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float fv = (r & 1) ? bf_hi(g2[r >> 1]) : bf_lo(g2[r >> 1]);
          s1[a][r] += fv; s2[a][r] += fv * fv;
        }
      }
    }
  }
}

}  // namespace
