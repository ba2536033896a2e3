// What bn.hip and nnops.hip share: 16-byte (8 x bf16) vector access along the NHWC channel axis, the bf16 conversions, the
// channel map of a batch-norm group, launch-grid sizing and the XCD row order.  (The convolution files keep their own
// conversions in conv_common.h: other instruction-level choices.)
#pragma once
#include "common.h"

namespace {

// Workgroups are dealt to the eight XCDs round-robin (b and b + 8 share one): logical id = a contiguous run per XCD, the mapping
// of the convolution kernels' tiles (conv_common.h xcd_remap).  A row-wise kernel that walks its rows by LOGICAL id reads what
// the producing convolution's tiles left in THIS XCD's L2 and leaves its output where the consuming convolution's tiles will
// look for it: an XCD's L2 keeps what a kernel wrote across the kernel boundary (tools/l2_persist.hip: 32 MB read back by the
// XCD that wrote it 6.2 us, by another 8.2 us).  MEASURED LEVEL on the training step (tools/xcd_rows_ab.sh: 14.64-14.66 vs
// 14.61-14.65 ms; the 512 x 512 leg 37.70 vs 37.85): the convolutions' K loops are not paced by where their operands come
// from (LAB_NOTES round 2: loaders that do not wait for their data run the same 0.43 us per step).  Off; MBX_XCD_ROWS=1.
__device__ __forceinline__ int xcd_logical(int bid, int nblk) {
  const int xcd = bid & 7, q = nblk >> 3, r = nblk & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}
inline int xcd_rows_on() { static const int v = mbx_env_int("MBX_XCD_ROWS", 0); return v; }

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
constexpr int kT = 256;

__device__ __forceinline__ float bf2f(unsigned h) { return __uint_as_float(h << 16); }
__device__ __forceinline__ unsigned f2bf(float f) { return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)f); }
// two floats to a packed bf16 pair in one v_cvt_pk_bf16_f32 (f2bf's rounding; the compiler emits one conversion per value
// plus a shift and an or), and max(x, 0) in one v_max_f32 (fmaxf canonicalises its operand first)
__device__ __forceinline__ unsigned pack2bf(float lo, float hi) {
  typedef float pk_f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 pk_bf16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_convertvector(pk_f32x2{lo, hi}, pk_bf16x2));
}
__device__ __forceinline__ float relu_f(float x) {
  float r;
  asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(x));
  return r;
}
__device__ __forceinline__ void unpack8(const u32x4 v, float* f) {
  f[0] = bf2f(v.x & 0xffffu); f[1] = bf2f(v.x >> 16); f[2] = bf2f(v.y & 0xffffu); f[3] = bf2f(v.y >> 16);
  f[4] = bf2f(v.z & 0xffffu); f[5] = bf2f(v.z >> 16); f[6] = bf2f(v.w & 0xffffu); f[7] = bf2f(v.w >> 16);
}
__device__ __forceinline__ u32x4 pack8(const float* f) {
  u32x4 v;
  v.x = pack2bf(f[0], f[1]); v.y = pack2bf(f[2], f[3]); v.z = pack2bf(f[4], f[5]); v.w = pack2bf(f[6], f[7]);
  return v;
}
__device__ __forceinline__ u32x4 ld8(const unsigned short* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ void st8(unsigned short* p, const u32x4 v) { *reinterpret_cast<u32x4*>(p) = v; }

// Channel map of a batch-norm GROUP (several sibling convolutions normalised by one set of launches): channel c of the
// group's contiguous [M, C] tensors (y, dy) lives at channel c + off[i] of the strided activation / gradient view, where
// i is the last entry with cb[i] <= c (n = 0: the identity).  Lane-constant wherever a lane owns a channel group.
struct ChanMap { int n; int cb[4]; int off[4]; };
__device__ __forceinline__ int chan_off(const ChanMap& m, int c) {
  int o = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) if (i < m.n && c >= m.cb[i]) o = m.off[i];
  return o;
}
inline int chan_map_max(const ChanMap& m) { int o = 0; for (int i = 0; i < m.n; ++i) if (m.off[i] > o) o = m.off[i]; return o; }

inline int grid_for(long long work_items) {
  long long b = (work_items + kT - 1) / kT;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
typedef const unsigned short* cus;
typedef unsigned short* us;

}  // namespace
