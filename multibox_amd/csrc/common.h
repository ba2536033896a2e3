// Shared helpers for libmbx (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mbx.h"

#include <stdio.h>
#include <stdlib.h>
// Launch checking: MBX_ENTER() drops any stale error another library left in the runtime's
// per-thread slot; MBX_LAUNCH_CHECK() then sees only this launch's own error.
#define MBX_ENTER() (void)hipGetLastError()
#define MBX_LAUNCH_CHECK()                                                              \
  do {                                                                                  \
    hipError_t mbx_e_ = hipGetLastError();                                              \
    if (mbx_e_ != hipSuccess) {                                                         \
      fprintf(stderr, "[libmbx] %s:%d launch failed: %s\n", __FILE__, __LINE__,         \
              hipGetErrorString(mbx_e_));                                               \
      return MBX_ERR_LAUNCH;                                                            \
    }                                                                                   \
  } while (0)

static inline hipStream_t mbx_s(mbx_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Compute units of the current device, or 0 when the query fails (no device visible).  A success is cached for the life of
// the process, a failure is not.  The convolution launchers size their persistent grids by `n ? n : 256` (MI355X); the
// one-launch BN backward, whose grid barrier needs every workgroup resident, refuses instead.
inline int mbx_cu_count() {
  static int ncu = 0;
  if (!ncu) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      ncu = n;
  }
  return ncu;
}

// Environment switches (MBX_*): the integer value, or dflt when unset; the first character, or 0 when unset.  The callers
// decide whether to read once (`static const`) or per call.
inline int mbx_env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline char mbx_env_char(const char* name) { const char* e = getenv(name); return e ? e[0] : '\0'; }
// MBX_DEBUG_BARRIER_FAULT (tests only), read once: '1' the one-launch BN backward's grid barrier, '2' the fused FORWARD
// barriers, '3' the fused BACKWARD barriers -- workgroup 0 never arrives and everyone else times out.
inline char mbx_barrier_fault() { static const char c = mbx_env_char("MBX_DEBUG_BARRIER_FAULT"); return c; }

__device__ __forceinline__ int mbx_lane() { return threadIdx.x & 63; }

// 64-lane butterfly reductions (wave = 64 on gfx950): every lane ends up with the result.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
