// qs_devfn.h -- small device functions shared by the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qs_device.h"

// float -> int32 the way x86-64 cvttss2si does it (the reference's
// `int range = roundf(a2)`): NaN / out of range => INT_MIN.
__device__ __forceinline__ int f2i_x86(float v) {
  return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000;
}

// C99 roundf: nearest, ties away from zero (exact: x - trunc(x) is exact).
__device__ __forceinline__ float round_half_away(float x) {
  float t = __builtin_truncf(x);
  float fr = __builtin_fabsf(x - t);
  return fr >= 0.5f ? t + __builtin_copysignf(1.0f, x) : t;
}

// nearest multiple of the quantiser (ties away from zero) via the reference's
// reciprocal tables, and the interval that quantises to it.
// reference quantsmooth.h:332-336, 1552-1557.
__device__ __forceinline__ void interval(int c, int div, int x1, int sh, int& orig, int& lo, int& hi) {
  int a = ((x1 * c) >> 16) + c;
  a = (int)(((uint32_t)a << sh) + 0x4000u) >> 15;   // == (-a * x2 + 0x4000) >> 15 with x2 = -(1 << sh), see QsConsts::x2
  a *= div;
  const int d0 = (div - 1) >> 1, d1 = div >> 1;
  orig = a;
  hi = a + (a < 0 ? d1 : d0);
  lo = a - (a > 0 ? d1 : d0);
}


// Dequantisation of one 16-byte group of a block's coefficients (reference quantsmooth.h:2597-2603): the eight int16 of
// eighth e of a block (natural indices 8e .. 8e + 7) times the file's quantiser q[0..7] = qraw[8e ..], each product
// stored as JCOEF (int16 wrap).  CHECK: `bad` collects products outside [-2048, 2047] (the reference's range check).
// Used where a wave moves coefficients as contiguous 16 B per lane: e = lane & 7 (pass A and the recovery kernels'
// stage-in of a plane whose coefficients are still quantised, QS_PLANE_QUANT).
__device__ __forceinline__ void qs_load_qraw8(const QsConsts* __restrict__ cst, int e, int (&q)[8]) {
  const int4* qp = reinterpret_cast<const int4*>(cst->qraw) + e * 2;
  const int4 a = qp[0], b = qp[1];
  q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = b.x; q[5] = b.y; q[6] = b.z; q[7] = b.w;
}
template <bool CHECK>
__device__ __forceinline__ uint4 qs_dequant8(uint4 v, const int (&q)[8], int& bad) {
  uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int lo = (int32_t)(int16_t)(d[c] & 0xffff) * q[c * 2];
    const int hi = ((int32_t)d[c] >> 16) * q[c * 2 + 1];
    if (CHECK) bad |= ((unsigned)(lo + 0x800) > 0xfffu) | ((unsigned)(hi + 0x800) > 0xfffu);
    d[c] = ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
  }
  return make_uint4(d[0], d[1], d[2], d[3]);
}

// index of the plane that owns 64-block group `w` of a plane-set launch
// (binary search over the prefix array; everything here is wave-uniform)
__device__ __forceinline__ int qs_set_find(const QsPlaneSet& set, int w) {
  int lo = 0, hi = set.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (set.wave0[mid] <= w) lo = mid; else hi = mid - 1;
  }
  return lo;
}
