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

// One coefficient of the rebalance step (reference quantsmooth.h:1836-1846): clamp((c * mul + 0x1000) >> 13, lo, hi)
// with [lo, hi] the interval of c -- for the lanes of a wave that holds no coefficient outside [-0x2000, 0x2000) when
// it is staged and whose mul lies in [8192, QS_REB_MUL_MAX].  There only the OUTWARD bound can bind:
//   * Every |c| stays below 0x4000 (a value moves inside intervals around |c| < 0x2000, quantiser < 0x800), where the
//     reciprocal tables divide exactly: orig = a * div is the multiple of div nearest to c, so c and orig never
//     differ in sign and lo <= c <= hi.
//   * |c| < 2^15 and mul < 2^15 keep c * mul + 0x1000 inside int32: the 24-bit product IS the reference's wrapping
//     32-bit one, and no wrap happens.  (mul itself is not bounded by the arithmetic alone -- the caller checks it.)
//   * c > 0: c * mul >= c << 13, so v = (c * mul + 0x1000) >> 13 >= c >= lo, and orig >= 0 makes hi = orig + d0.
//     c < 0: c * mul <= c << 13, so v <= (c * 8192 + 4096) >> 13 = c <= hi, and orig <= 0 makes lo = orig - d0.
//     c = 0: v = 0, orig = 0, and 0 lies between -d0 and d0.
//   With b = orig + d0 (c >= 0) or orig - d0 (c < 0) the result is min(v, b) for c > 0 and max(v, b) for c < 0: in both
//   cases c is the extreme of {v, b, c} on the side that cannot bind, and the answer is their median (c = 0: 0).
// tests/test_rebalance_lemma.py checks this against interval() over every c, quantiser and a spread of mul.
#define QS_REB_MUL_MAX 0x7fff
__device__ __forceinline__ int qs_rebalance_outward(int c, int mul, int div, int x1, int sh) {
  // interval()'s a = ((x << sh) + 0x4000) >> 15 with x = ((x1 * c) >> 16) + c, as (x + (0x4000 >> sh)) >> (15 - sh): the
  // same floor of the same quotient, since 0 <= sh <= 15 (the quantiser is at least 1), 0x4000 >> sh is exact for
  // sh <= 14 and for sh = 15 both forms give x.  Rounding constant and shift are scalars of the coefficient.
  const int rnd = 0x4000 >> sh, shr = 15 - sh;
  const int a = ((__mul24(x1, c) >> 16) + c + rnd) >> shr;   // x1 and c are int16 values: 24-bit operands, no wrap
  // +-d0 by the sign of c without a select: (d0 + t) ^ t with t = c >> 31 (t = -1: ~(d0 - 1) = -d0)
  const int d0 = (div - 1) >> 1, t = c >> 31;
  const int b = __mul24(a, div) + ((d0 + t) ^ t);            // |a| <= |c|, div < 2^11
  const int v = (__mul24(c, mul) + 0x1000) >> 13;
  int r;
  asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(v), "v"(b), "v"(c));
  return r;
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
