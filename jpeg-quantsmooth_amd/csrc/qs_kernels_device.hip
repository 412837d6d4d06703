// qs_kernels_device.hip -- the two kernels of the device-resident job route (csrc/qs_device_job.cpp):
//
//   qs_dev_precheck_kernel  before any pass: copies the coefficients of the components that may have to be rebuilt
//                           into a snapshot in the workspace, and evaluates the reference's range check
//                           (quantsmooth.h:2596-2602: val |= coef * quantval + 0x800; stop when val >> 12) on the
//                           components whose first pass A would run it.  The first component that fails, j, lands in
//                           one device word as n - j (atomicMax, one atomic per wave that saw a failure); 0 = none,
//                           so the word is reset with a ZERO memset (a captured hipMemsetAsync of 0xff bytes was seen
//                           to write 0 on the second and later replays of a graph on MI355X / ROCm 7).
//   qs_dev_fixup_kernel     after the last pass: reads that word once; nothing tripped (the normal case) -> every wave
//                           exits at once.  Otherwise it rebuilds what the reference leaves behind when it stops at
//                           component k (quantsmooth.h:2610, 2543-2566, 2668-2689) from the snapshot, per component
//                           by a table the host computed for every possible k.  Writes the job's `stop` word.
//
// Both stream 16 bytes per lane (8 coefficients, one eighth of a block), grid-stride.  The passes themselves run
// unconditionally between the two; the existing kernels are not touched (they tolerate tripped inputs: the eager
// host route runs them on such data before it re-runs the job).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qs_device_job.h"

// reference quantsmooth.h:2596-2602 over the 8 coefficients of one 16-byte vector: the OR of (coef * q + 0x800)
__device__ __forceinline__ int32_t qs_dev_range_bits(const uint4 v, const int32_t (&q)[8]) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
  int32_t acc = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int32_t lo = (int16_t)(d[c] & 0xffff), hi = (int32_t)d[c] >> 16;
    acc |= (lo * q[c * 2] + 0x800) | (hi * q[c * 2 + 1] + 0x800);
  }
  return acc;
}

// int16(coef * quantval) (reference :2563 / :2598, JCOEF arithmetic), then optionally the +-1023 clamp of :2668-2689
__device__ __forceinline__ uint4 qs_dev_dequant(const uint4 v, const int32_t (&q)[8], bool clamp) {
  uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    int32_t lo = (int16_t)(int32_t)((int16_t)(d[c] & 0xffff) * q[c * 2]);
    int32_t hi = (int16_t)(int32_t)(((int32_t)d[c] >> 16) * q[c * 2 + 1]);
    if (clamp) { lo = min(max(lo, -1023), 1023); hi = min(max(hi, -1023), 1023); }
    d[c] = ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
  }
  return make_uint4(d[0], d[1], d[2], d[3]);
}

// the 8 quantisers this lane's vectors are multiplied with: the grid stride is a multiple of 8 vectors, so a lane always
// handles the same eighth of a block
__device__ __forceinline__ void qs_dev_lane_quant(const QsDevComp& C, int32_t (&q)[8]) {
  const int e = (int)(threadIdx.x & 7);
#pragma unroll
  for (int k = 0; k < 8; ++k) q[k] = C.q[e * 8 + k];
}

__global__ void __launch_bounds__(256)
qs_dev_precheck_kernel(const QsDevJobArgs a, uint32_t* __restrict__ first_bad) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (int j = 0; j < a.n; ++j) {
    const QsDevComp& C = a.c[j];
    if (!C.snap && !C.check) continue;                       // (wave-uniform)
    int32_t q[8];
    qs_dev_lane_quant(C, q);
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(C.coef);
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(C.snap);
    int32_t acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < C.nvec; i += stride) {
      const uint4 v = src[i];
      if (dst) dst[i] = v;
      if (C.check) acc |= qs_dev_range_bits(v, q);
    }
    if (C.check && __any((acc >> 12) != 0) && (threadIdx.x & 63) == 0)
      atomicMax(first_bad, (uint32_t)(a.n - j));
  }
}

__global__ void __launch_bounds__(256)
qs_dev_fixup_kernel(const QsDevJobArgs a, const uint32_t* __restrict__ first_bad, int32_t* __restrict__ d_stop) {
  const uint32_t w = *first_bad;                             // one scalar load per wave: n - k, or 0
  const bool tripped = w != 0;
  const uint32_t k = tripped ? (uint32_t)a.n - w : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) *d_stop = (tripped || a.static_stop) ? 1 : 0;
  if (!tripped) return;
  const size_t stride = (size_t)gridDim.x * 256;
  for (int j = 0; j < a.n; ++j) {
    const QsDevComp& C = a.c[j];
    const int act = C.act[k];
    if (act == QS_DEV_KEEP) continue;                        // (wave-uniform)
    int32_t q[8];
    qs_dev_lane_quant(C, q);
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(C.snap);
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(C.coef);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < C.nvec; i += stride) {
      const uint4 v = src[i];
      dst[i] = act == QS_DEV_RESTORE ? v : qs_dev_dequant(v, q, act == QS_DEV_DEQUANT_CLAMP);
    }
  }
}

static int qs_dev_grid(size_t nvec, int cap) {
  const size_t g = (nvec + 255) / 256;
  return (int)(g < 1 ? 1 : g > (size_t)cap ? (size_t)cap : g);
}

void qs_launch_dev_precheck(const QsDevJobArgs& a, uint32_t* first_bad, hipStream_t s) {
  size_t nvec = 0;
  for (int j = 0; j < a.n; ++j) if (a.c[j].snap || a.c[j].check) nvec = a.c[j].nvec > nvec ? a.c[j].nvec : nvec;
  if (!nvec) return;
  hipLaunchKernelGGL(qs_dev_precheck_kernel, dim3(qs_dev_grid(nvec, 8192)), dim3(256), 0, s, a, first_bad);
}

void qs_launch_dev_fixup(const QsDevJobArgs& a, const uint32_t* first_bad, int32_t* d_stop, hipStream_t s) {
  size_t nvec = 0;
  for (int j = 0; j < a.n; ++j) nvec = a.c[j].nvec > nvec ? a.c[j].nvec : nvec;
  hipLaunchKernelGGL(qs_dev_fixup_kernel, dim3(qs_dev_grid(nvec, 1024)), dim3(256), 0, s, a, first_bad, d_stop);
}
