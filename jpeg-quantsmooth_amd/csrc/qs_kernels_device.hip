// qs_kernels_device.hip -- the kernels of the device-resident job route (csrc/qs_device_job.cpp), over the components
// of one or many jobs, one chunk (QS_DEVB_CHUNK components) per launch:
//
//   qs_dev_clear_words_kernel     zeroes the jobs' range-check words before the precheck.
//   qs_dev_precheck_batch_kernel  before any pass: copies the coefficients of the components that may have to be
//                                 rebuilt into a snapshot in the workspace, and evaluates the reference's range check
//                                 (quantsmooth.h:2596-2602: val |= coef * quantval + 0x800; stop when val >> 12) on the
//                                 components whose first pass A would run it.  The first component of a job that
//                                 fails, j, lands in the job's word as n - j (atomicMax, one atomic per wave that saw a
//                                 failure); 0 = none.
//   qs_dev_fixup_batch_kernel     after the last pass: reads the job's word; nothing tripped (the normal case) -> the
//                                 workgroup exits at once.  Otherwise it rebuilds what the reference leaves behind when
//                                 it stops at component k (quantsmooth.h:2610, 2543-2566, 2668-2689) from the snapshot,
//                                 per component by a row the host computed for every possible k.  Writes every job's
//                                 `stop`.
//
// The grid is flat over every 16-byte vector of the chunk: record c owns workgroups [blk0[c], blk0[c + 1]), so a small
// component does not wait behind a large one.  The passes themselves run unconditionally between precheck and fix-up;
// the existing kernels are not touched (they tolerate tripped inputs: the eager host route runs them on such data
// before it re-runs the job).
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

// the record that owns this workgroup: the last c with rec[c].blk0 <= blockIdx.x (wave-uniform)
__device__ __forceinline__ int qs_devb_find(const QsDevBatchArgs& a) {
  const uint32_t b = blockIdx.x;
  int lo = 0, hi = a.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.rec[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the snapshot of a record, or null when it has none or it would not lie inside the workspace
__device__ __forceinline__ uint4* qs_devb_snap(const QsDevBatchArgs& a, const QsDevBRec& R, uint64_t nvec) {
  const uint64_t off = R.snap_off;
  if (off == QS_DEVB_NO_SNAP || (off & 15) || off > a.ws_bytes || nvec > (a.ws_bytes - off) / 16) return nullptr;
  return reinterpret_cast<uint4*>(a.ws + off);
}

__device__ __forceinline__ void qs_devb_lane_quant(const QsDevBRec& R, int32_t (&q)[8]) {
  const int e = (int)(threadIdx.x & 7);                      // (a workgroup starts on a block boundary)
#pragma unroll
  for (int k = 0; k < 8; ++k) q[k] = R.q[e * 8 + k];
}

__global__ void __launch_bounds__(256)
qs_dev_precheck_batch_kernel(const QsDevBatchArgs a) {
  const int c = qs_devb_find(a);
  const QsDevBRec& R = a.rec[c];
  if (blockIdx.x < R.blk0 || R.job < 0 || R.job >= a.njobs) return;
  const uint64_t nvec = a.nvec[c];
  const uint64_t v0 = (uint64_t)(blockIdx.x - R.blk0) * QS_DEVB_PRE_VPB;
  if (v0 >= nvec) return;
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(a.coef[c]);
  uint4* __restrict__ dst = qs_devb_snap(a, R, nvec);
  const bool check = R.check != 0;
  int32_t q[8];
  qs_devb_lane_quant(R, q);
  int32_t acc = 0;
#pragma unroll 4
  for (int r = 0; r < QS_DEVB_PRE_VPB / 256; ++r) {
    const uint64_t i = v0 + (uint64_t)r * 256 + threadIdx.x;
    if (i < nvec) {
      const uint4 v = src[i];
      if (dst) dst[i] = v;
      if (check) acc |= qs_dev_range_bits(v, q);
    }
  }
  if (check && __any((acc >> 12) != 0) && (threadIdx.x & 63) == 0)
    atomicMax(a.words + R.job, (uint32_t)(R.ncomp - R.comp));
}

__global__ void __launch_bounds__(256)
qs_dev_fixup_batch_kernel(const QsDevBatchArgs a) {
  const int c = qs_devb_find(a);
  const QsDevBRec& R = a.rec[c];
  if (blockIdx.x < R.blk0 || R.job < 0 || R.job >= a.njobs) return;
  const uint32_t w = a.words[R.job];                         // n - k, or 0
  if (R.stop_writer && blockIdx.x == R.blk0 && threadIdx.x == 0) a.d_stop[R.job] = (w != 0 || R.static_stop) ? 1 : 0;
  if (!w) return;
  const uint32_t k = (uint32_t)R.ncomp - w;
  if (k >= QS_DEV_MAXC) return;
  const int act = R.act[k];
  const uint64_t nvec = a.nvec[c];
  const uint64_t v0 = (uint64_t)(blockIdx.x - R.blk0) * QS_DEVB_FIX_VPB;
  if (act == QS_DEV_KEEP || v0 >= nvec) return;
  const uint4* __restrict__ src = qs_devb_snap(a, R, nvec);
  if (!src) return;
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(a.coef[c]);
  int32_t q[8];
  qs_devb_lane_quant(R, q);
  for (int r = 0; r < QS_DEVB_FIX_VPB / 256; ++r) {
    const uint64_t i = v0 + (uint64_t)r * 256 + threadIdx.x;
    if (i < nvec) {
      const uint4 v = src[i];
      dst[i] = act == QS_DEV_RESTORE ? v : qs_dev_dequant(v, q, act == QS_DEV_DEQUANT_CLAMP);
    }
  }
}

// zeroes the range-check words.  A kernel, not a memset call: a captured 20-byte zero memset over five words left
// nonzero values in the first four on the second replay of a graph on MI355X / ROCm 7 (the fifth read 0).
__global__ void __launch_bounds__(256)
qs_dev_clear_words_kernel(uint32_t* __restrict__ words, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) words[i] = 0;
}

void qs_launch_dev_clear_words(uint32_t* words, int n, hipStream_t s) {
  const int g = (n + 255) / 256;
  hipLaunchKernelGGL(qs_dev_clear_words_kernel, dim3(g < 1 ? 1 : g > 64 ? 64 : g), dim3(256), 0, s, words, n);
}

// the grid of a chunk: the workgroups its records own (the same prefix the prepare call wrote into rec[].blk0)
static unsigned qs_devb_grid(const QsDevBatchArgs& a, uint64_t vpb) {
  uint64_t g = 0;
  for (int c = 0; c < a.n; ++c) g += (a.nvec[c] + vpb - 1) / vpb;
  return (unsigned)g;
}

void qs_launch_dev_precheck_batch(const QsDevBatchArgs& a, hipStream_t s) {
  if (const unsigned g = qs_devb_grid(a, QS_DEVB_PRE_VPB))
    hipLaunchKernelGGL(qs_dev_precheck_batch_kernel, dim3(g), dim3(256), 0, s, a);
}

void qs_launch_dev_fixup_batch(const QsDevBatchArgs& a, hipStream_t s) {
  if (const unsigned g = qs_devb_grid(a, QS_DEVB_FIX_VPB))
    hipLaunchKernelGGL(qs_dev_fixup_batch_kernel, dim3(g), dim3(256), 0, s, a);
}
