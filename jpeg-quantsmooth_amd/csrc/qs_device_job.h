// qs_device_job.h -- what the device-resident job route (qs_device_job.cpp) shares with its two kernels
// (qs_kernels_device.hip).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define QS_DEV_MAXC 4

// what the fix-up does to a component when the reference would have stopped at component k
enum {
  QS_DEV_KEEP = 0,            // the result the passes produced (or the untouched input) is the reference's
  QS_DEV_RESTORE = 1,         // the reference never touched it: the snapshot
  QS_DEV_DEQUANT = 2,         // int16(coef * quantval), reference :2551-2566
  QS_DEV_DEQUANT_CLAMP = 3    // the same, then the +-1023 clamp: the component whose range check tripped (:2598, 2668-2689)
};

struct QsDevComp {
  int16_t* coef;              // the caller's coefficient array (device)
  int16_t* snap;              // its snapshot in the workspace, null when no fix-up can need it
  uint64_t nvec;              // 16-byte vectors: blocks * 8
  int32_t check;              // its first pass A would run the range check (a component processed with passes)
  int32_t act[QS_DEV_MAXC];   // QS_DEV_* when the first tripped component is k = 0..3
  int32_t q[64];              // quantval as stored in the file, natural order
};

// passed by value (kernarg segment)
struct QsDevJobArgs {
  QsDevComp c[QS_DEV_MAXC];
  int32_t n;                  // components
  int32_t static_stop;        // the quant tables alone decide stop (a value >= 0x800, reference :2504)
};

// first_bad: the range-check word, zeroed before the precheck; n - k when component k is the first that tripped
void qs_launch_dev_precheck(const QsDevJobArgs& a, uint32_t* first_bad, hipStream_t s);
void qs_launch_dev_fixup(const QsDevJobArgs& a, const uint32_t* first_bad, int32_t* d_stop, hipStream_t s);
