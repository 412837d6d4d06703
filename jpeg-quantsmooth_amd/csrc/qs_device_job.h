// qs_device_job.h -- what the device-resident job route (qs_device_job.cpp) shares with its kernels
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

// One precheck / fix-up launch per chunk of components of one or many jobs.  What prepare derived from the quant
// tables lives in the workspace (QsDevBRec, one per component of a chunk); what addresses caller memory travels in the
// kernel arguments of the run call (QsDevBatchArgs).  The kernels bound every access by the latter: a record that does
// not match the run's geometry can give wrong numbers, never a stray address.
#define QS_DEVB_CHUNK 64            // components per launch (about 1.1 KiB of kernel arguments)
#define QS_DEVB_PRE_VPB 1024        // 16-byte vectors per workgroup: precheck (4 per lane) ...
#define QS_DEVB_FIX_VPB 8192        // ... and fix-up (32 per lane; nearly every workgroup exits at once)

struct QsDevBRec {
  int32_t q[64];                    // quantval as stored in the file, natural order
  int32_t act[QS_DEV_MAXC];         // QS_DEV_* when its job's first tripped component is k = 0..3
  uint64_t snap_off;                // byte offset of its snapshot in the workspace; QS_DEVB_NO_SNAP: none
  int32_t job;                      // its job's index in the batch: range-check word and d_stop entry
  int32_t comp, ncomp;              // component j of a job of n components (the word holds n - k)
  int32_t check;                    // precheck: run the range test on it
  int32_t stop_writer;              // fix-up: the record that writes d_stop[job]
  uint32_t blk0;                    // its first workgroup in its chunk's launch (prefix over the chunk)
  int32_t static_stop;              // its job's quant tables alone decide stop (a value >= 0x800, reference :2504)
  int32_t pad;
};
#define QS_DEVB_NO_SNAP (~(uint64_t)0)

// passed by value (kernarg segment): one chunk of records
struct QsDevBatchArgs {
  const QsDevBRec* rec;             // the chunk's records (workspace)
  char* ws;                         // the workspace and its size: snapshots must lie inside it
  uint64_t ws_bytes;
  uint32_t* words;                  // one range-check word per job (workspace)
  int32_t* d_stop;                  // the caller's int32[njobs] (fix-up)
  int32_t njobs, n;                 // jobs in the batch, records in the chunk
  int16_t* coef[QS_DEVB_CHUNK];     // record c's coefficient array ...
  uint64_t nvec[QS_DEVB_CHUNK];     // ... and its 16-byte vectors (blocks * 8)
};

void qs_launch_dev_clear_words(uint32_t* words, int n, hipStream_t s);
void qs_launch_dev_precheck_batch(const QsDevBatchArgs& a, hipStream_t s);
void qs_launch_dev_fixup_batch(const QsDevBatchArgs& a, hipStream_t s);
