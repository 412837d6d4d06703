// qs_stage.h -- what the host drivers of the device stages share (qs_device_job.cpp, qs_decode_job.cpp,
// qs_encode_job.cpp, qs_read_job.cpp, qs_compress_job.cpp): the guard at the C ABI, the workspace check and layout, the
// upload that ends a prepare call, and the checks on a qs_hip_job that several stages make with the same message.
// Host only, included after qs_common.h; everything is static, so the library exports nothing from here.
#pragma once
#include <new>
#include <vector>

// The C ABI never lets a C++ exception (std::bad_alloc from the host-side containers) escape.
template <class F> static int guarded(F f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return qs_fail(QS_HIP_ENOMEM, "out of host memory");
  } catch (...) {
    return qs_fail(QS_HIP_ENODEV, "unexpected internal error");
  }
}

static inline int device_ok() {
  if (qs_hip_device_count() <= 0)
    return qs_fail(QS_HIP_ENODEV, "no HIP device available (this library has no CPU fallback)");
  return QS_HIP_OK;
}

static inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline uint64_t align_up(uint64_t v, uint64_t a = 256) { return (v + a - 1) / a * a; }

struct Who {                                // "<call>: job <i>", the prefix of a job's error messages in a batch
  char s[96];
  Who(const char* who, int i, bool standalone = false) {
    if (standalone) snprintf(s, sizeof s, "%s", who);
    else snprintf(s, sizeof s, "%s: job %d", who, i);
  }
};

// ---- the workspace: byte offsets in steps of 256, the check of what the caller passed, the upload of the descriptors ----

struct Layout {
  uint64_t total = 0;
  uint64_t take(uint64_t bytes) {
    const uint64_t at = total;
    total += align_up(bytes);
    return at;
  }
};

static inline bool workspace_ok(const void* d_workspace, size_t bytes, uint64_t need) {
  return d_workspace && !(reinterpret_cast<uintptr_t>(d_workspace) & 255) && bytes >= need;
}

static inline int check_workspace(uint64_t need, const void* d_workspace, size_t bytes, const char* who,
                                  const char* what = "batch") {
  if (!workspace_ok(d_workspace, bytes, need))
    return qs_fail(QS_HIP_EINVAL, "%s: workspace of %zu bytes (256-byte aligned), the %s needs %llu", who, bytes, what,
                   (unsigned long long)need);
  return QS_HIP_OK;
}

// the end of a prepare call: the descriptors to the front of the workspace
template <class T> static int upload(void* d_workspace, const std::vector<T>& v, hipStream_t s) {
  HIP_TRY(hipMemcpyAsync(d_workspace, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));                        // (a pageable source: it must outlive the copy)
  return QS_HIP_OK;
}

// ---- checks on a job; `who` names the call (and the job of a batch) ----

static inline int check_job(const qs_hip_job* job, const char* who) {
  if (!job || job->ncomp < 1 || job->ncomp > QS_HIP_MAXC) return qs_fail(QS_HIP_EINVAL, "%s: bad job", who);
  return QS_HIP_OK;
}

static inline int check_sampling(const qs_hip_job* job, int ci, const char* who) {
  if (job->hsamp[ci] < 1 || job->hsamp[ci] > 4 || job->vsamp[ci] < 1 || job->vsamp[ci] > 4)   // JPEG: 1..4
    return qs_fail(QS_HIP_EINVAL, "%s: component %d has sampling factors %dx%d", who, ci, job->hsamp[ci], job->vsamp[ci]);
  return QS_HIP_OK;
}

static inline int check_block_count(const qs_hip_job* job, int ci, const char* who) {   // (the kernels index blocks by int)
  if ((long long)job->wblk[ci] * job->hblk[ci] > 0x7fffffffLL)
    return qs_fail(QS_HIP_EINVAL, "%s: component %d has more than 2^31 blocks", who, ci);
  return QS_HIP_OK;
}

static inline int check_array(const void* arr, int ci, bool replacement, const char* who) {   // (16 bytes per lane)
  if (!arr || (reinterpret_cast<uintptr_t>(arr) & 15))
    return qs_fail(QS_HIP_EINVAL, "%s: component %d%s has no data or is not 16-byte aligned", who, ci,
                   replacement ? " (replacement chroma)" : "");
  return QS_HIP_OK;
}

// ---- the pixel stages (decode, compress): the jobs they take; `noun` is the stage in the messages ----

enum { QS_PIX_GRAY = 0, QS_PIX_YCC = 1, QS_PIX_RGB = 2 };   // = QS_DEC_* = QS_CMP_*

// the image size, the layout from (ncomp, colorspace), a quant table and legal factors per component; zero_q: a
// quantiser of 0 is refused as well (the compress divides by it)
static inline int pixel_job(const qs_hip_job* job, const char* noun, bool zero_q, int* layout, const char* who) {
  if (int r = check_job(job, who)) return r;
  if (job->image_width <= 0 || job->image_height <= 0)
    return qs_fail(QS_HIP_EINVAL, "%s: the %s needs image_width x image_height (got %d x %d)", who, noun,
                   job->image_width, job->image_height);
  if (job->image_width > 65500 || job->image_height > 65500)
    return qs_fail(QS_HIP_EINVAL, "%s: image of %d x %d exceeds JPEG's 65500", who, job->image_width, job->image_height);
  if (job->ncomp == 1 && job->colorspace == 1) *layout = QS_PIX_GRAY;
  else if (job->ncomp == 3 && job->colorspace == 3) *layout = QS_PIX_YCC;
  else if (job->ncomp == 3 && job->colorspace == 2) *layout = QS_PIX_RGB;
  else
    return qs_fail(QS_HIP_ENOTSUP, "%s: %d components in colour space %d: the device %s covers grayscale, YCbCr "
                   "and RGB (3 components)", who, job->ncomp, job->colorspace, noun);
  for (int ci = 0; ci < job->ncomp; ++ci) {
    if (!job->has_quant[ci]) return qs_fail(QS_HIP_EINVAL, "%s: component %d has no quant table", who, ci);
    for (int i = 0; zero_q && i < 64; ++i)
      if (job->quant[ci][i] == 0) return qs_fail(QS_HIP_EINVAL, "%s: component %d has a quantiser of 0", who, ci);
    if (int r = check_sampling(job, ci, who)) return r;
  }
  return QS_HIP_OK;
}

// three components at their own sampling: 1x1 chroma, and the luma factors libjpeg 9 pairs with DCT-scaled chroma
static inline int pixel_sampling(const qs_hip_job* job, const char* noun, const char* who) {
  for (int ci = 1; ci < 3; ++ci)
    if (job->hsamp[ci] != 1 || job->vsamp[ci] != 1)
      return qs_fail(QS_HIP_ENOTSUP, "%s: chroma component %d is sampled %dx%d: the device %s needs 1x1 chroma", who, ci,
                     job->hsamp[ci], job->vsamp[ci], noun);
  const int h = job->hsamp[0], v = job->vsamp[0];
  if (!((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 1 && v == 2) || (h == 2 && v == 2) || (h == 4 && v == 1)))
    return qs_fail(QS_HIP_ENOTSUP, "%s: luma sampling %dx%d: the device %s covers 1x1, 2x1, 1x2, 2x2 and 4x1", who, h, v,
                   noun);
  return QS_HIP_OK;
}

// `what`: "output" / "pixel"
static inline int check_pitch(size_t pitch, int width, int samples, const char* what, const char* who) {
  if (pitch < (size_t)width * samples || pitch > ((size_t)1 << 40))
    return qs_fail(QS_HIP_EINVAL, "%s: %s pitch %zu for rows of %d x %d samples", who, what, pitch, width, samples);
  return QS_HIP_OK;
}
