// qs_compress_job.cpp -- the device compress of the flat C ABI (include/jpegqs_hip.h):
// qs_hip_compress_device_batch_info / _prepare (and their _opts forms) / qs_hip_compress_device_batch.  The coefficient
// arrays libjpeg 9 holds after jpeg_write_scanlines (JDCT_ISLOW, smoothing_factor 0) for device-resident pixels, written
// into the arrays of qs_hip_job records, every job of a batch in one launch (qs_kernels_compress.hip).  The chroma
// downsampling is per job (qs_hip_compress_opts): the box filter of do_fancy_downsampling FALSE, which is what the
// calls without opts do, or libjpeg 9's default, 2x chroma through 16-point scaled forward DCTs.  The `fancy` argument
// of the calls without opts keeps its meaning: anything but 0 is QS_HIP_ENOTSUP.
//
// Workspace: one QsCmpJob per job (geometry, mode, tables and their reciprocals, the job's tiles in its chunk's launch),
// written by prepare; its layout and contents are a function of the jobs' geometry and tables alone.  The run passes
// the pixels and the arrays in the kernel arguments, QS_CMP_CHUNK jobs per launch.
#include "qs_common.h"
#include "qs_stage.h"
#include "qs_compress.h"

#include <algorithm>

void qs_launch_compress(const QsCmpArgs& a, int tiles, hipStream_t s);

static_assert(QS_CMP_CHUNK == QS_HIP_COMPRESS_CHUNK, "the header documents the launch chunk");

static_assert(QS_CMP_GRAY == QS_PIX_GRAY && QS_CMP_YCC == QS_PIX_YCC && QS_CMP_RGB == QS_PIX_RGB,
              "pixel_job (qs_stage.h) returns the layouts of the kernel");

namespace {

// one job's layout, input shape and descriptor (pointers left null when d_pix is null: the info and prepare calls).
// The run call (d_pix set) needs the geometry, the tiles and the addresses only: the tables were checked and their
// reciprocals written by prepare, so it leaves D->q and D->recip alone.
int describe(const qs_hip_job* job, const uint8_t* d_pix, size_t pitch, QsCmpJob* D, QsCmpPtrs* P,
             qs_hip_compress_info* info, const char* who) {
  const bool tables = d_pix == nullptr;
  int layout;
  if (int r = pixel_job(job, "compress", tables, &layout, who)) return r;
  memset(D, 0, sizeof *D);
  int hs = job->hsamp[0], vs = job->vsamp[0];
  if (layout == QS_CMP_GRAY) hs = vs = 1;                  // one component: its own grid is the pixel grid
  else if (int r = pixel_sampling(job, "compress", who)) return r;
  const int W = job->image_width, Hh = job->image_height;
  D->width = W; D->height = Hh;
  D->layout = layout;
  D->nin = layout == QS_CMP_GRAY ? 1 : 3;
  D->hs = hs; D->vs = vs;
  for (int ci = 0; ci < job->ncomp; ++ci) {
    D->wib[ci] = qc_blocks(W, ci ? 1 : hs, hs);
    D->hib[ci] = qc_blocks(Hh, ci ? 1 : vs, vs);
    D->stride[ci] = job->wblk[ci];
    if (job->wblk[ci] < D->wib[ci] || job->hblk[ci] < D->hib[ci])
      return qs_fail(QS_HIP_EINVAL, "%s: component %d has %d x %d blocks, a %d x %d image needs %d x %d", who, ci,
                     job->wblk[ci], job->hblk[ci], W, Hh, D->wib[ci], D->hib[ci]);
    if (int r = check_block_count(job, ci, who)) return r;
    if (d_pix)
      if (int r = check_array(job->coef[ci], ci, false, who)) return r;
    for (int i = 0; tables && i < 64; ++i) {
      D->q[ci][i] = job->quant[ci][i];
      D->recip[ci][i] = qc_recip((uint32_t)job->quant[ci][i] << 3);
    }
    if (P) {
      P->coef[ci] = job->coef[ci];
      P->nblk[ci] = job->wblk[ci] * job->hblk[ci];
    }
  }
  D->tiles_x = ceil_div(W, QS_CMP_TW);
  D->tiles = D->tiles_x * ceil_div(Hh, QS_CMP_TH);
  if (d_pix) {
    if (int r = check_pitch(pitch, W, D->nin, "pixel", who)) return r;
    if (P) {
      P->pix = d_pix;
      P->pitch = (int64_t)pitch;
      P->width = W; P->height = Hh;
    }
  }
  if (info) {
    info->width = W; info->height = Hh; info->channels = D->nin; info->layout = layout;
    for (int ci = 0; ci < QS_HIP_MAXC; ++ci) {
      info->wblk[ci] = ci < job->ncomp ? D->wib[ci] : 0;
      info->hblk[ci] = ci < job->ncomp ? D->hib[ci] : 0;
    }
  }
  return QS_HIP_OK;
}

// the descriptors of a batch and, with d_pix (the run), the kernel-argument records; the tile prefix restarts with
// every chunk of QS_CMP_CHUNK jobs (one launch each)
int describe_all(qs_hip_job* const* jobs, int njobs, const qs_hip_compress_opts* const* opts,
                 const uint8_t* const* d_pix, const size_t* pitch, std::vector<QsCmpJob>& D, std::vector<QsCmpPtrs>* P,
                 qs_hip_compress_info* info, const char* who) {
  if (!jobs || njobs < 1) return qs_fail(QS_HIP_EINVAL, "%s: %d jobs (at least one)", who, njobs);
  if (d_pix && !pitch) return qs_fail(QS_HIP_EINVAL, "%s: null pitch", who);
  D.assign((size_t)njobs, QsCmpJob());
  if (P) P->assign((size_t)njobs, QsCmpPtrs());
  long long tiles = 0;
  for (int i = 0; i < njobs; ++i) {
    const uint8_t* pix = d_pix ? d_pix[i] : nullptr;
    if (d_pix && !pix) return qs_fail(QS_HIP_EINVAL, "%s: job %d has no pixels", who, i);
    if (int r = describe(jobs[i], pix, d_pix ? pitch[i] : 0, &D[i], P ? &(*P)[i] : nullptr, info ? &info[i] : nullptr,
                         Who(who, i).s)) return r;
    if (const qs_hip_compress_opts* o = opts ? opts[i] : nullptr) {
      if (o->downsampling != QS_HIP_DOWNSAMPLE_BOX && o->downsampling != QS_HIP_DOWNSAMPLE_DCT)
        return qs_fail(QS_HIP_EINVAL, "%s: job %d: downsampling %d (QS_HIP_DOWNSAMPLE_BOX or QS_HIP_DOWNSAMPLE_DCT)", who, i,
                       o->downsampling);
      if (o->reserved[0] || o->reserved[1] || o->reserved[2])
        return qs_fail(QS_HIP_EINVAL, "%s: job %d: the reserved fields of qs_hip_compress_opts must be 0", who, i);
      D[i].mode = o->downsampling == QS_HIP_DOWNSAMPLE_DCT ? QS_CMP_DS_DCT : QS_CMP_DS_BOX;
    }
    if (i % QS_CMP_CHUNK == 0) tiles = 0;
    D[i].tile0 = (int)tiles;
    tiles += D[i].tiles;
    if (tiles > 0x7fffffff) return qs_fail(QS_HIP_EINVAL, "%s: more than 2^31 tiles in one launch", who);
  }
  return QS_HIP_OK;
}

size_t workspace_bytes(int njobs) { return (size_t)njobs * sizeof(QsCmpJob); }

int no_fancy(int fancy, const char* who) {
  if (fancy)
    return qs_fail(QS_HIP_ENOTSUP, "%s: fancy != 0 is refused: pass 0 for the box filter of do_fancy_downsampling = FALSE; "
                   "libjpeg 9's default (2x chroma through 16-point scaled DCTs) is QS_HIP_DOWNSAMPLE_DCT of the _opts "
                   "calls", who);
  return QS_HIP_OK;
}

int info_impl(qs_hip_job* const* jobs, int njobs, const qs_hip_compress_opts* const* opts, int fancy,
              qs_hip_compress_info* per_job, size_t* bytes, const char* who) {
  if (!per_job || !bytes) return qs_fail(QS_HIP_EINVAL, "%s: null result", who);
  std::vector<QsCmpJob> D;
  if (int r = describe_all(jobs, njobs, opts, nullptr, nullptr, D, nullptr, per_job, who)) return r;
  if (int r = no_fancy(fancy, who)) return r;
  *bytes = workspace_bytes(njobs);
  return QS_HIP_OK;
}

int prepare_impl(qs_hip_job* const* jobs, int njobs, const qs_hip_compress_opts* const* opts, int fancy,
                 void* d_workspace, size_t bytes, void* stream, const char* who) {
  std::vector<QsCmpJob> D;
  if (int r = describe_all(jobs, njobs, opts, nullptr, nullptr, D, nullptr, nullptr, who)) return r;
  if (int r = no_fancy(fancy, who)) return r;
  if (int r = check_workspace(workspace_bytes(njobs), d_workspace, bytes, who)) return r;
  if (int r = device_ok()) return r;
  return upload(d_workspace, D, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" int qs_hip_compress_device_batch_info(qs_hip_job* const* jobs, int njobs, int fancy,
                                                 qs_hip_compress_info* per_job, size_t* bytes) {
  return guarded([&]() -> int {
    return info_impl(jobs, njobs, nullptr, fancy, per_job, bytes, "qs_hip_compress_device_batch_info");
  });
}

extern "C" int qs_hip_compress_device_batch_info_opts(qs_hip_job* const* jobs, int njobs,
                                                      const qs_hip_compress_opts* const* opts,
                                                      qs_hip_compress_info* per_job, size_t* bytes) {
  return guarded([&]() -> int {
    return info_impl(jobs, njobs, opts, 0, per_job, bytes, "qs_hip_compress_device_batch_info_opts");
  });
}

extern "C" int qs_hip_compress_device_batch_prepare(qs_hip_job* const* jobs, int njobs, int fancy, void* d_workspace,
                                                    size_t bytes, void* stream) {
  return guarded([&]() -> int {
    return prepare_impl(jobs, njobs, nullptr, fancy, d_workspace, bytes, stream, "qs_hip_compress_device_batch_prepare");
  });
}

extern "C" int qs_hip_compress_device_batch_prepare_opts(qs_hip_job* const* jobs, int njobs,
                                                         const qs_hip_compress_opts* const* opts, void* d_workspace,
                                                         size_t bytes, void* stream) {
  return guarded([&]() -> int {
    return prepare_impl(jobs, njobs, opts, 0, d_workspace, bytes, stream, "qs_hip_compress_device_batch_prepare_opts");
  });
}

extern "C" int qs_hip_compress_device_batch(qs_hip_job* const* jobs, int njobs, const uint8_t* const* d_pixels,
                                            const size_t* pitch, void* d_workspace, size_t bytes, void* stream) {
  return guarded([&]() -> int {
    const char* who = "qs_hip_compress_device_batch";
    std::vector<QsCmpJob> D;
    std::vector<QsCmpPtrs> P;
    if (!d_pixels) return qs_fail(QS_HIP_EINVAL, "%s: null d_pixels", who);
    if (int r = describe_all(jobs, njobs, nullptr, d_pixels, pitch, D, &P, nullptr, who)) return r;
    if (int r = check_workspace(workspace_bytes(njobs), d_workspace, bytes, who)) return r;
    if (int r = device_ok()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int j0 = 0; j0 < njobs; j0 += QS_CMP_CHUNK) {
      QsCmpArgs a;
      memset(&a, 0, sizeof a);
      a.jobs = static_cast<const QsCmpJob*>(d_workspace) + j0;
      a.n = std::min(QS_CMP_CHUNK, njobs - j0);
      for (int k = 0; k < a.n; ++k) a.p[k] = P[(size_t)j0 + k];
      const QsCmpJob& last = D[(size_t)j0 + a.n - 1];
      qs_launch_compress(a, last.tile0 + last.tiles, s);
    }
    HIP_TRY(hipGetLastError());
    return QS_HIP_OK;
  });
}
