// qs_decode_job.cpp -- the device decode to pixels of the flat C ABI (include/jpegqs_hip.h):
// qs_hip_decode_device_batch_info / _prepare (and their _opts forms) / qs_hip_decode_device_batch.  What libjpeg 9
// delivers from jpeg_read_scanlines (JDCT_ISLOW, default upsampling and output colour space) for the coefficient arrays
// of qs_hip_job records -- typically the result of qs_hip_do_quantsmooth_device[_batch] -- computed on the device, every
// job of a batch in one launch (qs_kernels_decode.hip).  The chroma upsampling is per job (qs_hip_decode_opts):
// libjpeg 9's DCT scaling, which is what the calls without opts do, or libjpeg-turbo's triangle filters; so is the size
// (qs_hip_decode_scale_opts): libjpeg 9's scale_denom 1, 2, 4 or 8, the reduced sizes through a kernel of their own
// (qs_decode_scaled_kernel), at most two launches per chunk.
//
// Workspace: one QsDecJob per job (geometry, mode, tables, the job's tiles in its chunk's launch), written by prepare; its
// layout and contents are a function of the jobs' geometry and tables alone.  The run passes the arrays and outputs in
// the kernel arguments, QS_DEC_CHUNK jobs per launch.
#include "qs_common.h"
#include "qs_stage.h"
#include "qs_decode.h"
#include "qs_encode_plan.h"

#include <algorithm>

void qs_launch_decode(const QsDecArgs& a, int tiles, hipStream_t s);
void qs_launch_decode_scaled(const QsDecArgs& a, int tiles, hipStream_t s);

static_assert(QS_DEC_GRAY == QS_PIX_GRAY && QS_DEC_YCC == QS_PIX_YCC && QS_DEC_RGB == QS_PIX_RGB,
              "pixel_job (qs_stage.h) returns the layouts of the kernel");

namespace {

// What one job's options come to: the upsampling mode and m = 8 / scale_denom, the samples per luma block edge.
struct Mode {
  int upsampling = QS_DEC_UP_DCT;
  int m = 8;
};

// The run call has no options, and the output size, the pitch check and the launches depend on the scales: prepare
// leaves each job's m here, by workspace address.  A workspace the run does not find (never prepared with this library
// instance, or pushed out by 256 later ones) runs at full size, as it always did; if its descriptors say otherwise the
// full-size kernel finds no tiles for them and writes nothing.
QsPrepared<std::vector<uint8_t>> g_scales(256);

// one job's layout, output shape and descriptor (pointers left null when d_out is null: the info call)
int describe(const qs_hip_job* job, int m, uint8_t* d_out, size_t pitch, QsDecJob* D, QsDecPtrs* P,
             qs_hip_decode_info* info, const char* who) {
  int layout;
  if (int r = pixel_job(job, "decode", false, &layout, who)) return r;
  memset(D, 0, sizeof *D);
  const int W = job->image_width, Hh = job->image_height;
  // the two geometries: variant 0 = replacement chroma when the job has it, variant 1 = the original arrays
  const bool up = job->up_wblk > 0 && layout != QS_DEC_GRAY;
  for (int v = 0; v < (up ? 2 : 1); ++v) {
    QsDecGeom& g = D->g[v];
    const bool repl = up && v == 0;
    int hs = job->hsamp[0], vs = job->vsamp[0];
    if (layout == QS_DEC_GRAY) hs = vs = 1;                // one component: its own grid is the pixel grid
    else if (repl) hs = vs = 1;
    else if (int rc = pixel_sampling(job, "decode", who)) return rc;   // (the only upsampler here: DCT-scaled chroma)
    g.hs = hs; g.vs = vs;
    for (int ci = 0; ci < job->ncomp; ++ci) {
      const bool r = repl && ci > 0;
      g.wblk[ci] = r ? job->up_wblk : job->wblk[ci];
      g.hblk[ci] = r ? job->up_hblk : job->hblk[ci];
      const int16_t* arr = r ? job->coef_up[ci - 1] : job->coef[ci];
      const int slot = (up && !repl && ci) ? 2 + ci : ci;
      const int cw = ci ? 8 * hs : 8, ch = ci ? 8 * vs : 8;
      const int nw = ceil_div(W, cw), nh = ceil_div(Hh, ch);
      if (g.wblk[ci] < nw || g.hblk[ci] < nh)
        return qs_fail(QS_HIP_EINVAL, "%s: component %d%s has %d x %d blocks, a %d x %d image needs %d x %d", who, ci,
                       r ? " (replacement chroma)" : "", g.wblk[ci], g.hblk[ci], W, Hh, nw, nh);
      if (d_out)
        if (int rc = check_array(arr, ci, r, who)) return rc;
      if (P) {
        P->coef[slot] = arr;
        P->nblk[slot] = g.wblk[ci] * g.hblk[ci];
      }
    }
  }
  // the output: libjpeg's ceil(image_width * m / 8) x ceil(image_height * m / 8) (jpeg_core_output_dimensions)
  const int OW = ceil_div((long long)W * m, 8), OH = ceil_div((long long)Hh * m, 8);
  D->two = up ? 1 : 0;
  D->width = OW; D->height = OH;
  D->layout = layout;
  D->nout = layout == QS_DEC_GRAY ? 1 : 3;
  if (m == 8) {                                            // (a reduced job has no tiles in the full-size kernel's launch)
    D->tiles_x = ceil_div(OW, QS_DEC_TW);
    D->tiles = D->tiles_x * ceil_div(OH, QS_DEC_TH);
  }
  for (int ci = 0; ci < job->ncomp; ++ci)
    for (int i = 0; i < 64; ++i) D->q[ci][i] = job->quant[ci][i];
  if (d_out) {
    if (int rc = check_pitch(pitch, OW, D->nout, "output", who)) return rc;
    if (P) {
      P->out = d_out;
      P->pitch = (int64_t)pitch;
      P->width = OW; P->height = OH;
    }
  }
  if (info) {
    info->width = OW; info->height = OH; info->channels = D->nout; info->layout = layout;
  }
  return QS_HIP_OK;
}

// the descriptors of a batch and, with d_out (the run), the kernel-argument records; the tile prefix restarts with
// every chunk of QS_DEC_CHUNK jobs (one launch each)
int describe_all(qs_hip_job* const* jobs, int njobs, const Mode* modes, uint8_t* const* d_out,
                 const size_t* pitch, std::vector<QsDecJob>& D, std::vector<QsDecPtrs>* P, qs_hip_decode_info* info, const char* who,
                 std::vector<int>* stile_end = nullptr) {       // stile_end[i]: the scaled launch's workgroups up to and with job i
  if (!jobs || njobs < 1) return qs_fail(QS_HIP_EINVAL, "%s: %d jobs (at least one)", who, njobs);
  if (d_out && !pitch) return qs_fail(QS_HIP_EINVAL, "%s: null out_pitch", who);
  D.assign((size_t)njobs, QsDecJob());
  if (P) P->assign((size_t)njobs, QsDecPtrs());
  if (stile_end) stile_end->assign((size_t)njobs, 0);
  long long tiles = 0, stiles = 0;
  for (int i = 0; i < njobs; ++i) {
    const Mode mode = modes ? modes[i] : Mode();
    uint8_t* out = d_out ? d_out[i] : nullptr;
    if (d_out && !out) return qs_fail(QS_HIP_EINVAL, "%s: job %d has no output buffer", who, i);
    if (int r = describe(jobs[i], mode.m, out, d_out ? pitch[i] : 0, &D[i], P ? &(*P)[i] : nullptr, info ? &info[i] : nullptr,
                         Who(who, i).s)) return r;
    D[i].upsampling = (int16_t)(mode.m == 8 ? mode.upsampling : QS_DEC_UP_DCT + 256 * (8 / mode.m));   // (qd_job_m)
    if (i % QS_DEC_CHUNK == 0) tiles = stiles = 0;
    D[i].tile0 = (int)tiles;
    if (P) (*P)[(size_t)i].stile0 = (int)stiles;
    tiles += D[i].tiles;
    if (mode.m != 8) stiles += (long long)ceil_div(D[i].width, QS_DEC_TW) * ceil_div(D[i].height, QS_DEC_TH);
    if (stile_end) (*stile_end)[(size_t)i] = (int)std::min(stiles, 0x7fffffffLL);
    if (tiles > 0x7fffffff || stiles > 0x7fffffff) return qs_fail(QS_HIP_EINVAL, "%s: more than 2^31 output tiles in one launch", who);
  }
  return QS_HIP_OK;
}

// the jobs' modes from either options record (one of the two arrays, or neither); checked before anything else
int read_modes(int njobs, const qs_hip_decode_opts* const* opts, const qs_hip_decode_scale_opts* const* sopts,
               std::vector<Mode>& modes, const char* who) {
  modes.assign((size_t)std::max(njobs, 0), Mode());
  for (int i = 0; i < njobs; ++i) {
    int up = QS_HIP_UPSAMPLE_DCT, denom = 1;
    if (opts && opts[i]) up = opts[i]->upsampling;
    if (sopts && sopts[i]) { up = sopts[i]->upsampling; denom = sopts[i]->scale_denom; }
    if (up != QS_HIP_UPSAMPLE_DCT && up != QS_HIP_UPSAMPLE_TRIANGLE)
      return qs_fail(QS_HIP_EINVAL, "%s: job %d: upsampling %d (QS_HIP_UPSAMPLE_DCT or QS_HIP_UPSAMPLE_TRIANGLE)", who, i, up);
    if (denom != 1 && denom != 2 && denom != 4 && denom != 8)
      return qs_fail(QS_HIP_EINVAL, "%s: job %d: scale_denom %d (1, 2, 4 or 8)", who, i, denom);
    if (up == QS_HIP_UPSAMPLE_TRIANGLE && denom != 1)
      return qs_fail(QS_HIP_ENOTSUP, "%s: job %d: QS_HIP_UPSAMPLE_TRIANGLE with scale_denom %d: the triangle mode decodes "
                     "at full size only", who, i, denom);
    modes[(size_t)i].upsampling = up == QS_HIP_UPSAMPLE_TRIANGLE ? QS_DEC_UP_TRIANGLE : QS_DEC_UP_DCT;
    modes[(size_t)i].m = 8 / denom;
  }
  return QS_HIP_OK;
}

size_t workspace_bytes(int njobs) { return (size_t)njobs * sizeof(QsDecJob); }

int info_impl(qs_hip_job* const* jobs, int njobs, const qs_hip_decode_opts* const* opts,
              const qs_hip_decode_scale_opts* const* sopts, qs_hip_decode_info* per_job, size_t* bytes, const char* who) {
  if (!per_job || !bytes) return qs_fail(QS_HIP_EINVAL, "%s: null result", who);
  std::vector<QsDecJob> D;
  std::vector<Mode> modes;
  if (int r = read_modes(njobs, opts, sopts, modes, who)) return r;
  if (int r = describe_all(jobs, njobs, modes.data(), nullptr, nullptr, D, nullptr, per_job, who)) return r;
  *bytes = workspace_bytes(njobs);
  return QS_HIP_OK;
}

int prepare_impl(qs_hip_job* const* jobs, int njobs, const qs_hip_decode_opts* const* opts,
                 const qs_hip_decode_scale_opts* const* sopts, void* d_workspace, size_t bytes, void* stream,
                 const char* who) {
  std::vector<QsDecJob> D;
  std::vector<Mode> modes;
  if (int r = read_modes(njobs, opts, sopts, modes, who)) return r;
  if (int r = describe_all(jobs, njobs, modes.data(), nullptr, nullptr, D, nullptr, nullptr, who)) return r;
  if (int r = check_workspace(workspace_bytes(njobs), d_workspace, bytes, who)) return r;
  if (int r = device_ok()) return r;
  if (int r = upload(d_workspace, D, static_cast<hipStream_t>(stream))) return r;
  std::vector<uint8_t> ms((size_t)njobs);
  for (int i = 0; i < njobs; ++i) ms[(size_t)i] = (uint8_t)modes[(size_t)i].m;
  g_scales.store(d_workspace, std::move(ms));
  return QS_HIP_OK;
}

}  // namespace

extern "C" int qs_hip_decode_device_batch_info(qs_hip_job* const* jobs, int njobs, qs_hip_decode_info* per_job,
                                               size_t* bytes) {
  return guarded([&]() -> int {
    return info_impl(jobs, njobs, nullptr, nullptr, per_job, bytes, "qs_hip_decode_device_batch_info");
  });
}

extern "C" int qs_hip_decode_device_batch_info_opts(qs_hip_job* const* jobs, int njobs,
                                                    const qs_hip_decode_opts* const* opts, qs_hip_decode_info* per_job,
                                                    size_t* bytes) {
  return guarded([&]() -> int {
    return info_impl(jobs, njobs, opts, nullptr, per_job, bytes, "qs_hip_decode_device_batch_info_opts");
  });
}

extern "C" int qs_hip_decode_device_batch_prepare(qs_hip_job* const* jobs, int njobs, void* d_workspace, size_t bytes,
                                                  void* stream) {
  return guarded([&]() -> int {
    return prepare_impl(jobs, njobs, nullptr, nullptr, d_workspace, bytes, stream, "qs_hip_decode_device_batch_prepare");
  });
}

extern "C" int qs_hip_decode_device_batch_prepare_opts(qs_hip_job* const* jobs, int njobs,
                                                       const qs_hip_decode_opts* const* opts, void* d_workspace,
                                                       size_t bytes, void* stream) {
  return guarded([&]() -> int {
    return prepare_impl(jobs, njobs, opts, nullptr, d_workspace, bytes, stream, "qs_hip_decode_device_batch_prepare_opts");
  });
}

extern "C" int qs_hip_decode_device_batch_info_scaled(qs_hip_job* const* jobs, int njobs,
                                                      const qs_hip_decode_scale_opts* const* opts,
                                                      qs_hip_decode_info* per_job, size_t* bytes) {
  return guarded([&]() -> int {
    return info_impl(jobs, njobs, nullptr, opts, per_job, bytes, "qs_hip_decode_device_batch_info_scaled");
  });
}

extern "C" int qs_hip_decode_device_batch_prepare_scaled(qs_hip_job* const* jobs, int njobs,
                                                         const qs_hip_decode_scale_opts* const* opts, void* d_workspace,
                                                         size_t bytes, void* stream) {
  return guarded([&]() -> int {
    return prepare_impl(jobs, njobs, nullptr, opts, d_workspace, bytes, stream, "qs_hip_decode_device_batch_prepare_scaled");
  });
}

extern "C" int qs_hip_decode_device_batch(qs_hip_job* const* jobs, int njobs, const int32_t* d_stop,
                                          uint8_t* const* d_out, const size_t* out_pitch, void* d_workspace,
                                          size_t bytes, void* stream) {
  return guarded([&]() -> int {
    const char* who = "qs_hip_decode_device_batch";
    std::vector<QsDecJob> D;
    std::vector<QsDecPtrs> P;
    if (!d_out) return qs_fail(QS_HIP_EINVAL, "%s: null d_out", who);
    // the scales the last prepare of this workspace left (full size where there is none)
    std::vector<Mode> modes;
    if (const auto ms = g_scales.find(d_workspace))
      if ((int)ms->size() == njobs) {
        modes.assign((size_t)njobs, Mode());
        for (int i = 0; i < njobs; ++i) modes[(size_t)i].m = (*ms)[(size_t)i];
      }
    std::vector<int> stile_end;
    if (int r = describe_all(jobs, njobs, modes.empty() ? nullptr : modes.data(), d_out, out_pitch, D, &P, nullptr, who,
                             &stile_end))
      return r;
    if (int r = check_workspace(workspace_bytes(njobs), d_workspace, bytes, who)) return r;
    if (int r = device_ok()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int j0 = 0; j0 < njobs; j0 += QS_DEC_CHUNK) {
      QsDecArgs a;
      memset(&a, 0, sizeof a);
      a.jobs = static_cast<const QsDecJob*>(d_workspace) + j0;
      a.d_stop = d_stop;
      a.job0 = j0;
      a.n = std::min(QS_DEC_CHUNK, njobs - j0);
      for (int k = 0; k < a.n; ++k) a.p[k] = P[(size_t)j0 + k];
      const QsDecJob& last = D[(size_t)j0 + a.n - 1];
      qs_launch_decode(a, last.tile0 + last.tiles, s);               // the chunk's full-size jobs, if it has any
      qs_launch_decode_scaled(a, stile_end[(size_t)j0 + a.n - 1], s);   // and its jobs at a reduced size
    }
    HIP_TRY(hipGetLastError());
    return QS_HIP_OK;
  });
}
