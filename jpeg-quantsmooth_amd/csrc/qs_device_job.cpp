// qs_device_job.cpp -- the device-resident job route of the flat C ABI (include/jpegqs_hip.h):
// qs_hip_device_job_info / qs_hip_device_job_prepare / qs_hip_do_quantsmooth_device.
//
// The whole of the reference's do_quantsmooth (quantsmooth.h:2404-2878) on coefficient arrays that already live in
// device memory, enqueued on ONE caller stream: no allocation, no synchronisation, no event, no other stream, no copy
// from host memory -- so a capture of the call is a linear graph.  Everything the job needs besides the caller's
// arrays lives in one caller-provided workspace whose layout is a function of the job alone (DevPlan below, computed
// identically by all three calls); the per-component constant blocks are written into it by the prepare call.
//
// The job layer (qs_job.cpp) finds a tripped range check by reading a flag on the host and re-runs the job from the
// untouched host input.  Here the input is rewritten in place and the host never waits, so the stop is decided on the
// device: a precheck kernel snapshots the components a stop could have to rebuild and runs the reference's range
// test before any pass; all passes then run unconditionally; a fix-up kernel at the end rebuilds the reference's
// state from the snapshot if (and only if) a component tripped, and writes `stop` (qs_kernels_device.hip).
#include "qs_device_plan.h"

#include <new>
#include <vector>

namespace qsdev {

int device_ok() {
  if (qs_hip_device_count() <= 0)
    return qs_fail(QS_HIP_ENODEV, "no HIP device available (this library has no CPU fallback)");
  return QS_HIP_OK;
}

int run_device(qs_hip_job* job, int flags, const DevPlan& P, char* ws, int32_t* d_stop, hipStream_t s) {
  uint32_t* word = reinterpret_cast<uint32_t*>(ws + P.off_word);
  const int niter = P.niter;
  auto cst = [&](int ci) { return ws + P.c[ci].off_cst; };
  auto coef = [&](int ci) { return job->coef[ci]; };

  QsDevJobArgs args;
  memset(&args, 0, sizeof args);
  args.n = job->ncomp;
  args.static_stop = P.static_stop;
  bool any_check = false;
  for (int j = 0; j < job->ncomp; ++j) {
    QsDevComp& D = args.c[j];
    D.coef = coef(j);
    D.snap = P.c[j].snap ? reinterpret_cast<int16_t*>(ws + P.c[j].off_snap) : nullptr;
    D.nvec = (uint64_t)job->wblk[j] * job->hblk[j] * 8;
    D.check = P.c[j].passes;
    any_check = any_check || D.check;
    for (int k = 0; k < QS_DEV_MAXC; ++k) D.act[k] = k < job->ncomp && P.c[k].passes ? fix_action(P, k, j) : QS_DEV_KEEP;
    if (job->has_quant[j]) for (int i = 0; i < 64; ++i) D.q[i] = job->quant[j][i];
  }
  HIP_TRY(hipMemsetAsync(word, 0, sizeof(uint32_t), s));        // 0: nothing tripped (qs_kernels_device.hip)
  if (any_check) qs_launch_dev_precheck(args, word, s);

  if (P.fused) {
    // every component runs niter iterations on its own planes: pass A once, then pass B per iteration, each over the
    // whole job in one launch; every pass B but the last writes the next iteration's planes (qs_fused.cpp)
    qs_hip_plane_ref refs[QS_HIP_MAXC];
    uint8_t* a[QS_HIP_MAXC];
    uint8_t* b[QS_HIP_MAXC];
    uint8_t* nxt[QS_HIP_MAXC];
    const int n = job->ncomp;
    for (int ci = 0; ci < n; ++ci) {
      const DevComp& C = P.c[ci];
      a[ci] = reinterpret_cast<uint8_t*>(ws + C.off_plane);
      b[ci] = C.fuse ? reinterpret_cast<uint8_t*>(ws + C.off_plane2) : nullptr;
      refs[ci] = qs_hip_plane_ref{cst(ci), coef(ci), a[ci], reinterpret_cast<int32_t*>(ws + C.off_status),
                                  job->wblk[ci], job->hblk[ci], comp_luma(job, ci), 0};
    }
    if (int r = qs_hip_idct_planes(refs, n, 1, s)) return r;
    const int pf = flags & (QS_DIAGONALS | QS_NO_REBALANCE | QS_NO_REBALANCE_UV);
    for (int it = 0; it < niter; ++it) {
      const bool last = it == niter - 1;
      for (int ci = 0; ci < n; ++ci) {
        refs[ci].d_plane = (it & 1) ? b[ci] : a[ci];
        nxt[ci] = last ? nullptr : (it & 1) ? a[ci] : b[ci];
      }
      if (int r = qs_hip_smooth_planes_next(refs, last ? nullptr : nxt, n, pf, last, s)) return r;
    }
  } else {
    // run_job's component order on the one stream (qs_job.cpp)
    uint8_t* llow = nullptr;
    uint8_t* yfull = nullptr;
    for (int ci = 0; ci < job->ncomp; ++ci) {
      const DevComp& C = P.c[ci];
      if (!C.modified) continue;
      const int wb = job->wblk[ci], hb = job->hblk[ci];
      if (!C.passes) {
        if (int r = qs_hip_dequant_plane(cst(ci), coef(ci), wb, hb, s)) return r;
        continue;
      }
      const int luma = comp_luma(job, ci);
      const int rebalance = !(flags & QS_NO_REBALANCE) && (luma || !(flags & QS_NO_REBALANCE_UV));   // :1567-1568
      const bool joint = llow && (flags & QS_JOINT_YUV);     // :2636
      const int pf = flags & (QS_DIAGONALS | QS_NO_REBALANCE | QS_NO_REBALANCE_UV);
      int32_t* status = reinterpret_cast<int32_t*>(ws + C.off_status);
      uint8_t* plane = reinterpret_cast<uint8_t*>(ws + C.off_plane);
      uint8_t* plane2 = C.fuse ? reinterpret_cast<uint8_t*>(ws + C.off_plane2) : nullptr;
      const int iters = C.iters, extra = C.extra;
      bool clamped = false, have_next = false;
      for (int it = 0; it < iters + extra; ++it) {
        if (!have_next)
          if (int r = qs_hip_idct_plane(cst(ci), coef(ci), plane, wb, hb, it == 0, 1, 1, status, s)) return r;
        have_next = false;
        if (it == iters) break;                            // refresh-only pass, :2622
        const int last = (it == iters - 1) && !extra;      // the clamp follows the refresh pass otherwise (:2668-2689)
        if (flags & QS_LOW_QUALITY) {                      // :924-938
          if (joint) {
            if (int r = qs_hip_joint_plane(cst(ci), coef(ci), plane, llow, wb, hb, rebalance, last, s)) return r;
          } else if (int r = qs_hip_lowq_plane(cst(ci), coef(ci), plane, wb, hb, rebalance, last, s)) return r;
        } else {
          if (joint)
            if (int r = qs_hip_joint_plane(cst(ci), coef(ci), plane, llow, wb, hb, 0, 0, s)) return r;
          if (C.fuse && it + 1 < iters + extra) {
            const int clamp_now = it == iters - 1;
            if (int r = qs_hip_smooth_plane_next(cst(ci), coef(ci), plane, plane2, wb, hb, pf, luma, clamp_now, 1, 1, s))
              return r;
            uint8_t* t = plane; plane = plane2; plane2 = t;
            have_next = true;
            if (clamp_now) clamped = true;
          } else if (int r = qs_hip_smooth_plane(cst(ci), coef(ci), plane, wb, hb, pf, luma, last, s)) return r;
        }
        if (last) clamped = true;
      }
      if (!clamped)
        if (int r = qs_hip_clamp_plane(coef(ci), wb, hb, s)) return r;

      if (C.upsample) {                                    // :2691-2752
        const int ws0 = job->hsamp[0], hs0 = job->vsamp[0];
        uint8_t* px = reinterpret_cast<uint8_t*>(ws + P.off_px);
        if (int r = qs_hip_upsample_plane(plane, llow, wb, yfull, job->wblk[0], job->hblk[0], px,
                                          job->image_width, job->image_height, ws0, hs0, s)) return r;
        if (int r = qs_hip_fdct_plane(px, qs_hip_upsample_pitch(job->image_width, ws0), job->coef_up[ci - 1],
                                      job->wblk[0], job->hblk[0], s)) return r;
      } else if (!ci && P.need_lowres) {                   // :2753-2815
        if (!P.llow_own) llow = plane;                     // image2 = image
        else {
          llow = reinterpret_cast<uint8_t*>(ws + P.off_llow);
          if (int r = qs_hip_downsample_plane(plane, wb, hb, llow, job->wblk[1], job->hblk[1],
                                              job->hsamp[0], job->vsamp[0], s)) return r;
          if (P.have_yfull) yfull = plane;                 // image1 = image
        }
      }
    }
  }
  qs_launch_dev_fixup(args, word, d_stop, s);
  HIP_TRY(hipGetLastError());
  return QS_HIP_OK;
}

int check_job_arrays(const qs_hip_job* job, const DevPlan& P, const char* who) {
  for (int ci = 0; ci < job->ncomp; ++ci)                  // (the kernels move 16 bytes per lane)
    if (!job->coef[ci] || (reinterpret_cast<uintptr_t>(job->coef[ci]) & 15))
      return qs_fail(QS_HIP_EINVAL, "%s: component %d has no data or is not 16-byte aligned", who, ci);
  if (P.up && (!job->coef_up[0] || !job->coef_up[1] || ((reinterpret_cast<uintptr_t>(job->coef_up[0]) |
                                                           reinterpret_cast<uintptr_t>(job->coef_up[1])) & 15)))
    return qs_fail(QS_HIP_EINVAL, "%s: UPSAMPLE_UV replaces the chroma: coef_up[0] and coef_up[1] must be device arrays "
                   "of %d x %d blocks", who, job->wblk[0], job->hblk[0]);
  return QS_HIP_OK;
}

int prepare_job(const qs_hip_job* job, int flags, const DevPlan& P, char* ws, QsConsts* hc, hipStream_t s) {
  for (int ci = 0; ci < job->ncomp; ++ci) {
    if (!P.c[ci].modified) continue;
    if (int r = qs_hip_consts_build(&hc[ci], job->quant[ci], flags)) return r;
    HIP_TRY(hipMemcpyAsync(ws + P.c[ci].off_cst, &hc[ci], sizeof(QsConsts), hipMemcpyHostToDevice, s));
  }
  return QS_HIP_OK;
}

void report_geometry(qs_hip_job* job, const DevPlan& P) {
  qs_hip_device_info info;
  fill_info(job, P, &info);
  job->up_wblk = info.up_wblk; job->up_hblk = info.up_hblk;
  job->out_hsamp0 = info.out_hsamp0; job->out_vsamp0 = info.out_vsamp0;
}

void report_quant(qs_hip_job* job, const DevPlan& P) {    // reference :2851-2859 (not after the early out, :2458)
  if (!P.todo) return;
  for (int ci = 0; ci < job->ncomp; ++ci)
    if (job->has_quant[ci]) for (int i = 0; i < 64; ++i) job->quant[ci][i] = 1;
}

int enqueue_job(qs_hip_job* job, int flags, const DevPlan& P, char* ws, int32_t* d_stop, hipStream_t s) {
  if (!P.todo) {                                           // reference :2458: nothing happens, stop = 0
    HIP_TRY(hipMemsetAsync(d_stop, 0, sizeof(int32_t), s));
    return QS_HIP_OK;
  }
  return run_device(job, flags, P, ws, d_stop, s);
}

}  // namespace qsdev

using namespace qsdev;

extern "C" int qs_hip_device_job_info(const qs_hip_job* job, int flags, int niter, qs_hip_device_info* out) {
  try {
    if (!out) return qs_fail(QS_HIP_EINVAL, "qs_hip_device_job_info: null result");
    DevPlan P;
    if (int r = make_plan(job, flags, niter, P, "qs_hip_device_job_info")) return r;
    fill_info(job, P, out);
    return QS_HIP_OK;
  } catch (...) {
    return qs_fail(QS_HIP_ENOMEM, "out of host memory");
  }
}

extern "C" int qs_hip_device_job_prepare(const qs_hip_job* job, int flags, int niter, void* d_workspace, size_t bytes,
                                         void* stream) {
  try {
    DevPlan P;
    if (int r = make_plan(job, flags, niter, P, "qs_hip_device_job_prepare")) return r;
    if (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 255) || bytes < P.total)
      return qs_fail(QS_HIP_EINVAL, "qs_hip_device_job_prepare: workspace of %zu bytes, the job needs %zu", bytes, P.total);
    if (int r = device_ok()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<QsConsts> hc(QS_HIP_MAXC);
    if (int r = prepare_job(job, flags, P, static_cast<char*>(d_workspace), hc.data(), s)) return r;
    HIP_TRY(hipStreamSynchronize(s));                      // (pageable source: it must outlive the copies)
    return QS_HIP_OK;
  } catch (const std::bad_alloc&) {
    return qs_fail(QS_HIP_ENOMEM, "out of host memory");
  } catch (...) {
    return qs_fail(QS_HIP_ENODEV, "unexpected internal error");
  }
}

extern "C" int qs_hip_do_quantsmooth_device(qs_hip_job* job, int flags, int niter, void* d_workspace, size_t bytes,
                                            int32_t* d_stop, void* stream) {
  try {
    static const char* who = "qs_hip_do_quantsmooth_device";
    DevPlan P;
    if (int r = make_plan(job, flags, niter, P, who)) return r;
    if (!d_stop) return qs_fail(QS_HIP_EINVAL, "%s: null stop word", who);
    if (int r = check_job_arrays(job, P, who)) return r;
    if (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 255) || bytes < P.total)
      return qs_fail(QS_HIP_EINVAL, "%s: workspace of %zu bytes (256-byte aligned), the job needs %zu", who, bytes, P.total);
    if (int r = device_ok()) return r;
    report_geometry(job, P);
    if (int r = enqueue_job(job, flags, P, static_cast<char*>(d_workspace), d_stop, static_cast<hipStream_t>(stream)))
      return r;
    report_quant(job, P);
    return QS_HIP_OK;
  } catch (const std::bad_alloc&) {
    return qs_fail(QS_HIP_ENOMEM, "out of host memory");
  } catch (...) {
    return qs_fail(QS_HIP_ENODEV, "unexpected internal error");
  }
}
