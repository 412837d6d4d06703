// qs_device_plan.h -- the plan of one device-resident job (workspace layout, route, stop actions), shared by the
// single-job route (qs_device_job.cpp) and the batch route (qs_device_batch.cpp).  Host side, not part of the ABI.
#pragma once
#include "qs_common.h"
#include "qs_device_job.h"

namespace qsdev {


inline size_t align_up(size_t n) { return (n + 255) & ~(size_t)255; }

struct DevComp {
  bool modified = false;      // the plan writes this component's coefficients
  bool passes = false;        // ... through pass A / pass B (else: dequantise only, reference :2551-2566)
  bool fuse = false;          // pass B writes the next iteration's plane into a second plane
  bool upsample = false;      // UPSAMPLE_UV: re-encoded at luma resolution into coef_up[ci - 1]
  int iters = 0, extra = 0;
  size_t off_cst = 0, off_status = 0, off_plane = 0, off_plane2 = 0, off_snap = 0;
  bool snap = false;
};

// The job layer's own decisions (qs_job.cpp: run_job, job_fusable) for a job that trips no range check, as a
// function of geometry, quant tables, flags and niter -- plus the workspace layout they need.
struct DevPlan {
  int todo = 0;               // 0: the reference's early out (:2458), nothing is done, stop = 0
  int niter = 0;
  int need_lowres = 0;        // reference :2447-2453
  int fused = 0;              // independent components: the plane-set launches
  int static_stop = 0;        // a table value >= 0x800 (reference :2504)
  int have_llow = 0, llow_own = 0, have_yfull = 0, up = 0;
  DevComp c[QS_HIP_MAXC];
  size_t off_word = 0, off_llow = 0, off_px = 0, total = 0;
};

inline int comp_luma(const qs_hip_job* job, int ci) { return !ci || job->colorspace != 3; }   // reference :2639

// JOINT_YUV / UPSAMPLE_UV couple chroma to luma (reference :2447-2453; tied to ncomp == 3 as in qs_job.cpp)
inline int needs_lowres(const qs_hip_job* job, int flags) {
  return (flags & (QS_JOINT_YUV | QS_UPSAMPLE_UV)) && job->colorspace == 3 && job->ncomp == 3 &&
         job->hsamp[1] == 1 && job->vsamp[1] == 1 && job->hsamp[2] == 1 && job->vsamp[2] == 1;
}

inline int check_geometry(const qs_hip_job* job, const char* who) {
  if (!job || job->ncomp < 1 || job->ncomp > QS_HIP_MAXC) return qs_fail(QS_HIP_EINVAL, "%s: bad job", who);
  for (int ci = 0; ci < job->ncomp; ++ci) {
    if (job->wblk[ci] <= 0 || job->hblk[ci] <= 0)
      return qs_fail(QS_HIP_EINVAL, "%s: component %d has no blocks", who, ci);
    if (job->hsamp[ci] < 1 || job->hsamp[ci] > 4 || job->vsamp[ci] < 1 || job->vsamp[ci] > 4)
      return qs_fail(QS_HIP_EINVAL, "%s: component %d has sampling factors %dx%d", who, ci, job->hsamp[ci], job->vsamp[ci]);
    if ((long long)job->wblk[ci] * job->hblk[ci] > (1ll << 27))
      return qs_fail(QS_HIP_EINVAL, "%s: component %d is too large", who, ci);
  }
  return QS_HIP_OK;
}

inline int make_plan(const qs_hip_job* job, int flags, int niter, DevPlan& P, const char* who) {
  if (int r = check_geometry(job, who)) return r;
  P = DevPlan();
  niter = niter < 0 ? 0 : niter > 100 ? 100 : niter;       // reference :2455-2456
  P.niter = niter;
  P.need_lowres = needs_lowres(job, flags);
  size_t off = 0;
  auto take = [&](size_t n) { const size_t o = off; off += align_up(n); return o; };
  P.off_word = take(sizeof(uint32_t));
  if (niter <= 0 && !((flags & QS_UPSAMPLE_UV) && P.need_lowres)) { P.total = off; return QS_HIP_OK; }   // reference :2458
  P.todo = 1;

  // independent components and ordinary tables (qs_job.cpp: job_fusable): one plane-set launch per pass
  P.fused = !(flags & QS_LOW_QUALITY) && !P.need_lowres;
  for (int ci = 0; ci < job->ncomp && P.fused; ++ci) {
    int acc = 0;
    for (int i = 0; i < 64; ++i) acc |= job->quant[ci][i];
    P.fused = job->has_quant[ci] && acc > 1 && acc < 0x800;
  }

  int stop = 0, have_yfull = 0;
  for (int ci = 0; ci < job->ncomp; ++ci) {               // run_job's component loop, no range check tripping
    DevComp& C = P.c[ci];
    if (!job->has_quant[ci]) continue;                     // reference :2493
    C.extra = (have_yfull || (!ci && P.need_lowres)) ? 1 : 0;   // :2495
    int acc = 0;
    for (int i = 0; i < 64; ++i) acc |= job->quant[ci][i];
    C.iters = acc <= 1 ? 0 : niter;                        // :2501
    if (acc >= 0x800) stop = 1;                            // :2504
    if (C.iters + C.extra == 0) continue;                  // :2542
    C.modified = true;
    C.off_cst = take(sizeof(QsConsts));
    if (stop) continue;                                    // dequantise only, :2551-2566
    C.passes = true;
    C.off_status = take(sizeof(int32_t));
    C.off_plane = take(qs_hip_plane_bytes(job->wblk[ci], job->hblk[ci]));
    C.fuse = !(flags & QS_LOW_QUALITY) && C.iters + C.extra > 1;
    if (C.fuse) C.off_plane2 = take(qs_hip_plane_bytes(job->wblk[ci], job->hblk[ci]));
    if (have_yfull) C.upsample = true;                     // :2691-2752
    else if (!ci && P.need_lowres) {                       // :2753-2815
      P.have_llow = 1;
      if (!(job->hsamp[0] == 1 && job->vsamp[0] == 1)) {
        P.llow_own = 1;
        P.off_llow = take(qs_hip_plane_bytes(job->wblk[1], job->hblk[1]));
        if (flags & QS_UPSAMPLE_UV) have_yfull = P.have_yfull = 1;
      }
    }
  }
  P.static_stop = stop;
  // replacement chroma only when both chroma components were re-encoded and nothing stopped (qs_job.cpp, :2833-2849);
  // otherwise the job layer discards them, and so are they not computed here
  P.up = P.have_yfull && job->ncomp == 3 && P.c[1].upsample && P.c[2].upsample && !stop;
  if (P.up) P.off_px = take(qs_hip_upsample_bytes(job->image_width, job->image_height, job->hsamp[0], job->vsamp[0]));
  else P.c[1].upsample = P.c[2].upsample = false;

  // the snapshot: every component the passes write that a stop at an earlier-or-equal checked component must rebuild
  int first_checked = -1;
  for (int ci = 0; ci < job->ncomp; ++ci) if (P.c[ci].passes && first_checked < 0) first_checked = ci;
  if (first_checked >= 0)
    for (int ci = first_checked; ci < job->ncomp; ++ci)
      if (P.c[ci].modified) {
        P.c[ci].snap = true;
        P.c[ci].off_snap = take((size_t)job->wblk[ci] * job->hblk[ci] * 64 * sizeof(int16_t));
      }
  P.total = off;
  return QS_HIP_OK;
}

inline void fill_info(const qs_hip_job* job, const DevPlan& P, qs_hip_device_info* out) {
  out->workspace_bytes = P.total;
  out->up_wblk = P.up ? job->wblk[0] : 0;
  out->up_hblk = P.up ? job->hblk[0] : 0;
  out->out_hsamp0 = P.up ? 1 : job->hsamp[0];
  out->out_vsamp0 = P.up ? 1 : job->vsamp[0];
  out->static_stop = P.static_stop;
}

// What the reference leaves in component j when its range check trips first at component k (k < the static stop;
// a component checked by the precheck has passes, so it lies before it):
//   j <  k   its full result;                        j == k  int16(coef * q), then the clamp (:2598, 2610, 2668-2689);
//   j >  k   stop is set, so it is dequantised only when iters + extra > 0 (:2542, 2551-2566), where extra now
//            comes from the full-resolution luma plane alone -- which exists only when luma itself finished (k >= 1).
inline int fix_action(const DevPlan& P, int k, int j) {
  const DevComp& C = P.c[j];
  if (j < k || !C.modified) return QS_DEV_KEEP;
  if (j == k) return QS_DEV_DEQUANT_CLAMP;
  const int extra = (k >= 1 && P.have_yfull) ? 1 : 0;
  return C.iters + extra > 0 ? QS_DEV_DEQUANT : QS_DEV_RESTORE;
}

// the single-job sequence, shared with the batch route (qs_device_job.cpp)
int device_ok();
// job->coef / coef_up present and aligned; `who` names the call (and the job of a batch)
int check_job_arrays(const qs_hip_job* job, const DevPlan& P, const char* who);
// the constant blocks of the job's region at `ws` (host tables in hc, which must outlive the copies)
int prepare_job(const qs_hip_job* job, int flags, const DevPlan& P, char* ws, QsConsts* hc, hipStream_t s);
// the range-check word, precheck, every pass and the fix-up of one job on its own region at `ws`
int run_device(qs_hip_job* job, int flags, const DevPlan& P, char* ws, int32_t* d_stop, hipStream_t s);
// what the run call reports on the job: up_* / out_*samp0 (before enqueueing) and the quant tables set to 1 (after)
void report_geometry(qs_hip_job* job, const DevPlan& P);
void report_quant(qs_hip_job* job, const DevPlan& P);
// the whole job: the early out, or run_device
int enqueue_job(qs_hip_job* job, int flags, const DevPlan& P, char* ws, int32_t* d_stop, hipStream_t s);

}  // namespace qsdev
