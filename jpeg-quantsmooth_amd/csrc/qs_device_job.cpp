// qs_device_job.cpp -- the device-resident job route of the flat C ABI (include/jpegqs_hip.h), for one job
// (qs_hip_device_job_info / qs_hip_device_job_prepare / qs_hip_do_quantsmooth_device) or many
// (qs_hip_device_batch_info / qs_hip_device_batch_prepare / qs_hip_do_quantsmooth_device_batch).  A single job is a
// batch of one.
//
// The whole of the reference's do_quantsmooth (quantsmooth.h:2404-2878) on coefficient arrays that already live in
// device memory, enqueued on ONE caller stream: no allocation, no synchronisation, no event, no other stream, no copy
// from host memory -- so a capture of the call is a linear graph.  Everything the jobs need besides the caller's
// arrays lives in one caller-provided workspace whose layout is a function of the jobs alone (make_batch_plan,
// computed identically by all three calls); the constant blocks and the precheck / fix-up tables are written into it
// by the prepare call.
//
// One image's planes leave most of the chip idle (1080p 4:2:0: 510 + 2 x 128 groups of 64 blocks on 1024 SIMDs), so
// the planes of many jobs share launches, as the host batch route does (qs_batch.cpp):
//   independent jobs (DevPlan::fused, --quality 3/4)  pass A and every pass B as plane-set launches over all of them;
//   coupled YCbCr jobs (JOINT_YUV / UPSAMPLE_UV)      run_coupled's stage order: luma as sets (together with the
//                                                     independent planes), the per-job downsample, chroma as sets with
//                                                     the low-res aux, the per-job upsample and FDCT into coef_up;
//   every other job                                   run_job's component sequence (run_seq) on its own region.
// A set holds at most QS_MAX_PLANES planes; planes of different jobs do not depend on each other, so the cut into
// several launches per pass does not change results.
//
// The job layer (qs_job.cpp) finds a tripped range check by reading a flag on the host and re-runs the job from the
// untouched host input.  Here the input is rewritten in place and the host never waits, so the stop is decided on the
// device, per job (qs_kernels_device.hip): a kernel zeroes the jobs' range-check words; a precheck kernel snapshots the
// components a stop could have to rebuild and runs the reference's range test before any pass of any job; all passes
// then run unconditionally; a fix-up kernel at the end rebuilds the reference's state from the snapshot where a
// component tripped, and writes every job's `stop`.
//
// Workspace of a batch: the range-check words, then each job's own region laid out by make_plan, then the precheck and
// fix-up tables (QsDevBRec).  A single job's workspace is its region alone: make_plan reserves its word and room for
// its own tables in it.
#include "qs_common.h"
#include "qs_stage.h"
#include "qs_device_job.h"

#include <algorithm>

namespace {

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
  size_t off_word = 0, off_pre = 0, off_fix = 0;   // the job's word and tables when it runs alone
  size_t off_llow = 0, off_px = 0, total = 0;
};

int comp_luma(const qs_hip_job* job, int ci) { return !ci || job->colorspace != 3; }   // reference :2639

// JOINT_YUV / UPSAMPLE_UV couple chroma to luma (reference :2447-2453; tied to ncomp == 3 as in qs_job.cpp)
int needs_lowres(const qs_hip_job* job, int flags) {
  return (flags & (QS_JOINT_YUV | QS_UPSAMPLE_UV)) && job->colorspace == 3 && job->ncomp == 3 &&
         job->hsamp[1] == 1 && job->vsamp[1] == 1 && job->hsamp[2] == 1 && job->vsamp[2] == 1;
}

int check_geometry(const qs_hip_job* job, const char* who) {
  if (int r = check_job(job, who)) return r;
  for (int ci = 0; ci < job->ncomp; ++ci) {
    if (job->wblk[ci] <= 0 || job->hblk[ci] <= 0)
      return qs_fail(QS_HIP_EINVAL, "%s: component %d has no blocks", who, ci);
    if (int r = check_sampling(job, ci, who)) return r;
    if ((long long)job->wblk[ci] * job->hblk[ci] > (1ll << 27))
      return qs_fail(QS_HIP_EINVAL, "%s: component %d is too large", who, ci);
  }
  return QS_HIP_OK;
}

int make_plan(const qs_hip_job* job, int flags, int niter, DevPlan& P, const char* who) {
  if (int r = check_geometry(job, who)) return r;
  P = DevPlan();
  niter = niter < 0 ? 0 : niter > 100 ? 100 : niter;       // reference :2455-2456
  P.niter = niter;
  P.need_lowres = needs_lowres(job, flags);
  Layout L;
  P.off_word = L.take(sizeof(uint32_t));
  P.off_pre = L.take(job->ncomp * sizeof(QsDevBRec));        // (at most one precheck and one fix-up record per component)
  P.off_fix = L.take(job->ncomp * sizeof(QsDevBRec));
  if (niter <= 0 && !((flags & QS_UPSAMPLE_UV) && P.need_lowres)) { P.total = L.total; return QS_HIP_OK; }   // reference :2458
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
    C.off_cst = L.take(sizeof(QsConsts));
    if (stop) continue;                                    // dequantise only, :2551-2566
    C.passes = true;
    C.off_status = L.take(sizeof(int32_t));
    C.off_plane = L.take(qs_hip_plane_bytes(job->wblk[ci], job->hblk[ci]));
    C.fuse = !(flags & QS_LOW_QUALITY) && C.iters + C.extra > 1;
    if (C.fuse) C.off_plane2 = L.take(qs_hip_plane_bytes(job->wblk[ci], job->hblk[ci]));
    if (have_yfull) C.upsample = true;                     // :2691-2752
    else if (!ci && P.need_lowres) {                       // :2753-2815
      P.have_llow = 1;
      if (!(job->hsamp[0] == 1 && job->vsamp[0] == 1)) {
        P.llow_own = 1;
        P.off_llow = L.take(qs_hip_plane_bytes(job->wblk[1], job->hblk[1]));
        if (flags & QS_UPSAMPLE_UV) have_yfull = P.have_yfull = 1;
      }
    }
  }
  P.static_stop = stop;
  // replacement chroma only when both chroma components were re-encoded and nothing stopped (qs_job.cpp, :2833-2849);
  // otherwise the job layer discards them, and so are they not computed here
  P.up = P.have_yfull && job->ncomp == 3 && P.c[1].upsample && P.c[2].upsample && !stop;
  if (P.up) P.off_px = L.take(qs_hip_upsample_bytes(job->image_width, job->image_height, job->hsamp[0], job->vsamp[0]));
  else P.c[1].upsample = P.c[2].upsample = false;

  // the snapshot: every component the passes write that a stop at an earlier-or-equal checked component must rebuild
  int first_checked = -1;
  for (int ci = 0; ci < job->ncomp; ++ci) if (P.c[ci].passes && first_checked < 0) first_checked = ci;
  if (first_checked >= 0)
    for (int ci = first_checked; ci < job->ncomp; ++ci)
      if (P.c[ci].modified) {
        P.c[ci].snap = true;
        P.c[ci].off_snap = L.take((size_t)job->wblk[ci] * job->hblk[ci] * 64 * sizeof(int16_t));
      }
  P.total = L.total;
  return QS_HIP_OK;
}

void fill_info(const qs_hip_job* job, const DevPlan& P, qs_hip_device_info* out) {
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
int fix_action(const DevPlan& P, int k, int j) {
  const DevComp& C = P.c[j];
  if (j < k || !C.modified) return QS_DEV_KEEP;
  if (j == k) return QS_DEV_DEQUANT_CLAMP;
  const int extra = (k >= 1 && P.have_yfull) ? 1 : 0;
  return C.iters + extra > 0 ? QS_DEV_DEQUANT : QS_DEV_RESTORE;
}

enum { ROUTE_SEQ = 0, ROUTE_SET = 1, ROUTE_COUPLED = 2 };

// run_coupled's test (qs_batch.cpp: job_couplable) on the plan: three components with passes, niter iterations each
int route_of(int flags, const DevPlan& P) {
  if (!P.todo || P.static_stop) return ROUTE_SEQ;
  if (P.fused) return ROUTE_SET;
  if (!P.need_lowres || (flags & QS_LOW_QUALITY) || P.niter < 1) return ROUTE_SEQ;
  for (int ci = 0; ci < 3; ++ci)
    if (!P.c[ci].passes || P.c[ci].iters != P.niter) return ROUTE_SEQ;
  return ROUTE_COUPLED;
}

struct RecOf { int job, comp; };

struct BatchPlan {
  std::vector<DevPlan> P;
  std::vector<int> route;
  std::vector<size_t> region;               // offset of job i's region in the workspace
  std::vector<QsDevBRec> pre, fix;          // the tables prepare writes
  std::vector<RecOf> pre_of, fix_of;        // ... and whose component each record is
  size_t off_words = 0, off_pre = 0, off_fix = 0, total = 0;
};

uint64_t comp_nvec(const qs_hip_job* job, int ci) { return (uint64_t)job->wblk[ci] * job->hblk[ci] * 8; }

// blk0: a prefix over the workgroups of each chunk's launch (qs_kernels_device.hip: qs_devb_grid)
void assign_blk0(std::vector<QsDevBRec>& recs, const std::vector<RecOf>& of, qs_hip_job* const* jobs, uint64_t vpb) {
  uint64_t w = 0;
  for (size_t r = 0; r < recs.size(); ++r) {
    if (r % QS_DEVB_CHUNK == 0) w = 0;
    recs[r].blk0 = (uint32_t)w;
    w += (comp_nvec(jobs[of[r].job], of[r].comp) + vpb - 1) / vpb;
  }
}

// standalone: the single-job calls (njobs == 1), whose workspace is the job's own region
int make_batch_plan(qs_hip_job* const* jobs, int njobs, int flags, int niter, bool standalone, BatchPlan& B,
                    const char* who) {
  if (!jobs || njobs < 1) return qs_fail(QS_HIP_EINVAL, "%s: %d jobs (at least one)", who, njobs);
  B = BatchPlan();
  B.P.resize((size_t)njobs);
  B.route.resize((size_t)njobs);
  B.region.resize((size_t)njobs);
  Layout L;
  if (!standalone) B.off_words = L.take((size_t)njobs * sizeof(uint32_t));
  for (int i = 0; i < njobs; ++i) {
    if (int r = make_plan(jobs[i], flags, niter, B.P[i], Who(who, i, standalone).s)) return r;
    B.route[i] = route_of(flags, B.P[i]);
    B.region[i] = L.take(B.P[i].total);
  }
  for (int i = 0; i < njobs; ++i) {
    const qs_hip_job* job = jobs[i];
    const DevPlan& P = B.P[i];
    auto rec = [&](int j) {
      QsDevBRec R;
      memset(&R, 0, sizeof R);
      for (int e = 0; e < 64; ++e) R.q[e] = job->quant[j][e];
      for (int k = 0; k < QS_DEV_MAXC; ++k) R.act[k] = k < job->ncomp && P.c[k].passes ? fix_action(P, k, j) : QS_DEV_KEEP;
      R.snap_off = P.c[j].snap ? B.region[i] + P.c[j].off_snap : QS_DEVB_NO_SNAP;
      R.job = i; R.comp = j; R.ncomp = job->ncomp;
      R.check = P.c[j].passes;
      R.static_stop = P.static_stop;
      return R;
    };
    bool writer = true;
    for (int j = 0; j < job->ncomp; ++j) {
      if (P.c[j].snap || P.c[j].passes) { B.pre.push_back(rec(j)); B.pre_of.push_back({i, j}); }
      QsDevBRec R = rec(j);
      bool acts = false;
      for (int k = 0; k < QS_DEV_MAXC; ++k) acts = acts || R.act[k] != QS_DEV_KEEP;
      if (!acts && !(writer && j == job->ncomp - 1)) continue;   // (every job has one record that writes its stop)
      R.stop_writer = writer;
      writer = false;
      B.fix.push_back(R);
      B.fix_of.push_back({i, j});
    }
  }
  assign_blk0(B.pre, B.pre_of, jobs, QS_DEVB_PRE_VPB);
  assign_blk0(B.fix, B.fix_of, jobs, QS_DEVB_FIX_VPB);
  if (standalone) {
    B.off_words = B.P[0].off_word; B.off_pre = B.P[0].off_pre; B.off_fix = B.P[0].off_fix;
  } else {
    B.off_pre = L.take(B.pre.size() * sizeof(QsDevBRec));
    B.off_fix = L.take(B.fix.size() * sizeof(QsDevBRec));
  }
  B.total = L.total;
  return QS_HIP_OK;
}

// job->coef / coef_up present and aligned; `who` names the call (and the job of a batch)
int check_job_arrays(const qs_hip_job* job, const DevPlan& P, const char* who) {
  for (int ci = 0; ci < job->ncomp; ++ci)                  // (the kernels move 16 bytes per lane)
    if (int r = check_array(job->coef[ci], ci, false, who)) return r;
  if (P.up && (!job->coef_up[0] || !job->coef_up[1] || ((reinterpret_cast<uintptr_t>(job->coef_up[0]) |
                                                           reinterpret_cast<uintptr_t>(job->coef_up[1])) & 15)))
    return qs_fail(QS_HIP_EINVAL, "%s: UPSAMPLE_UV replaces the chroma: coef_up[0] and coef_up[1] must be device arrays "
                   "of %d x %d blocks", who, job->wblk[0], job->hblk[0]);
  return QS_HIP_OK;
}

// no two jobs may write the same memory: their coefficient arrays (and replacement chroma) must not overlap
int check_disjoint(qs_hip_job* const* jobs, int njobs, const BatchPlan& B, const char* who) {
  struct Span { uintptr_t lo, hi; int job; };
  std::vector<Span> v;
  for (int i = 0; i < njobs; ++i) {
    const qs_hip_job* job = jobs[i];
    for (int ci = 0; ci < job->ncomp; ++ci) {
      const uintptr_t p = reinterpret_cast<uintptr_t>(job->coef[ci]);
      v.push_back({p, p + comp_nvec(job, ci) * 16, i});
    }
    for (int k = 0; k < 2 && B.P[i].up; ++k) {
      const uintptr_t p = reinterpret_cast<uintptr_t>(job->coef_up[k]);
      v.push_back({p, p + comp_nvec(job, 0) * 16, i});
    }
  }
  std::sort(v.begin(), v.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
  // the spans seen so far that reach past the current start all overlap each other, so (when no two jobs overlapped
  // so far) they belong to one job: comparing with the one that reaches furthest is enough
  uintptr_t far = 0;
  int far_job = -1;
  for (const Span& s : v) {
    if (s.lo < far && far_job != s.job)
      return qs_fail(QS_HIP_EINVAL, "%s: jobs %d and %d have overlapping arrays", who, std::min(far_job, s.job),
                     std::max(far_job, s.job));
    if (s.hi > far) { far = s.hi; far_job = s.job; }
  }
  return QS_HIP_OK;
}

// the constant blocks of the job's region at `ws` (host tables in hc, which must outlive the copies)
int prepare_job(const qs_hip_job* job, int flags, const DevPlan& P, char* ws, QsConsts* hc, hipStream_t s) {
  for (int ci = 0; ci < job->ncomp; ++ci) {
    if (!P.c[ci].modified) continue;
    if (int r = qs_hip_consts_build(&hc[ci], job->quant[ci], flags)) return r;
    HIP_TRY(hipMemcpyAsync(ws + P.c[ci].off_cst, &hc[ci], sizeof(QsConsts), hipMemcpyHostToDevice, s));
  }
  return QS_HIP_OK;
}

// Every pass of a job that runs alone (ROUTE_SEQ), in run_job's component order (qs_job.cpp), on its region at `ws`
int run_seq(qs_hip_job* job, int flags, const DevPlan& P, char* ws, hipStream_t s) {
  auto cst = [&](int ci) { return ws + P.c[ci].off_cst; };
  auto coef = [&](int ci) { return job->coef[ci]; };
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
  return QS_HIP_OK;
}

// The jobs in sets, from the first pass A to the last pass B and the upsampling (qs_batch.cpp: run_coupled's order).
int run_sets(qs_hip_job* const* jobs, int njobs, int flags, const BatchPlan& B, char* ws, hipStream_t s) {
  struct Id { int job, ci; };
  std::vector<unsigned char> cur((size_t)njobs * QS_HIP_MAXC, 0);   // which of its two planes is (job, ci)'s current one
  auto plane_at = [&](const Id& d, int which) {
    const DevComp& C = B.P[d.job].c[d.ci];
    return reinterpret_cast<uint8_t*>(ws + B.region[d.job] + (which ? C.off_plane2 : C.off_plane));
  };
  auto plane_of = [&](const Id& d) { return plane_at(d, cur[(size_t)d.job * QS_HIP_MAXC + d.ci]); };
  auto lowres_of = [&](int i) {
    return B.P[i].llow_own ? reinterpret_cast<uint8_t*>(ws + B.region[i] + B.P[i].off_llow) : plane_of(Id{i, 0});
  };
  const int diag = (flags & QS_DIAGONALS) != 0;
  // one stage over `ids`, cut into launches of at most QS_MAX_PLANES planes; next(d): the pass B writes d's next plane
  // quant: deferred dequantisation (qs_device.h: QS_PLANE_QUANT) -- a first pass A and the first pass B behind it, where
  // nothing reads the coefficients in between.  A job whose range check trips runs on all the same; the fix-up rebuilds
  // its arrays from the snapshot afterwards.
  auto stage = [&](const std::vector<Id>& ids, bool idct, bool joint, int final_clamp, auto next, bool quant = false) {
    for (size_t c0 = 0; c0 < ids.size(); c0 += QS_MAX_PLANES) {
      QsPlaneSet set;
      QsPlaneAux aux;
      memset(&set, 0, sizeof set);
      memset(&aux, 0, sizeof aux);
      const int n = (int)std::min<size_t>(QS_MAX_PLANES, ids.size() - c0);
      int w = 0;
      for (int k = 0; k < n; ++k) {
        const Id& d = ids[c0 + k];
        const qs_hip_job* job = jobs[d.job];
        const DevComp& C = B.P[d.job].c[d.ci];
        set.wave0[k] = w;
        w += (job->wblk[d.ci] * job->hblk[d.ci] + 63) / 64;
        QsPlaneRef& R = set.ref[k];
        R.cst = reinterpret_cast<const QsConsts*>(ws + B.region[d.job] + C.off_cst);
        R.coef = job->coef[d.ci];
        R.plane = plane_of(d);
        R.plane_next = !idct && next(d) ? plane_at(d, !cur[(size_t)d.job * QS_HIP_MAXC + d.ci]) : nullptr;
        R.status = reinterpret_cast<int32_t*>(ws + B.region[d.job] + C.off_status);
        R.wblk = job->wblk[d.ci]; R.hblk = job->hblk[d.ci]; R.pitch = qs_plane_pitch(job->wblk[d.ci]);
        const int rebalance = !(flags & QS_NO_REBALANCE) && (comp_luma(job, d.ci) || !(flags & QS_NO_REBALANCE_UV));
        R.mode = QS_PLANE_REP_TOP | QS_PLANE_REP_BOT | (rebalance ? QS_PLANE_REBALANCE : 0) | (quant ? QS_PLANE_QUANT : 0);
        aux.p[k] = lowres_of(d.job);
      }
      set.n = n;
      for (int k = n; k < QS_MAX_PLANES + 2; ++k) set.wave0[k] = w;
      if (idct) {
        qs_launch_idct_set(set, 1, s);
      } else {
        if (joint) qs_launch_joint_set(set, aux, 0, 0, s);   // JOINT_YUV acts through the low-res luma (reference :2636)
        qs_launch_smooth_set(set, diag, final_clamp, s);
      }
    }
    if (!idct)
      for (const Id& d : ids) if (next(d)) cur[(size_t)d.job * QS_HIP_MAXC + d.ci] ^= 1;
  };

  std::vector<Id> first, chroma;
  for (int i = 0; i < njobs; ++i) {
    if (B.route[i] == ROUTE_SET) for (int ci = 0; ci < jobs[i]->ncomp; ++ci) first.push_back({i, ci});
    if (B.route[i] == ROUTE_COUPLED) { first.push_back({i, 0}); chroma.push_back({i, 1}); chroma.push_back({i, 2}); }
  }
  // niter is one for the batch: every plane in a set runs niter iterations
  int niter = 0;
  for (int i = 0; i < njobs; ++i) if (B.route[i] != ROUTE_SEQ) niter = B.P[i].niter;
  const auto none = [](const Id&) { return false; };

  // independent planes and coupled luma: pass A, then niter passes B; each pass B but an independent plane's last
  // writes the next plane (coupled luma: the refresh the chroma stages read, reference :2495, :2622); the last carries
  // the +-1023 clamp
  const bool defer = niter > 0;
  stage(first, true, false, 0, none, defer);
  for (int it = 0; it < niter; ++it) {
    const bool last = it == niter - 1;
    stage(first, false, false, last, [&](const Id& d) { return !last || B.route[d.job] == ROUTE_COUPLED; }, defer && it == 0);
  }
  if (chroma.empty()) return QS_HIP_OK;
  for (int i = 0; i < njobs; ++i) {                          // image2 (reference :2753-2815)
    if (B.route[i] != ROUTE_COUPLED || !B.P[i].llow_own) continue;
    const qs_hip_job* job = jobs[i];
    if (int r = qs_hip_downsample_plane(plane_of(Id{i, 0}), job->wblk[0], job->hblk[0], lowres_of(i), job->wblk[1],
                                        job->hblk[1], job->hsamp[0], job->vsamp[0], s)) return r;
  }
  // chroma: a job upsampled afterwards needs one more refresh, which its last pass B writes
  const bool joint = (flags & QS_JOINT_YUV) != 0;
  // (with JOINT_YUV the predictor step reads and writes the coefficients between pass A and pass B: eager)
  const bool defer_c = defer && !joint;
  stage(chroma, true, false, 0, none, defer_c);
  for (int it = 0; it < niter; ++it) {
    const bool last = it == niter - 1;
    stage(chroma, false, joint, last, [&](const Id& d) { return !last || B.P[d.job].c[d.ci].upsample; }, defer_c && it == 0);
  }
  for (int i = 0; i < njobs; ++i) {                          // UPSAMPLE_UV (reference :2691-2752)
    if (B.route[i] != ROUTE_COUPLED || !B.P[i].up) continue;
    qs_hip_job* job = jobs[i];
    const int ws0 = job->hsamp[0], hs0 = job->vsamp[0];
    uint8_t* px = reinterpret_cast<uint8_t*>(ws + B.region[i] + B.P[i].off_px);
    for (int ci = 1; ci < 3; ++ci) {
      if (int r = qs_hip_upsample_plane(plane_of(Id{i, ci}), lowres_of(i), job->wblk[ci], plane_of(Id{i, 0}),
                                        job->wblk[0], job->hblk[0], px, job->image_width, job->image_height, ws0, hs0, s))
        return r;
      if (int r = qs_hip_fdct_plane(px, qs_hip_upsample_pitch(job->image_width, ws0), job->coef_up[ci - 1],
                                    job->wblk[0], job->hblk[0], s)) return r;
    }
  }
  return QS_HIP_OK;
}

// the batched precheck or fix-up, one launch per chunk of records
void launch_checks(qs_hip_job* const* jobs, int njobs, const BatchPlan& B, bool fix, char* ws, size_t bytes,
                   int32_t* d_stop, hipStream_t s) {
  const std::vector<RecOf>& of = fix ? B.fix_of : B.pre_of;
  const QsDevBRec* tab = reinterpret_cast<const QsDevBRec*>(ws + (fix ? B.off_fix : B.off_pre));
  for (size_t c0 = 0; c0 < of.size(); c0 += QS_DEVB_CHUNK) {
    QsDevBatchArgs a;
    memset(&a, 0, sizeof a);
    a.rec = tab + c0;
    a.ws = ws;
    a.ws_bytes = bytes;
    a.words = reinterpret_cast<uint32_t*>(ws + B.off_words);
    a.d_stop = d_stop;
    a.njobs = njobs;
    a.n = (int)std::min<size_t>(QS_DEVB_CHUNK, of.size() - c0);
    for (int k = 0; k < a.n; ++k) {
      const RecOf& r = of[c0 + k];
      a.coef[k] = jobs[r.job]->coef[r.comp];
      a.nvec[k] = comp_nvec(jobs[r.job], r.comp);
    }
    if (fix) qs_launch_dev_fixup_batch(a, s);
    else qs_launch_dev_precheck_batch(a, s);
  }
}

// what the run call reports on a job: up_* / out_*samp0 (before enqueueing) and the quant tables set to 1 (after)
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

// ---- the three calls on njobs jobs; standalone: a single-job call (its own layout, no "job <i>" in messages) ----

int info(qs_hip_job* const* jobs, int njobs, int flags, int niter, qs_hip_device_info* per_job, size_t* workspace_bytes,
         bool standalone, const char* who) {
  if (!per_job || !workspace_bytes) return qs_fail(QS_HIP_EINVAL, "%s: null result", who);
  BatchPlan B;
  if (int r = make_batch_plan(jobs, njobs, flags, niter, standalone, B, who)) return r;
  for (int i = 0; i < njobs; ++i) fill_info(jobs[i], B.P[i], &per_job[i]);
  *workspace_bytes = B.total;
  return QS_HIP_OK;
}

int prepare(qs_hip_job* const* jobs, int njobs, int flags, int niter, void* d_workspace, size_t bytes, void* stream,
            bool standalone, const char* who) {
  BatchPlan B;
  if (int r = make_batch_plan(jobs, njobs, flags, niter, standalone, B, who)) return r;
  if (int r = check_workspace(B.total, d_workspace, bytes, who, standalone ? "job" : "batch")) return r;
  if (int r = device_ok()) return r;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(d_workspace);
  std::vector<QsConsts> hc((size_t)njobs * QS_HIP_MAXC);
  for (int i = 0; i < njobs; ++i)
    if (int r = prepare_job(jobs[i], flags, B.P[i], ws + B.region[i], &hc[(size_t)i * QS_HIP_MAXC], s)) return r;
  if (!B.pre.empty())
    HIP_TRY(hipMemcpyAsync(ws + B.off_pre, B.pre.data(), B.pre.size() * sizeof(QsDevBRec), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ws + B.off_fix, B.fix.data(), B.fix.size() * sizeof(QsDevBRec), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));                        // (pageable sources: they must outlive the copies)
  return QS_HIP_OK;
}

int run(qs_hip_job* const* jobs, int njobs, int flags, int niter, void* d_workspace, size_t bytes, int32_t* d_stop,
        void* stream, bool standalone, const char* who) {
  BatchPlan B;
  if (int r = make_batch_plan(jobs, njobs, flags, niter, standalone, B, who)) return r;
  if (!d_stop) return qs_fail(QS_HIP_EINVAL, "%s: null d_stop", who);
  for (int i = 0; i < njobs; ++i)
    if (int r = check_job_arrays(jobs[i], B.P[i], Who(who, i, standalone).s)) return r;
  if (int r = check_disjoint(jobs, njobs, B, who)) return r;
  if (int r = check_workspace(B.total, d_workspace, bytes, who, standalone ? "job" : "batch")) return r;
  if (int r = device_ok()) return r;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(d_workspace);
  for (int i = 0; i < njobs; ++i) report_geometry(jobs[i], B.P[i]);
  qs_launch_dev_clear_words(reinterpret_cast<uint32_t*>(ws + B.off_words), njobs, s);   // 0: nothing tripped
  launch_checks(jobs, njobs, B, false, ws, bytes, d_stop, s);                           // before any pass of any job
  for (int i = 0; i < njobs; ++i)
    if (B.route[i] == ROUTE_SEQ)
      if (int r = run_seq(jobs[i], flags, B.P[i], ws + B.region[i], s)) return r;
  if (int r = run_sets(jobs, njobs, flags, B, ws, s)) return r;
  launch_checks(jobs, njobs, B, true, ws, bytes, d_stop, s);                            // after the last, every stop
  HIP_TRY(hipGetLastError());
  for (int i = 0; i < njobs; ++i) report_quant(jobs[i], B.P[i]);
  return QS_HIP_OK;
}

}  // namespace

// the single-job calls: a batch of one in the job's own workspace layout (the calls do not write the job through
// these pointers where the signature says const)
extern "C" int qs_hip_device_job_info(const qs_hip_job* job, int flags, int niter, qs_hip_device_info* out) {
  qs_hip_job* j = const_cast<qs_hip_job*>(job);
  size_t total;
  return guarded([&] { return info(&j, 1, flags, niter, out, &total, true, "qs_hip_device_job_info"); });
}

extern "C" int qs_hip_device_job_prepare(const qs_hip_job* job, int flags, int niter, void* d_workspace, size_t bytes,
                                         void* stream) {
  qs_hip_job* j = const_cast<qs_hip_job*>(job);
  return guarded([&] { return prepare(&j, 1, flags, niter, d_workspace, bytes, stream, true, "qs_hip_device_job_prepare"); });
}

extern "C" int qs_hip_do_quantsmooth_device(qs_hip_job* job, int flags, int niter, void* d_workspace, size_t bytes,
                                            int32_t* d_stop, void* stream) {
  return guarded([&] {
    return run(&job, 1, flags, niter, d_workspace, bytes, d_stop, stream, true, "qs_hip_do_quantsmooth_device");
  });
}

extern "C" int qs_hip_device_batch_info(qs_hip_job* const* jobs, int njobs, int flags, int niter,
                                        qs_hip_device_info* per_job, size_t* workspace_bytes) {
  return guarded([&] { return info(jobs, njobs, flags, niter, per_job, workspace_bytes, false, "qs_hip_device_batch_info"); });
}

extern "C" int qs_hip_device_batch_prepare(qs_hip_job* const* jobs, int njobs, int flags, int niter, void* d_workspace,
                                           size_t bytes, void* stream) {
  return guarded([&] {
    return prepare(jobs, njobs, flags, niter, d_workspace, bytes, stream, false, "qs_hip_device_batch_prepare");
  });
}

extern "C" int qs_hip_do_quantsmooth_device_batch(qs_hip_job* const* jobs, int njobs, int flags, int niter,
                                                  void* d_workspace, size_t bytes, int32_t* d_stop, void* stream) {
  return guarded([&] {
    return run(jobs, njobs, flags, niter, d_workspace, bytes, d_stop, stream, false, "qs_hip_do_quantsmooth_device_batch");
  });
}
