// qs_device_batch.cpp -- the batch form of the device-resident job route (include/jpegqs_hip.h):
// qs_hip_device_batch_info / qs_hip_device_batch_prepare / qs_hip_do_quantsmooth_device_batch.
//
// Many jobs on device arrays, enqueued on ONE caller stream with the single-job call's promises (no allocation, no
// synchronisation, no event, no other stream, no copy from host memory: a capture is a linear graph).  One image's
// planes leave most of the chip idle (1080p 4:2:0: 510 + 2 x 128 groups of 64 blocks on 1024 SIMDs), so the planes of
// many jobs share launches, as the host batch route does (qs_batch.cpp):
//   independent jobs (DevPlan::fused, --quality 3/4)  pass A and every pass B as plane-set launches over all of them;
//   coupled YCbCr jobs (JOINT_YUV / UPSAMPLE_UV)      run_coupled's stage order: luma as sets (together with the
//                                                     independent planes), the per-job downsample, chroma as sets with
//                                                     the low-res aux, the per-job upsample and FDCT into coef_up;
//   every other job                                   the single-job sequence (run_device) on its own region.
// A set holds at most QS_MAX_PLANES planes; planes of different jobs do not depend on each other, so the cut into
// several launches per pass does not change results.  The range-check stop of the jobs in sets is decided by the batched
// precheck / fix-up kernels (qs_kernels_device.hip): one word and one d_stop entry per job, independent of the others.
//
// Workspace: the batch's range-check words, then each job's own region laid out by make_plan, then the precheck and
// fix-up tables (QsDevBRec) the prepare call writes.  The layout is a function of the jobs' geometry, tables, flags and
// niter alone (make_batch_plan, computed identically by all three calls).
#include "qs_device_plan.h"

#include <algorithm>
#include <new>
#include <vector>

namespace {

using namespace qsdev;

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
  bool any_set = false;
};

struct Who {                                // "<call>: job <i>", the prefix of a job's error messages
  char s[96];
  Who(const char* who, int i) { snprintf(s, sizeof s, "%s: job %d", who, i); }
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

int make_batch_plan(qs_hip_job* const* jobs, int njobs, int flags, int niter, BatchPlan& B, const char* who) {
  if (!jobs || njobs < 1) return qs_fail(QS_HIP_EINVAL, "%s: %d jobs (at least one)", who, njobs);
  B = BatchPlan();
  B.P.resize((size_t)njobs);
  B.route.resize((size_t)njobs);
  B.region.resize((size_t)njobs);
  size_t off = 0;
  auto take = [&](size_t n) { const size_t o = off; off += align_up(n); return o; };
  B.off_words = take((size_t)njobs * sizeof(uint32_t));
  for (int i = 0; i < njobs; ++i) {
    if (!jobs[i]) return qs_fail(QS_HIP_EINVAL, "%s: job %d is null", who, i);
    if (int r = make_plan(jobs[i], flags, niter, B.P[i], Who(who, i).s)) return r;
    B.route[i] = route_of(flags, B.P[i]);
    B.any_set = B.any_set || B.route[i] != ROUTE_SEQ;
    B.region[i] = take(B.P[i].total);
  }
  for (int i = 0; i < njobs; ++i) {
    if (B.route[i] == ROUTE_SEQ) continue;
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
  B.off_pre = take(B.pre.size() * sizeof(QsDevBRec));
  B.off_fix = take(B.fix.size() * sizeof(QsDevBRec));
  B.total = off;
  return QS_HIP_OK;
}

int check_workspace(const BatchPlan& B, const void* d_workspace, size_t bytes, const char* who) {
  if (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 255) || bytes < B.total)
    return qs_fail(QS_HIP_EINVAL, "%s: workspace of %zu bytes (256-byte aligned), the batch needs %zu", who, bytes, B.total);
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
  auto stage = [&](const std::vector<Id>& ids, bool idct, bool joint, int final_clamp, auto next) {
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
        R.mode = QS_PLANE_REP_TOP | QS_PLANE_REP_BOT | (rebalance ? QS_PLANE_REBALANCE : 0);
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
  stage(first, true, false, 0, none);
  for (int it = 0; it < niter; ++it) {
    const bool last = it == niter - 1;
    stage(first, false, false, last, [&](const Id& d) { return !last || B.route[d.job] == ROUTE_COUPLED; });
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
  stage(chroma, true, false, 0, none);
  for (int it = 0; it < niter; ++it) {
    const bool last = it == niter - 1;
    stage(chroma, false, joint, last, [&](const Id& d) { return !last || B.P[d.job].c[d.ci].upsample; });
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

}  // namespace

extern "C" int qs_hip_device_batch_info(qs_hip_job* const* jobs, int njobs, int flags, int niter,
                                        qs_hip_device_info* per_job, size_t* workspace_bytes) {
  try {
    static const char* who = "qs_hip_device_batch_info";
    if (!per_job || !workspace_bytes) return qs_fail(QS_HIP_EINVAL, "%s: null result", who);
    BatchPlan B;
    if (int r = make_batch_plan(jobs, njobs, flags, niter, B, who)) return r;
    for (int i = 0; i < njobs; ++i) fill_info(jobs[i], B.P[i], &per_job[i]);
    *workspace_bytes = B.total;
    return QS_HIP_OK;
  } catch (...) {
    return qs_fail(QS_HIP_ENOMEM, "out of host memory");
  }
}

extern "C" int qs_hip_device_batch_prepare(qs_hip_job* const* jobs, int njobs, int flags, int niter, void* d_workspace,
                                           size_t bytes, void* stream) {
  try {
    static const char* who = "qs_hip_device_batch_prepare";
    BatchPlan B;
    if (int r = make_batch_plan(jobs, njobs, flags, niter, B, who)) return r;
    if (int r = check_workspace(B, d_workspace, bytes, who)) return r;
    if (int r = device_ok()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(d_workspace);
    std::vector<QsConsts> hc((size_t)njobs * QS_HIP_MAXC);
    for (int i = 0; i < njobs; ++i)
      if (int r = prepare_job(jobs[i], flags, B.P[i], ws + B.region[i], &hc[(size_t)i * QS_HIP_MAXC], s)) return r;
    if (!B.pre.empty())
      HIP_TRY(hipMemcpyAsync(ws + B.off_pre, B.pre.data(), B.pre.size() * sizeof(QsDevBRec), hipMemcpyHostToDevice, s));
    if (!B.fix.empty())
      HIP_TRY(hipMemcpyAsync(ws + B.off_fix, B.fix.data(), B.fix.size() * sizeof(QsDevBRec), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                      // (pageable sources: they must outlive the copies)
    return QS_HIP_OK;
  } catch (const std::bad_alloc&) {
    return qs_fail(QS_HIP_ENOMEM, "out of host memory");
  } catch (...) {
    return qs_fail(QS_HIP_ENODEV, "unexpected internal error");
  }
}

extern "C" int qs_hip_do_quantsmooth_device_batch(qs_hip_job* const* jobs, int njobs, int flags, int niter,
                                                  void* d_workspace, size_t bytes, int32_t* d_stop, void* stream) {
  try {
    static const char* who = "qs_hip_do_quantsmooth_device_batch";
    BatchPlan B;
    if (int r = make_batch_plan(jobs, njobs, flags, niter, B, who)) return r;
    if (!d_stop) return qs_fail(QS_HIP_EINVAL, "%s: null stop array", who);
    for (int i = 0; i < njobs; ++i)
      if (int r = check_job_arrays(jobs[i], B.P[i], Who(who, i).s)) return r;
    if (int r = check_disjoint(jobs, njobs, B, who)) return r;
    if (int r = check_workspace(B, d_workspace, bytes, who)) return r;
    if (int r = device_ok()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(d_workspace);
    for (int i = 0; i < njobs; ++i) report_geometry(jobs[i], B.P[i]);
    for (int i = 0; i < njobs; ++i)                        // the single-job sequence, each on its own region and word
      if (B.route[i] == ROUTE_SEQ)
        if (int r = enqueue_job(jobs[i], flags, B.P[i], ws + B.region[i], d_stop + i, s)) return r;
    if (B.any_set) {
      qs_launch_dev_clear_words(reinterpret_cast<uint32_t*>(ws + B.off_words), njobs, s);   // 0: nothing tripped
      launch_checks(jobs, njobs, B, false, ws, bytes, d_stop, s);
      if (int r = run_sets(jobs, njobs, flags, B, ws, s)) return r;
      launch_checks(jobs, njobs, B, true, ws, bytes, d_stop, s);
    }
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < njobs; ++i) report_quant(jobs[i], B.P[i]);
    return QS_HIP_OK;
  } catch (const std::bad_alloc&) {
    return qs_fail(QS_HIP_ENOMEM, "out of host memory");
  } catch (...) {
    return qs_fail(QS_HIP_ENODEV, "unexpected internal error");
  }
}
