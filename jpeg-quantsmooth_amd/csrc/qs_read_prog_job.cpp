// qs_read_prog_job.cpp -- the progressive route of the device scan reader of the flat C ABI (include/jpegqs_hip.h):
// qs_hip_read_prog_device_batch_info / _prepare / qs_hip_read_prog_device_batch.  The bytes of a whole progressive
// Huffman file (SOF2) in device memory into the coefficient arrays of qs_hip_job records: what libjpeg 9's
// jpeg_read_coefficients leaves there (qs_kernels_read_prog.hip, one lane per restart interval of one scan, one decode
// launch per level of the script).  DESIGN.md section 18.
//
// A job with n scans becomes n (job, scan) pairs.  Workspace: QrJob[pairs] (the scan's own geometry, interval, code tables
// and marker arrays: what the marker kernels of the interval route work on), QrpScan[pairs], the decode launches'
// entries QrpEntry[pairs] by chunk of jobs and level, the marker kernels' status word per pair, then per pair its state,
// the marker counts per 4 KiB of scan with their scan, and the interval offsets.  The registry (qs_encode_plan.h) holds
// the plan -- the pairs, the level lists and the grids -- under the workspace's address: the run has no options.
#include "qs_common.h"
#include "qs_stage.h"
#include "qs_read_prog.h"
#include "qs_encode_plan.h"

#include <algorithm>

void qs_launch_read_markers(const QrArgs& a, int zwgs, int mwgs, hipStream_t s);
void qs_launch_read_prog_init(const QrpArgs& a, int zwgs, hipStream_t s);
void qs_launch_read_prog_check(const QrpArgs& a, hipStream_t s);
void qs_launch_read_prog_decode(const QrpArgs& a, int dwgs, hipStream_t s);

static_assert(sizeof(qs_hip_encode_scan) == sizeof(QpScanRec), "qs_hip_encode_scan is the header's QpScanRec");
static_assert(QS_HIP_MAX_SCANS == QRP_MAX_SCANS && QS_RD_CHUNK == QS_HIP_READ_CHUNK, "include/jpegqs_hip.h and qs_read_prog.h disagree");
static_assert(sizeof(QrpArgs) <= 4096 && sizeof(QrArgs) <= 4096, "kernel arguments: 4 KiB at most");

namespace {

struct Level {                     // one decode launch: its entries in the workspace's list, its workgroups
  uint32_t first, count;
  int32_t wgs;
};
struct Plan {
  int njobs = 0;
  std::vector<QrJob> D;            // per pair, job by job in file order
  std::vector<QrpScan> X;
  std::vector<QrpEntry> E;         // by chunk of jobs, then level
  std::vector<QsEncGeom> full;     // per job: the frame's geometry the plan was made for
  std::vector<int> pair0;          // per job: its first pair; [njobs]: the pairs of the batch
  std::vector<std::vector<Level>> levels;   // per chunk of jobs
  uint64_t off_x = 0, off_e = 0, off_pstatus = 0, total = 0;
};
QsPrepared<Plan> g_plans(256);

int make_plan(qs_hip_job* const* jobs, int njobs, const qs_hip_read_prog_opts* const* opts, bool tables, Plan& P,
              qs_hip_read_prog_info* per_job, const char* who) {
  if (!jobs || njobs < 1) return qs_fail(QS_HIP_EINVAL, "%s: %d jobs (at least one)", who, njobs);
  if (!opts) return qs_fail(QS_HIP_EINVAL, "%s: null opts", who);
  P = Plan();
  P.njobs = njobs;
  std::vector<int32_t> level;
  for (int i = 0; i < njobs; ++i) {
    const qs_hip_job* job = jobs[i];
    const qs_hip_read_prog_opts* o = opts[i];
    if (int rc = check_job(job, Who(who, i).s)) return rc;
    if (!o || !o->scans || o->nscans < 1) return qs_fail(QS_HIP_EINVAL, "%s: job %d has no scans (the file's script, tables and offsets)", who, i);
    if (o->nscans > QRP_MAX_SCANS)
      return qs_fail(QS_HIP_ENOTSUP, "%s: job %d: %d scans; at most %d are read", who, i, o->nscans, QRP_MAX_SCANS);
    const int nc = job->ncomp;
    std::vector<QpScanRec> recs((size_t)o->nscans);
    for (int s = 0; s < o->nscans; ++s) memcpy(&recs[(size_t)s], &o->scans[s].scan, sizeof(QpScanRec));
    int bad = -1;
    const char* why = "";
    switch (qp_validate_script(recs.data(), o->nscans, nc, &bad, &why)) {
      case QP_SCRIPT_OK:
      case QP_SCRIPT_REFINE: break;
      case QP_SCRIPT_SEQUENTIAL:
        return qs_fail(QS_HIP_ENOTSUP, "%s: job %d, scan %d: %s is not a progressive file", who, i, bad, why);
      default:
        if (bad >= 0) return qs_fail(QS_HIP_EINVAL, "%s: job %d, scan %d: %s", who, i, bad, why);
        return qs_fail(QS_HIP_EINVAL, "%s: job %d: %s", who, i, why);
    }
    QsEncGeom full;
    int detail = 0;
    for (int c = 0; c < nc; ++c)
      if (int rc = check_block_count(job, c, Who(who, i).s)) return rc;
    if (qrp_frame_geometry(nc, job->image_width, job->image_height, job->hsamp, job->vsamp, job->wblk, job->hblk, &full,
                           &detail) != QS_GEOM_OK)
      return qs_fail(QS_HIP_EINVAL, "%s: job %d: a %d x %d image needs sampling factors 1..4 and, per component, at least "
                     "libjpeg's width_in_blocks x height_in_blocks blocks", who, i, job->image_width, job->image_height);
    level.assign((size_t)o->nscans, 0);
    const int nlevels = qrp_levels(recs.data(), o->nscans, level.data());
    P.pair0.push_back((int)P.D.size());
    P.full.push_back(full);
    if (per_job) {
      memset(&per_job[i], 0, sizeof per_job[i]);
      per_job[i].nscans = o->nscans;
      per_job[i].levels = nlevels;
    }
    for (int s = 0; s < o->nscans; ++s) {
      const qs_hip_read_prog_scan& r = o->scans[s];
      QrJob J;
      QrpScan X;
      memset(&J, 0, sizeof J);
      memset(&X, 0, sizeof X);
      if (r.restart_interval < 0 || r.restart_interval > 65535)
        return qs_fail(QS_HIP_EINVAL, "%s: job %d, scan %d: restart_interval %d (0 .. 65535)", who, i, s, r.restart_interval);
      long long d = 0;
      switch (qrp_describe(full, recs[(size_t)s], r.dc_tbl, r.ac_tbl, r.restart_interval, r.offset, i, &J, &X, &d)) {
        case QRP_OK: break;
        case QRP_MCU:
          return qs_fail(QS_HIP_ENOTSUP, "%s: job %d, scan %d: %lld blocks in an MCU; libjpeg takes at most 10", who, i, s, d);
        case QRP_CAP:
          return qs_fail(QS_HIP_ENOTSUP, "%s: job %d, scan %d: %lld blocks in a restart interval (restart_interval %d, %d MCUs "
                         "of %d blocks); one lane reads an interval, of at most %d blocks", who, i, s, d, r.restart_interval,
                         J.g.mcus, J.g.bpm, QS_RD_MAX_INTERVAL_BLOCKS);
        default:
          return qs_fail(QS_HIP_EINVAL, "%s: job %d, scan %d: component %lld names a table outside 0 .. 3", who, i, s, d);
      }
      X.level = level[(size_t)s];
      if (s + 1 < o->nscans) {
        X.limit = o->scans[s + 1].offset;
        if (X.limit < X.offset)
          return qs_fail(QS_HIP_EINVAL, "%s: job %d, scan %d: the next scan's offset lies in front of this one's", who, i, s);
      }
      if (!(X.Ss == 0 && X.Ah))                                       // a DC refinement has no symbols
        for (int c = 0; c < recs[(size_t)s].ncomp; ++c) {
          const bool ac = X.Ss != 0;
          const int id = ac ? J.ac_tbl[c] : J.dc_tbl[c];
          if (!(ac ? r.has_ac[id] : r.has_dc[id]))
            return qs_fail(QS_HIP_EINVAL, "%s: job %d, scan %d: component %d uses %s table %d, which the scan's record does "
                           "not hold", who, i, s, c, ac ? "AC" : "DC", id);
          if (tables && qr_build_table(ac ? r.ac[id].bits : r.dc[id].bits, ac ? r.ac[id].huffval : r.dc[id].huffval, !ac,
                                       &J.tab[(ac ? 4 : 0) + id]))
            return qs_fail(QS_HIP_EINVAL, "%s: job %d, scan %d: %s table %d is not a valid Huffman table", who, i, s,
                           ac ? "AC" : "DC", id);
        }
      if (per_job) {
        per_job[i].mcus[s] = J.g.mcus;
        per_job[i].intervals[s] = J.intervals;
      }
      P.D.push_back(J);
      P.X.push_back(X);
    }
  }
  P.pair0.push_back((int)P.D.size());
  const size_t np = P.D.size();
  // the decode launches: per chunk of jobs, level by level, the pairs of that level and their first workgroups
  for (int j0 = 0; j0 < njobs; j0 += QS_RD_CHUNK) {
    const int p0 = P.pair0[(size_t)j0], p1 = P.pair0[(size_t)std::min(njobs, j0 + QS_RD_CHUNK)];
    int nlev = 0;
    for (int p = p0; p < p1; ++p) nlev = std::max(nlev, P.X[(size_t)p].level + 1);
    std::vector<Level> lv;
    for (int l = 0; l < nlev; ++l) {
      Level L{(uint32_t)P.E.size(), 0, 0};
      long long wgs = 0;
      for (int p = p0; p < p1; ++p) {
        if (P.X[(size_t)p].level != l) continue;
        P.E.push_back(QrpEntry{p, (int32_t)wgs});
        wgs += ceil_div(P.D[(size_t)p].intervals, QS_RD_DWG);
        if (wgs > 0x7fffffffLL) return qs_fail(QS_HIP_EINVAL, "%s: more than 2^31 workgroups in one launch", who);
        ++L.count;
      }
      L.wgs = (int32_t)wgs;
      lv.push_back(L);
    }
    P.levels.push_back(lv);
  }
  Layout L;
  L.take(np * sizeof(QrJob));
  P.off_x = L.take(np * sizeof(QrpScan));
  P.off_e = L.take(np * sizeof(QrpEntry));
  P.off_pstatus = L.take(np * 4);
  for (size_t p = 0; p < np; ++p) {
    QrJob& J = P.D[p];
    const uint64_t chunks = (J.max_scan + 32) / QS_RD_MCHUNK + 2;
    J.off_state = L.take(sizeof(QrState));
    J.off_cnt = L.take(chunks * 4);
    J.off_off = L.take(chunks * 4);
    J.off_p = L.take(((uint64_t)J.intervals + 1) * 8);
  }
  P.total = L.total;
  return QS_HIP_OK;
}

}  // namespace

extern "C" int qs_hip_read_prog_device_batch_info(qs_hip_job* const* jobs, int njobs, const qs_hip_read_prog_opts* const* opts,
                                                  qs_hip_read_prog_info* per_job, size_t* bytes) {
  return guarded([&]() -> int {
    const char* who = "qs_hip_read_prog_device_batch_info";
    if (!per_job || !bytes) return qs_fail(QS_HIP_EINVAL, "%s: null result", who);
    Plan P;
    if (int r = make_plan(jobs, njobs, opts, false, P, per_job, who)) return r;
    *bytes = (size_t)P.total;
    return QS_HIP_OK;
  });
}

extern "C" int qs_hip_read_prog_device_batch_prepare(qs_hip_job* const* jobs, int njobs,
                                                     const qs_hip_read_prog_opts* const* opts, void* d_workspace,
                                                     size_t bytes, void* stream) {
  return guarded([&]() -> int {
    const char* who = "qs_hip_read_prog_device_batch_prepare";
    Plan P;
    if (int r = make_plan(jobs, njobs, opts, true, P, nullptr, who)) return r;
    if (int r = check_workspace(P.total, d_workspace, bytes, who)) return r;
    if (int r = device_ok()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    HIP_TRY(hipMemcpyAsync(ws, P.D.data(), P.D.size() * sizeof(QrJob), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws + P.off_x, P.X.data(), P.X.size() * sizeof(QrpScan), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws + P.off_e, P.E.data(), P.E.size() * sizeof(QrpEntry), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                // (pageable sources: they must outlive the copies)
    for (QrJob& J : P.D) memset(J.tab, 0, sizeof J.tab);   // (the registry needs no tables)
    g_plans.store(d_workspace, std::move(P));
    return QS_HIP_OK;
  });
}

extern "C" int qs_hip_read_prog_device_batch(qs_hip_job* const* jobs, int njobs, const uint8_t* const* d_file,
                                             const uint64_t* file_bytes, int32_t* d_status, void* d_workspace, size_t bytes,
                                             void* stream) {
  return guarded([&]() -> int {
    const char* who = "qs_hip_read_prog_device_batch";
    if (!jobs || njobs < 1) return qs_fail(QS_HIP_EINVAL, "%s: %d jobs (at least one)", who, njobs);
    if (!d_file || !file_bytes || !d_status) return qs_fail(QS_HIP_EINVAL, "%s: null argument", who);
    if (!workspace_ok(d_workspace, bytes, 0)) return qs_fail(QS_HIP_EINVAL, "%s: no workspace (256-byte aligned)", who);
    const std::shared_ptr<const Plan> plan = g_plans.find(d_workspace);
    if (!plan) return qs_fail(QS_HIP_EINVAL, "%s: the workspace was never prepared for this route", who);
    const Plan& P = *plan;
    if (P.njobs != njobs)
      return qs_fail(QS_HIP_EINVAL, "%s: the workspace was prepared for %d jobs, the call has %d", who, P.njobs, njobs);
    if (int r = check_workspace(P.total, d_workspace, bytes, who)) return r;
    for (int i = 0; i < njobs; ++i) {
      const qs_hip_job* job = jobs[i];
      const Who w(who, i);
      if (int rc = check_job(job, w.s)) return rc;
      if (!d_file[i]) return qs_fail(QS_HIP_EINVAL, "%s: no file bytes", w.s);
      QsEncGeom full;
      int detail = 0;
      if (qrp_frame_geometry(job->ncomp, job->image_width, job->image_height, job->hsamp, job->vsamp, job->wblk, job->hblk,
                             &full, &detail) != QS_GEOM_OK || memcmp(&full, &P.full[(size_t)i], sizeof full))
        return qs_fail(QS_HIP_EINVAL, "%s: not the geometry prepare saw", w.s);
      for (int c = 0; c < job->ncomp; ++c) {
        if (int rc = check_array(job->coef[c], c, false, w.s)) return rc;
        if (int rc = check_block_count(job, c, w.s)) return rc;
      }
    }
    if (int r = device_ok()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    for (int j0 = 0; j0 < njobs; j0 += QS_RD_CHUNK) {
      QrpArgs a;
      memset(&a, 0, sizeof a);
      a.pairs = reinterpret_cast<const QrJob*>(ws);
      a.scans = reinterpret_cast<const QrpScan*>(ws + P.off_x);
      a.ws = ws;
      a.d_status = d_status;
      a.job0 = j0;
      a.n = std::min(QS_RD_CHUNK, njobs - j0);
      a.pair0 = P.pair0[(size_t)j0];
      a.npairs = P.pair0[(size_t)(j0 + a.n)] - a.pair0;
      long long zwgs = 0;
      for (int k = 0; k < a.n; ++k) {
        const qs_hip_job* job = jobs[j0 + k];
        long long blocks = 0;
        for (int c = 0; c < job->ncomp; ++c) {
          a.coef[k][c] = job->coef[c];
          a.nblk[k][c] = job->wblk[c] * job->hblk[c];
          blocks += a.nblk[k][c];
        }
        a.file[k] = d_file[j0 + k];
        a.file_bytes[k] = file_bytes[j0 + k];
        a.zwg0[k] = (int)zwgs;
        zwgs += qr_zero_wgs(blocks);
      }
      a.zwg0[a.n] = (int)zwgs;
      qs_launch_read_prog_init(a, (int)zwgs, s);
      // the scans' ends and RSTn markers: the interval route's marker launches on the pairs' descriptors, 32 pairs a set
      // (a pair's status word lies in the workspace; its arrays are the job's, zeroed above: the set's own zeroing is empty)
      for (int p0 = 0; p0 < a.npairs; p0 += QS_RD_CHUNK) {
        QrArgs m;
        memset(&m, 0, sizeof m);
        m.jobs = a.pairs + a.pair0 + p0;
        m.ws = ws;
        m.d_status = reinterpret_cast<int32_t*>(ws + P.off_pstatus);
        m.job0 = a.pair0 + p0;
        m.n = std::min(QS_RD_CHUNK, a.npairs - p0);
        long long mwgs = 0;
        for (int q = 0; q < m.n; ++q) {
          const size_t p = (size_t)(a.pair0 + p0 + q);
          const int k = P.X[p].job - j0;
          QrSrc file;
          file.p = a.file[k];
          file.n = a.file_bytes[k];
          const QrSrc sc = qrp_scan_src(file, P.D[p], P.X[p]);
          m.p[q].scan = sc.p;
          m.p[q].scan_bytes = sc.n;
          m.zwg0[q] = q;
          const uint64_t units = ((reinterpret_cast<uintptr_t>(sc.p) & 15) + sc.n + 15) / 16;
          m.mwg0[q] = (int)mwgs;
          mwgs += (long long)((units + QS_RD_WG - 1) / QS_RD_WG);
          if (mwgs > 0x7fffffffLL) return qs_fail(QS_HIP_EINVAL, "%s: more than 2^31 workgroups in one launch", who);
        }
        qs_launch_read_markers(m, m.n, (int)mwgs, s);
      }
      qs_launch_read_prog_check(a, s);
      for (const Level& L : P.levels[(size_t)(j0 / QS_RD_CHUNK)]) {
        if (!L.count) continue;
        a.list = reinterpret_cast<const QrpEntry*>(ws + P.off_e) + L.first;
        a.nlist = (int32_t)L.count;
        qs_launch_read_prog_decode(a, L.wgs, s);
      }
    }
    HIP_TRY(hipGetLastError());
    return QS_HIP_OK;
  });
}
