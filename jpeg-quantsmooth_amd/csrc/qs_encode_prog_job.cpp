// qs_encode_prog_job.cpp -- progressive files (spectral selection, refinement scans behind a flag) of the flat C ABI (include/jpegqs_hip.h):
// qs_hip_encode_progressive_device_batch_info / _prepare / _files.  DESIGN.md section 17.
//
// A job with a script of n scans becomes n scan jobs: QsEncJob descriptors with the scan's own geometry (csrc/
// qs_encode_prog.h: qp_scan_geometry), restart interval and workspace arrays, so that the coder's shared kernels run on
// them as on any job, and QpScan records with what only the progressive kernels need.
// Workspace: QsEncJob[scan jobs], QpScan[scan jobs], QpJob[jobs], the bytes of the DRI / SOS markers, then per scan job
// the arrays of one coded scan (csrc/qs_encode_plan.h, with the restart rule, the scratch and the registry of prepared
// workspaces) and the EOB-run arrays.  Scratch: the whole-file run's arrays and each scan job's length, status and d_stop.
// The registry holds the whole plan; a workspace the run does not find there gives every job status 4.
#include "qs_common.h"
#include "qs_stage.h"
#include "qs_encode.h"
#include "qs_encode_prog.h"
#include "qs_encode_plan.h"

#include <algorithm>

void qs_launch_encode_prog(const QsEncArgs& a, const QpScan* xs, const QsHuffArgs& h, int wgs, int swgs, int refine,
                           hipStream_t s);
void qs_launch_encode_prog_stuff(const QsEncArgs& a, int swgs, hipStream_t s);
void qs_launch_encode_prog_begin(const QpJobArgs& a, hipStream_t s);
void qs_launch_encode_prog_frame(const QpJobArgs& a, hipStream_t s);
void qs_launch_encode_prog_nofile(uint64_t* d_len, int32_t* d_status, int njobs, hipStream_t s);

static_assert(sizeof(qs_hip_encode_scan) == sizeof(QpScanRec), "qs_hip_encode_scan is the header's QpScanRec");
static_assert(QS_HIP_MAX_SCANS == QP_MAX_SCANS, "one limit");
static_assert(sizeof(QpJobArgs) <= 4096, "kernel arguments: 4 KiB at most");
static_assert(QP_MAXBITS <= 0xffff, "a block's bits travel as uint16");
static_assert(QR_AC_MAXBITS(1, 63) <= QP_MAXBITS, "the emit kernel's LDS image holds a refinement scan's blocks");
static_assert(QS_HIP_PROG_REFINE == 1, "the one flag");

namespace {

struct Plan {
  int njobs = 0;
  std::vector<QsEncJob> D;         // per scan job
  std::vector<QpScan> X;
  std::vector<QpJob> Q;            // per job
  std::vector<QsEncJob> full;      // per job: the frame's geometry the plan was made for
  std::vector<int> refine;         // per chunk of scan jobs: -1 without a refinement scan, else its rounds of qr_hop
  std::vector<uint8_t> mids;       // the DRI / SOS bytes, and where they go in the workspace
  uint64_t off_mids = 0, off_x = 0, off_q = 0;
  uint64_t total = 0;
};
QsPrepared<Plan> g_plans(256);

struct Scratch : QsEncScratch {    // the whole-file run's arrays per scan job, and each scan job's length, status and d_stop
  uint64_t seglen, sstatus, sstop;
  explicit Scratch(size_t nsj) : QsEncScratch(nsj) {
    seglen = L.take(nsj * 8);
    sstatus = L.take(nsj * 4);
    sstop = L.take(nsj * 4);
    total = L.total;
  }
};

// jpeg_set_colorspace's component ids
void default_ids(int cs, int32_t* id) {
  static const int32_t RGB[4] = {0x52, 0x47, 0x42, 0}, CMYK[4] = {0x43, 0x4D, 0x59, 0x4B};
  for (int c = 0; c < 4; ++c) id[c] = cs == 2 ? RGB[c] : cs == 4 ? CMYK[c] : c + 1;
}

// the plan of a batch; per_job may be null
int make_plan(qs_hip_job* const* jobs, int njobs, const qs_hip_encode_prog_opts* const* opts, Plan& P,
              qs_hip_encode_prog_info* per_job, const char* who) {
  if (!jobs || njobs < 1) return qs_fail(QS_HIP_EINVAL, "%s: %d jobs (at least one)", who, njobs);
  if (!opts) return qs_fail(QS_HIP_EINVAL, "%s: no scripts", who);
  P = Plan();
  P.njobs = njobs;
  std::vector<uint64_t> maxbits, nints;             // per scan job: the worst case of one block, its intervals at most
  std::vector<int> nblks;                           // ... and its blocks at most
  std::vector<uint64_t> mid_at;                     // per scan job and variant: offset into P.mids
  for (int i = 0; i < njobs; ++i) {
    const qs_hip_encode_prog_opts* o = opts[i];
    if (!o || !o->scans) return qs_fail(QS_HIP_EINVAL, "%s: job %d has no script", who, i);
    if (o->flags & ~QS_HIP_PROG_REFINE) return qs_fail(QS_HIP_EINVAL, "%s: job %d: flags %#x", who, i, (unsigned)o->flags);
    QsEncJob full;
    if (int r = qs_enc_describe(jobs[i], &full, nullptr, false, Who(who, i).s)) return r;
    const int nc = jobs[i]->ncomp;
    int bad = -1;
    const char* why = "";
    const QpScanRec* recs = reinterpret_cast<const QpScanRec*>(o->scans);
    switch (qp_validate_script(recs, o->nscans, nc, &bad, &why)) {
      case QP_SCRIPT_OK: break;
      case QP_SCRIPT_REFINE:
        if (o->flags & QS_HIP_PROG_REFINE) {
          if (o->nscans > QP_MAX_SCANS)
            return qs_fail(QS_HIP_ENOTSUP, "%s: job %d: a valid script of %d scans; at most %d are written", who, i, o->nscans,
                           QP_MAX_SCANS);
          break;
        }
        return qs_fail(QS_HIP_ENOTSUP, "%s: job %d, scan %d: %s: refinement scans are not implemented", who, i, bad, why);
      case QP_SCRIPT_SEQUENTIAL:
        return qs_fail(QS_HIP_ENOTSUP, "%s: job %d, scan %d: %s is not a progressive file", who, i, bad, why);
      default:
        if (bad >= 0) return qs_fail(QS_HIP_EINVAL, "%s: job %d, scan %d: %s", who, i, bad, why);
        return qs_fail(QS_HIP_EINVAL, "%s: job %d: %s", who, i, why);
    }
    if (o->nscans > QP_MAX_SCANS)                    // (no script of Ah = 0 scans that passes is that long)
      return qs_fail(QS_HIP_EINVAL, "%s: job %d: %d scans, at most %d", who, i, o->nscans, QP_MAX_SCANS);
    if (int r = qs_enc_check_restart(o->restart_interval, o->restart_in_rows, who, i)) return r;
    int32_t ids[4];
    default_ids(jobs[i]->colorspace, ids);
    if (o->component_id[0] | o->component_id[1] | o->component_id[2] | o->component_id[3])
      for (int c = 0; c < 4; ++c) ids[c] = o->component_id[c];
    QpJob q{(int32_t)P.D.size(), o->nscans, full.two, 0};
    P.Q.push_back(q);
    P.full.push_back(full);
    if (per_job) {
      memset(&per_job[i], 0, sizeof per_job[i]);
      per_job[i].nscans = o->nscans;
      per_job[i].max_body_bytes = 2;
    }
    int last_dri[2] = {0, 0};
    for (int s = 0; s < o->nscans; ++s) {
      const QpScanRec& r = recs[s];
      QsEncJob J;
      memset(&J, 0, sizeof J);
      QpScan X;
      memset(&X, 0, sizeof X);
      J.two = full.two;
      X.Ss = r.Ss;
      X.Se = r.Se;
      X.Al = r.Al;
      X.Ah = r.Ah;
      X.job = i;
      uint8_t sos[QP_MID_MAX];
      int n = 0;
      sos[n++] = 0xff;
      sos[n++] = 0xda;
      sos[n++] = 0;
      sos[n++] = (uint8_t)(6 + 2 * r.ncomp);
      sos[n++] = (uint8_t)r.ncomp;
      for (int c = 0; c < r.ncomp; ++c) {
        const int tb = full.tbl[r.comp[c]];
        J.tbl[c] = tb;
        // jcmarker.c emit_sos: a DC scan names no AC table, an AC scan no DC table, a DC refinement no table at all
        sos[n++] = (uint8_t)ids[r.comp[c]];
        sos[n++] = (uint8_t)(r.Ss == 0 ? (r.Ah ? 0 : tb << 4) : tb);
        const int w = (r.Ss == 0 ? 0 : 2) + tb;                      // each table once, in component order
        bool sent = false;
        for (int t = 0; t < X.ntab; ++t) sent |= X.tab[t] == w;
        if (!sent && !(r.Ss == 0 && r.Ah)) X.tab[X.ntab++] = w;          // (a DC refinement has no symbols: no DHT)
      }
      X.actb = J.tbl[0];
      sos[n++] = (uint8_t)r.Ss;
      sos[n++] = (uint8_t)r.Se;
      sos[n++] = (uint8_t)((r.Ah << 4) | r.Al);
      uint64_t nint = 1;
      int nblocks = 0, rounds = r.Ah ? 0 : -1;
      for (int v = 0; v < (full.two ? 2 : 1); ++v) {
        int detail = 0;
        if (qp_scan_geometry(full.g[v], r, &J.g[v], &detail) != QS_GEOM_OK)
          return qs_fail(QS_HIP_EINVAL, "%s: job %d, scan %d: %d blocks in an MCU; libjpeg takes at most 10", who, i, s, detail);
        const QsEncGeom& g = J.g[v];
        int ri = 0;                                                  // (counted in this scan's MCUs)
        J.ri[v] = qs_enc_restart(o->restart_interval, o->restart_in_rows, g, &ri);
        if (J.ri[v]) nint = std::max<uint64_t>(nint, (uint64_t)ceil_div(g.mcus, J.ri[v]));
        nblocks = std::max(nblocks, g.nblocks);
        if (r.Ah && r.Ss) {
          // a run stays inside a restart interval and cuts a piece every QR_PIECE_MIN blocks at the soonest: after k rounds
          // of qr_hop every piece start less than 2^k pieces behind the run's start is marked
          const long long per = (long long)(J.ri[v] ? J.ri[v] : g.mcus) * g.bpm;
          const long long pieces = ceil_div(std::min<long long>(per, g.nblocks), (long long)QR_PIECE_MIN);
          int k = 0;
          while ((1LL << k) < pieces) ++k;
          rounds = std::max(rounds, k);
        }
        // jcmarker.c write_scan_header: DRI when the interval differs from the last one written
        mid_at.push_back(P.mids.size());
        if (ri != last_dri[v]) {
          const uint8_t dri[6] = {0xff, 0xdd, 0, 4, (uint8_t)(ri >> 8), (uint8_t)ri};
          P.mids.insert(P.mids.end(), dri, dri + 6);
          last_dri[v] = ri;
          X.mid_bytes[v] = 6;
        }
        P.mids.insert(P.mids.end(), sos, sos + n);
        X.mid_bytes[v] += (uint32_t)n;
        if (v == 0 && per_job) {
          per_job[i].mcus[s] = g.mcus;
          per_job[i].interval[s] = ri;
        }
      }
      if (!full.two) mid_at.push_back(P.mids.size());
      const uint64_t mb = r.Ah ? (r.Ss == 0 ? QR_DC_MAXBITS : QR_AC_MAXBITS(r.Ss, r.Se))
                               : (r.Ss == 0 ? QP_DC_MAXBITS : QP_AC_MAXBITS(r.Ss, r.Se));
      maxbits.push_back(mb);
      if (per_job)   // every byte stuffed; per interval end a pad byte that may be stuffed and the marker; the markers
        per_job[i].max_body_bytes += 2 * (((uint64_t)nblocks * mb + 7) / 8 + 1) + 4 * (nint - 1) + 2 * (21 + 256) + QP_MID_MAX;
      nblks.push_back(nblocks);
      nints.push_back(nint);
      if (P.D.size() % QS_ENC_CHUNK == 0) P.refine.push_back(-1);
      P.refine.back() = std::max(P.refine.back(), rounds);
      P.D.push_back(J);
      P.X.push_back(X);
    }
  }
  // the workspace
  const size_t nsj = P.D.size();
  Layout L;
  L.take(nsj * sizeof(QsEncJob));
  P.off_x = L.take(nsj * sizeof(QpScan));
  P.off_q = L.take((uint64_t)njobs * sizeof(QpJob));
  P.off_mids = L.take(P.mids.size());
  long long wgs = 0, swgs = 0;
  for (size_t j = 0; j < nsj; ++j) {
    QsEncJob& J = P.D[j];
    QpScan& X = P.X[j];
    if (j % QS_ENC_CHUNK == 0) wgs = swgs = 0;
    if (int r = qs_enc_scan_layout(L, J, wgs, swgs, nblks[j], nints[j], maxbits[j], true, who)) return r;
    const uint64_t slots = (uint64_t)J.nwg * QS_ENC_WG;
    X.off_flags = L.take(slots);
    X.off_wghead = L.take((uint64_t)J.nwg * 4);
    X.off_wgcarry = L.take((uint64_t)J.nwg * 4);
    X.off_eob = L.take(slots * 2);
    if (X.Ah && X.Ss) {
      X.off_w = L.take(slots * 4);
      X.off_jump[0] = L.take(slots * 4);
      X.off_jump[1] = L.take(slots * 4);
      X.off_reach = L.take(slots);
    }
    X.off_mid[0] = P.off_mids + mid_at[2 * j];
    X.off_mid[1] = P.off_mids + mid_at[2 * j + 1];
  }
  P.total = L.total;
  return QS_HIP_OK;
}

}  // namespace

extern "C" int qs_hip_encode_progressive_device_batch_info(qs_hip_job* const* jobs, int njobs,
                                                           const qs_hip_encode_prog_opts* const* opts,
                                                           qs_hip_encode_prog_info* per_job, size_t* workspace_bytes,
                                                           size_t* scratch_bytes) {
  return guarded([&]() -> int {
    const char* who = "qs_hip_encode_progressive_device_batch_info";
    if (!per_job || !workspace_bytes || !scratch_bytes) return qs_fail(QS_HIP_EINVAL, "%s: null result", who);
    Plan P;
    if (int r = make_plan(jobs, njobs, opts, P, per_job, who)) return r;
    *workspace_bytes = (size_t)P.total;
    *scratch_bytes = (size_t)Scratch(P.D.size()).total;
    return QS_HIP_OK;
  });
}

extern "C" int qs_hip_encode_progressive_device_batch_prepare(qs_hip_job* const* jobs, int njobs,
                                                              const qs_hip_encode_prog_opts* const* opts,
                                                              void* d_workspace, size_t bytes, void* stream) {
  return guarded([&]() -> int {
    const char* who = "qs_hip_encode_progressive_device_batch_prepare";
    Plan P;
    if (int r = make_plan(jobs, njobs, opts, P, nullptr, who)) return r;
    if (int r = check_workspace(P.total, d_workspace, bytes, who)) return r;
    if (int r = device_ok()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    HIP_TRY(hipMemcpyAsync(ws, P.D.data(), P.D.size() * sizeof(QsEncJob), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws + P.off_x, P.X.data(), P.X.size() * sizeof(QpScan), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws + P.off_q, P.Q.data(), P.Q.size() * sizeof(QpJob), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws + P.off_mids, P.mids.data(), P.mids.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                // (pageable sources: they must outlive the copies)
    g_plans.store(d_workspace, std::move(P));        // (a plan that leaves the registry: its workspace runs to status 4)
    return QS_HIP_OK;
  });
}

extern "C" int qs_hip_encode_progressive_device_batch_files(qs_hip_job* const* jobs, int njobs,
                                                            const qs_hip_encode_frame* frames, const int32_t* d_stop,
                                                            uint8_t* const* d_out, const size_t* out_capacity,
                                                            uint64_t* d_len, int32_t* d_status, void* d_scratch,
                                                            size_t scratch_bytes, void* d_workspace, size_t bytes,
                                                            void* stream) {
  return guarded([&]() -> int {
    const char* who = "qs_hip_encode_progressive_device_batch_files";
    if (!jobs || njobs < 1) return qs_fail(QS_HIP_EINVAL, "%s: %d jobs (at least one)", who, njobs);
    if (!frames || !d_out || !out_capacity || !d_len || !d_status) return qs_fail(QS_HIP_EINVAL, "%s: null argument", who);
    if (!workspace_ok(d_workspace, bytes, 0)) return qs_fail(QS_HIP_EINVAL, "%s: no workspace (256-byte aligned)", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const std::shared_ptr<const Plan> plan = g_plans.find(d_workspace);
    if (!plan) {
      if (int r = device_ok()) return r;
      qs_launch_encode_prog_nofile(d_len, d_status, njobs, s);
      HIP_TRY(hipGetLastError());
      return QS_HIP_OK;
    }
    const Plan& P = *plan;
    if (P.njobs != njobs)
      return qs_fail(QS_HIP_EINVAL, "%s: the workspace was prepared for %d jobs, the call has %d", who, P.njobs, njobs);
    if (int r = check_workspace(P.total, d_workspace, bytes, who)) return r;
    const size_t nsj = P.D.size();
    const Scratch FS(nsj);
    if (!workspace_ok(d_scratch, scratch_bytes, FS.total))
      return qs_fail(QS_HIP_EINVAL, "%s: scratch of %zu bytes (256-byte aligned), the batch needs %llu", who, scratch_bytes,
                     (unsigned long long)FS.total);
    std::vector<QsEncPtrs> ptrs((size_t)njobs);
    for (int i = 0; i < njobs; ++i) {
      QsEncJob full;
      if (int r = qs_enc_describe(jobs[i], &full, &ptrs[(size_t)i], true, Who(who, i).s)) return r;
      const QsEncJob& was = P.full[(size_t)i];
      if (full.two != was.two || memcmp(full.g, was.g, sizeof full.g) || memcmp(full.tbl, was.tbl, sizeof full.tbl))
        return qs_fail(QS_HIP_EINVAL, "%s: job %d is not the job the workspace was prepared for", who, i);
      if (!d_out[i]) return qs_fail(QS_HIP_EINVAL, "%s: job %d has no output buffer", who, i);
      ptrs[(size_t)i].out = d_out[i];
      ptrs[(size_t)i].cap = out_capacity[i];
      const int nv = (full.two && d_stop) ? 2 : 1;
      for (int v = 0; v < nv; ++v)
        if (!frames[i].d_head[v] || !frames[i].head_bytes[v])
          return qs_fail(QS_HIP_EINVAL, "%s: job %d: the frame lacks the head of variant %d, which the job can take", who, i, v);
    }
    if (int r = device_ok()) return r;
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    uint8_t* sc = static_cast<uint8_t*>(d_scratch);
    const QsEncJob* d_jobs = reinterpret_cast<const QsEncJob*>(ws);
    const QpScan* d_scans = reinterpret_cast<const QpScan*>(ws + P.off_x);
    const QpJob* d_q = reinterpret_cast<const QpJob*>(ws + P.off_q);
    auto job_args = [&](int j0) {
      QpJobArgs q;
      memset(&q, 0, sizeof q);
      q.sjobs = d_jobs;
      q.scans = d_scans;
      q.jobs = d_q + j0;
      q.ws = ws;
      q.d_stop = d_stop;
      q.sstop = reinterpret_cast<int32_t*>(sc + FS.sstop);
      q.tables = sc + FS.tables;
      q.prefix = reinterpret_cast<uint64_t*>(sc + FS.prefix);
      q.seglen = reinterpret_cast<const uint64_t*>(sc + FS.seglen);
      q.sstatus = reinterpret_cast<const int32_t*>(sc + FS.sstatus);
      q.d_len = d_len;
      q.d_status = d_status;
      q.job0 = j0;
      q.n = std::min(QS_ENC_CHUNK, njobs - j0);
      for (int k = 0; k < q.n; ++k) {
        const qs_hip_encode_frame& f = frames[j0 + k];
        for (int v = 0; v < 2; ++v) {
          q.f[k].head[v] = f.d_head[v];
          q.f[k].head_bytes[v] = f.d_head[v] ? f.head_bytes[v] : 0;
        }
        q.f[k].out = d_out[j0 + k];
        q.f[k].cap = out_capacity[j0 + k];
      }
      return q;
    };
    auto scan_args = [&](size_t j0) {
      QsEncArgs a;
      memset(&a, 0, sizeof a);
      a.jobs = d_jobs + j0;
      a.ws = ws;
      a.d_stop = reinterpret_cast<const int32_t*>(sc + FS.sstop);
      a.d_len = reinterpret_cast<uint64_t*>(sc + FS.seglen);
      a.d_status = reinterpret_cast<int32_t*>(sc + FS.sstatus);
      a.d_counts = reinterpret_cast<uint32_t*>(sc + FS.counts);
      a.codes = reinterpret_cast<const uint32_t*>(sc + FS.codes);
      a.tstatus = reinterpret_cast<const int32_t*>(sc + FS.tstatus);
      a.job0 = (int32_t)j0;
      a.n = (int32_t)std::min<size_t>(QS_ENC_CHUNK, nsj - j0);
      a.restart = 1;
      for (int k = 0; k < a.n; ++k) {
        a.p[k] = ptrs[(size_t)P.X[j0 + k].job];
        a.wg0[k] = P.D[j0 + k].wg0;
        a.swg0[k] = P.D[j0 + k].swg0;
      }
      return a;
    };
    for (int j0 = 0; j0 < njobs; j0 += QS_ENC_CHUNK) qs_launch_encode_prog_begin(job_args(j0), s);
    for (size_t j0 = 0; j0 < nsj; j0 += QS_ENC_CHUNK) {
      const QsEncArgs a = scan_args(j0);
      QsHuffArgs h;
      memset(&h, 0, sizeof h);
      h.jobs = a.jobs;
      h.d_stop = a.d_stop;
      qs_enc_huff_scratch(h, sc, FS);
      h.job0 = a.job0;
      h.n = a.n;
      h.optimize = 1;
      const QsEncJob& last = P.D[j0 + a.n - 1];
      qs_launch_encode_prog(a, d_scans + j0, h, last.wg0 + last.nwg, last.swg0 + last.nswg, P.refine[j0 / QS_ENC_CHUNK], s);
    }
    for (int j0 = 0; j0 < njobs; j0 += QS_ENC_CHUNK) qs_launch_encode_prog_frame(job_args(j0), s);
    for (size_t j0 = 0; j0 < nsj; j0 += QS_ENC_CHUNK) {
      QsEncArgs a = scan_args(j0);
      a.d_counts = nullptr;
      a.prefix = reinterpret_cast<uint64_t*>(sc + FS.prefix);
      const QsEncJob& last = P.D[j0 + a.n - 1];
      qs_launch_encode_prog_stuff(a, last.swg0 + last.nswg, s);
    }
    HIP_TRY(hipGetLastError());
    return QS_HIP_OK;
  });
}
