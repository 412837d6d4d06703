// qs_read_job.cpp -- the device scan reader of the flat C ABI (include/jpegqs_hip.h): qs_hip_read_device_batch_info /
// _prepare / qs_hip_read_device_batch.  The entropy-coded segment of one sequential Huffman scan with restart intervals,
// in device memory, into the coefficient arrays of qs_hip_job records: what libjpeg 9's jpeg_read_coefficients leaves
// there, computed on the device (qs_kernels_read.hip, one lane per restart interval).
//
// Workspace: the QrJob descriptors of the batch (geometry, derived code tables), then per job its state, the marker
// counts per 4 KiB of scan with their scan, and the interval offsets -- a function of the jobs' geometry and options
// alone.  The segment's length is not known before the run: the arrays that depend on it are sized for the longest
// segment the geometry can have, and the kernels look no further.
//
// The split route (qs_hip_read_split_device_batch_*, qs_kernels_read_split.hip, one lane per QS_RD_SPLIT_BYTES of an
// interval) shares all of it and has no interval cap; behind the QrJob descriptors its workspace holds the QrsJob
// descriptors and, per job, the segment map, the segments' entry and exit states and block counts, the DC differences
// in scan order and the tiles of the two prefix sums.
#include "qs_common.h"
#include "qs_stage.h"
#include "qs_read_split.h"

#include <algorithm>

void qs_launch_read(const QrArgs& a, int zwgs, int mwgs, int dwgs, hipStream_t s);
void qs_launch_read_split(QrsArgs& x, int zwgs, int mwgs, int swgs, int twgs, hipStream_t s);

static_assert(QS_RD_CHUNK == QS_HIP_READ_CHUNK && QS_RD_MAX_INTERVAL_BLOCKS == QS_HIP_READ_MAX_INTERVAL_BLOCKS,
              "include/jpegqs_hip.h and qs_read.h disagree");
static_assert(QS_RD_SPLIT_BYTES == QS_HIP_READ_SPLIT_BYTES && QS_RD_SPLIT_ROUNDS == QS_HIP_READ_SPLIT_ROUNDS,
              "include/jpegqs_hip.h and qs_read_split.h disagree");

namespace {

uint64_t descriptors_bytes(int njobs) { return align_up((uint64_t)njobs * sizeof(QrJob)); }
uint64_t split_descriptors_bytes(int njobs) { return align_up((uint64_t)njobs * sizeof(QrsJob)); }

// geometry, tables and intervals of one job; the code tables themselves only when `tables`; split: no interval cap
int describe(const qs_hip_job* job, const qs_hip_read_opts* o, bool tables, bool split, QrJob* D, qs_hip_read_info* info,
             const char* who) {
  if (int rc = check_job(job, who)) return rc;
  if (!o) return qs_fail(QS_HIP_EINVAL, "%s: no options (the tables of each component and the restart interval)", who);
  const int n = job->ncomp;
  memset(D, 0, sizeof *D);
  if (int rc = qr_geometry(n, job->image_width, job->image_height, job->hsamp, job->vsamp, job->wblk, job->hblk, &D->g)) {
    if (rc == 2) return qs_fail(QS_HIP_ENOTSUP, "%s: more than 10 blocks in an MCU; libjpeg takes at most 10", who);
    return qs_fail(QS_HIP_EINVAL, "%s: a %d x %d image needs sampling factors 1..4 and, per component, at least libjpeg's "
                   "width_in_blocks x height_in_blocks blocks", who, job->image_width, job->image_height);
  }
  if (o->restart_interval < 0 || o->restart_interval > 65535)
    return qs_fail(QS_HIP_EINVAL, "%s: restart_interval %d (0 .. 65535)", who, o->restart_interval);
  qr_intervals(D->g, o->restart_interval, &D->ri, &D->intervals);
  const long long per = (long long)D->ri * D->g.bpm;
  if (!split && per > QS_RD_MAX_INTERVAL_BLOCKS)
    return qs_fail(QS_HIP_ENOTSUP, "%s: %lld blocks in a restart interval (restart_interval %d, %d MCUs); one lane reads "
                   "an interval, of at most %d blocks", who, per, o->restart_interval, D->g.mcus, QS_RD_MAX_INTERVAL_BLOCKS);
  for (int c = 0; c < n; ++c) {
    const int td = o->dc_tbl[c], ta = o->ac_tbl[c];
    if (td < 0 || td > 3 || ta < 0 || ta > 3)
      return qs_fail(QS_HIP_EINVAL, "%s: component %d names tables %d / %d (0 .. 3)", who, c, td, ta);
    if ((td > 1 && !o->has_dc[td]) || (ta > 1 && !o->has_ac[ta]))
      return qs_fail(QS_HIP_EINVAL, "%s: component %d uses a table the options do not hold (only 0 and 1 have a "
                     "standard table)", who, c);
    D->dc_tbl[c] = td;
    D->ac_tbl[c] = ta;
    if (int rc = check_block_count(job, c, who)) return rc;
  }
  if (tables) {
    for (int t = 0; t < 8; ++t) {
      const bool ac = t >= 4;
      const int id = t & 3;
      bool used = false;
      for (int c = 0; c < n; ++c) used |= (ac ? D->ac_tbl[c] : D->dc_tbl[c]) == id;
      if (!used) continue;                                          // (stays all zero: never looked at)
      qs_hip_huff_table tb;
      if (ac ? o->has_ac[id] : o->has_dc[id]) tb = ac ? o->ac[id] : o->dc[id];
      else if (int rc = qs_hip_huff_standard(ac, id, tb.bits, tb.huffval)) return rc;
      if (qr_build_table(tb.bits, tb.huffval, !ac, &D->tab[t]))
        return qs_fail(QS_HIP_EINVAL, "%s: %s table %d is not a valid Huffman table", who, ac ? "AC" : "DC", id);
    }
  }
  D->max_scan = qr_max_scan(D->g, D->intervals);
  if (info) {
    info->blocks_in_mcu = D->g.bpm;
    info->mcus = D->g.mcus;
    info->intervals = D->intervals;
    info->blocks_per_interval = per;
  }
  return QS_HIP_OK;
}

// S: null for the one-lane-per-interval route; the split route's descriptors otherwise
int describe_all(qs_hip_job* const* jobs, int njobs, const qs_hip_read_opts* const* opts, bool tables,
                 std::vector<QrJob>& D, std::vector<QrsJob>* S, qs_hip_read_info* info, uint64_t* total, const char* who) {
  if (!jobs || njobs < 1) return qs_fail(QS_HIP_EINVAL, "%s: %d jobs (at least one)", who, njobs);
  if (!opts) return qs_fail(QS_HIP_EINVAL, "%s: null opts", who);
  D.assign((size_t)njobs, QrJob());
  Layout L;
  L.take(descriptors_bytes(njobs));
  if (S) {
    S->assign((size_t)njobs, QrsJob());
    L.take(split_descriptors_bytes(njobs));
  }
  for (int i = 0; i < njobs; ++i) {
    if (int r = describe(jobs[i], opts[i], tables, S != nullptr, &D[(size_t)i], info ? &info[i] : nullptr, Who(who, i).s))
      return r;
    QrJob& J = D[(size_t)i];
    long long blocks = 0;
    for (int c = 0; c < J.g.ncomp; ++c) blocks += (long long)jobs[i]->wblk[c] * jobs[i]->hblk[c];
    J.nzwg = qr_zero_wgs(blocks);
    const uint64_t chunks = (J.max_scan + 32) / QS_RD_MCHUNK + 2;
    J.off_state = L.take(sizeof(QrState));
    J.off_cnt = L.take(chunks * 4);
    J.off_off = L.take(chunks * 4);
    J.off_p = L.take(((uint64_t)J.intervals + 1) * 8);
    if (S) {
      QrsJob& X = (*S)[(size_t)i];
      memset(&X, 0, sizeof X);
      qrs_describe(J, &X);
      X.max_segments = qrs_max_segments(J.max_scan, J.intervals);
      if (X.max_segments > 0x7fffff00ull)
        return qs_fail(QS_HIP_ENOTSUP, "%s: more than 2^31 segments of %d bytes in the longest scan of this geometry",
                       Who(who, i).s, QS_RD_SPLIT_BYTES);
      const uint64_t stiles = (X.max_segments + QS_RD_SPLIT_WG - 1) / QS_RD_SPLIT_WG;
      const uint64_t mtiles = ((uint64_t)J.g.mcus + QS_RD_SPLIT_WG - 1) / QS_RD_SPLIT_WG;
      X.off_nseg = L.take(4);
      X.off_seg0 = L.take(((uint64_t)J.intervals + 1) * 4);
      X.off_entry = L.take(X.max_segments * 8);
      X.off_exit = L.take(X.max_segments * 16);
      X.off_cnt = L.take(X.max_segments * 4);
      X.off_stile = L.take(stiles * 12);
      X.off_dcd = L.take((uint64_t)J.g.nblocks * 2);
      X.off_mtile = L.take(mtiles * 36);
    }
  }
  *total = L.total;
  return QS_HIP_OK;
}

}  // namespace

extern "C" int qs_hip_read_device_batch_info(qs_hip_job* const* jobs, int njobs, const qs_hip_read_opts* const* opts,
                                             qs_hip_read_info* per_job, size_t* bytes) {
  return guarded([&]() -> int {
    const char* who = "qs_hip_read_device_batch_info";
    if (!per_job || !bytes) return qs_fail(QS_HIP_EINVAL, "%s: null result", who);
    std::vector<QrJob> D;
    uint64_t total = 0;
    if (int r = describe_all(jobs, njobs, opts, false, D, nullptr, per_job, &total, who)) return r;
    *bytes = (size_t)total;
    return QS_HIP_OK;
  });
}

extern "C" int qs_hip_read_device_batch_prepare(qs_hip_job* const* jobs, int njobs, const qs_hip_read_opts* const* opts,
                                                void* d_workspace, size_t bytes, void* stream) {
  return guarded([&]() -> int {
    const char* who = "qs_hip_read_device_batch_prepare";
    std::vector<QrJob> D;
    uint64_t total = 0;
    if (int r = describe_all(jobs, njobs, opts, true, D, nullptr, nullptr, &total, who)) return r;
    if (int r = check_workspace(total, d_workspace, bytes, who)) return r;
    if (int r = device_ok()) return r;
    return upload(d_workspace, D, static_cast<hipStream_t>(stream));
  });
}

// The run sees no options, and reads nothing back from the workspace: the launch sizes that depend on the restart
// interval are bounded from the geometry instead (intervals <= MCUs).  A marker workgroup behind the descriptor's own
// clamp of the scan and a decode workgroup behind the job's intervals return at once.  split: the launches over
// segments are sized for the bytes at hand, no further than the longest segment of the geometry, with a segment more
// per MCU (an interval's last one may be short); a workgroup behind the segments the map kernel found returns at once.
static int run_read(qs_hip_job* const* jobs, int njobs, const uint8_t* const* d_scan, const uint64_t* scan_bytes,
                    int32_t* d_status, void* d_workspace, size_t bytes, void* stream, bool split, const char* who) {
  if (!jobs || njobs < 1) return qs_fail(QS_HIP_EINVAL, "%s: %d jobs (at least one)", who, njobs);
  if (!d_scan || !scan_bytes || !d_status) return qs_fail(QS_HIP_EINVAL, "%s: null argument", who);
  if (!workspace_ok(d_workspace, bytes, descriptors_bytes(njobs) + (split ? split_descriptors_bytes(njobs) : 0)))
    return qs_fail(QS_HIP_EINVAL, "%s: workspace of %zu bytes (256-byte aligned): not what prepare was given", who, bytes);
  if (int r = device_ok()) return r;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int j0 = 0; j0 < njobs; j0 += QS_RD_CHUNK) {
    QrsArgs x;
    memset(&x, 0, sizeof x);
    QrArgs& a = x.a;
    a.jobs = static_cast<const QrJob*>(d_workspace) + j0;
    a.ws = static_cast<uint8_t*>(d_workspace);
    a.d_status = d_status;
    a.job0 = j0;
    a.n = std::min(QS_RD_CHUNK, njobs - j0);
    x.sjobs = reinterpret_cast<const QrsJob*>(a.ws + descriptors_bytes(njobs)) + j0;
    long long zwgs = 0, mwgs = 0, dwgs = 0, swgs = 0, twgs = 0;
    for (int k = 0; k < a.n; ++k) {
      const qs_hip_job* job = jobs[j0 + k];
      const Who w(who, j0 + k);
      if (int rc = check_job(job, w.s)) return rc;
      if (!d_scan[j0 + k]) return qs_fail(QS_HIP_EINVAL, "%s: no scan bytes", w.s);
      QsEncGeom g;
      if (int rc = qr_geometry(job->ncomp, job->image_width, job->image_height, job->hsamp, job->vsamp, job->wblk,
                               job->hblk, &g))
        return qs_fail(rc == 2 ? QS_HIP_ENOTSUP : QS_HIP_EINVAL, "%s: not the geometry prepare saw", w.s);
      long long blocks = 0;
      QrPtrs& P = a.p[k];
      for (int c = 0; c < job->ncomp; ++c) {
        int16_t* arr = job->coef[c];
        if (int rc = check_array(arr, c, false, w.s)) return rc;
        if (int rc = check_block_count(job, c, w.s)) return rc;
        P.coef[c] = arr;
        P.nblk[c] = job->wblk[c] * job->hblk[c];
        blocks += P.nblk[c];
      }
      P.scan = d_scan[j0 + k];
      P.scan_bytes = scan_bytes[j0 + k];
      a.zwg0[k] = (int)zwgs;
      zwgs += qr_zero_wgs(blocks);                              // (the descriptor's nzwg: the same function)
      // the marker launches: a workgroup per 4 KiB of aligned memory the scan touches, no further than the longest
      // segment of the geometry (the intervals are at most the MCUs: an upper bound is all the clamp needs here; the
      // kernels clamp with the descriptor's exact value and leave the units behind it alone)
      const uint64_t n = std::min<uint64_t>(P.scan_bytes, qr_max_scan(g, g.mcus));
      const uint64_t units = ((reinterpret_cast<uintptr_t>(P.scan) & 15) + n + 15) / 16;
      a.mwg0[k] = (int)mwgs;
      mwgs += (long long)((units + QS_RD_WG - 1) / QS_RD_WG);
      a.dwg0[k] = (int)dwgs;
      dwgs += ceil_div(g.mcus, QS_RD_DWG);
      x.swg0[k] = (int)swgs;
      swgs += (long long)((qrs_max_segments(n, g.mcus) + QS_RD_SPLIT_WG - 1) / QS_RD_SPLIT_WG);
      x.twg0[k] = (int)twgs;
      twgs += ceil_div(g.mcus, QS_RD_SPLIT_WG);
      if (mwgs > 0x7fffffffLL || dwgs > 0x7fffffffLL || (split && swgs > 0x7fffffffLL))
        return qs_fail(QS_HIP_EINVAL, "%s: more than 2^31 workgroups in one launch", who);
    }
    if (split) qs_launch_read_split(x, (int)zwgs, (int)mwgs, (int)swgs, (int)twgs, s);
    else qs_launch_read(a, (int)zwgs, (int)mwgs, (int)dwgs, s);
  }
  HIP_TRY(hipGetLastError());
  return QS_HIP_OK;
}

extern "C" int qs_hip_read_device_batch(qs_hip_job* const* jobs, int njobs, const uint8_t* const* d_scan,
                                        const uint64_t* scan_bytes, int32_t* d_status, void* d_workspace, size_t bytes,
                                        void* stream) {
  return guarded([&]() -> int {
    return run_read(jobs, njobs, d_scan, scan_bytes, d_status, d_workspace, bytes, stream, false, "qs_hip_read_device_batch");
  });
}

// ---- the split route: the same three calls -----------------------------------------------------------------------------------

extern "C" int qs_hip_read_split_device_batch_info(qs_hip_job* const* jobs, int njobs, const qs_hip_read_opts* const* opts,
                                                   qs_hip_read_split_info* per_job, size_t* bytes) {
  return guarded([&]() -> int {
    const char* who = "qs_hip_read_split_device_batch_info";
    if (!per_job || !bytes) return qs_fail(QS_HIP_EINVAL, "%s: null result", who);
    std::vector<QrJob> D;
    std::vector<QrsJob> S;
    std::vector<qs_hip_read_info> info((size_t)std::max(njobs, 1));
    uint64_t total = 0;
    if (int r = describe_all(jobs, njobs, opts, false, D, &S, info.data(), &total, who)) return r;
    for (int i = 0; i < njobs; ++i) {
      per_job[i].blocks_in_mcu = info[(size_t)i].blocks_in_mcu;
      per_job[i].mcus = info[(size_t)i].mcus;
      per_job[i].intervals = info[(size_t)i].intervals;
      per_job[i].blocks_per_interval = info[(size_t)i].blocks_per_interval;
      per_job[i].max_segments = (int64_t)S[(size_t)i].max_segments;
    }
    *bytes = (size_t)total;
    return QS_HIP_OK;
  });
}

extern "C" int qs_hip_read_split_device_batch_prepare(qs_hip_job* const* jobs, int njobs,
                                                      const qs_hip_read_opts* const* opts, void* d_workspace, size_t bytes,
                                                      void* stream) {
  return guarded([&]() -> int {
    const char* who = "qs_hip_read_split_device_batch_prepare";
    std::vector<QrJob> D;
    std::vector<QrsJob> S;
    uint64_t total = 0;
    if (int r = describe_all(jobs, njobs, opts, true, D, &S, nullptr, &total, who)) return r;
    if (int r = check_workspace(total, d_workspace, bytes, who)) return r;
    if (int r = device_ok()) return r;
    if (int r = upload(d_workspace, D, static_cast<hipStream_t>(stream))) return r;
    return upload(static_cast<uint8_t*>(d_workspace) + descriptors_bytes(njobs), S, static_cast<hipStream_t>(stream));
  });
}

extern "C" int qs_hip_read_split_device_batch(qs_hip_job* const* jobs, int njobs, const uint8_t* const* d_scan,
                                              const uint64_t* scan_bytes, int32_t* d_status, void* d_workspace,
                                              size_t bytes, void* stream) {
  return guarded([&]() -> int {
    return run_read(jobs, njobs, d_scan, scan_bytes, d_status, d_workspace, bytes, stream, true,
                    "qs_hip_read_split_device_batch");
  });
}
