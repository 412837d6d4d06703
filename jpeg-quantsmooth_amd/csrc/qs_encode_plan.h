// qs_encode_plan.h -- what the host drivers of the entropy coder share (qs_encode_job.cpp: baseline scans and files,
// qs_encode_prog_job.cpp: progressive files; DESIGN.md sections 13 and 17): the restart rule, the registry of prepared
// workspaces, the workspace arrays of one coded scan and the whole-file run's scratch.  A coded scan is a job of the
// baseline route and a (job, scan) pair of the progressive one.  Host only.  The first part needs qs_encode.h alone
// (tests/encode_plan_host.cpp compiles it without HIP); the second is the drivers', included after qs_stage.h.
#pragma once
#include "qs_encode.h"

#include <algorithm>
#include <memory>
#include <mutex>
#include <unordered_map>

// jcmaster.c (per_scan_setup): restart_in_rows wins and is counted in the geometry's MCU rows, limited to 16 bits.
// -> the interval the kernels work with: 0 where no marker is written (none asked for, or one interval covers the scan);
// *dri: what a DRI marker in front of the scan carries
static inline int qs_enc_restart(int restart_interval, int restart_in_rows, const QsEncGeom& g, int* dri = nullptr) {
  long long ri = restart_interval;
  if (restart_in_rows > 0) ri = (long long)restart_in_rows * g.mcus_x;
  if (restart_in_rows > 0 && ri > 65535) ri = 65535;
  if (dri) *dri = (int)ri;
  return ri >= g.mcus ? 0 : (int)ri;
}

// What a prepare call leaves for the run calls, which have no options: by workspace address, at most `cap` entries.
// Past the cap the one stored longest ago goes, and its workspace runs as one never prepared until it is prepared again.
// One instance per route: an address may be prepared for one route and then the other.
template <class T> class QsPrepared {
 public:
  explicit QsPrepared(size_t cap) : cap_(cap) {}
  void store(const void* d_workspace, T v) {
    std::lock_guard<std::mutex> lock(mutex_);
    map_[d_workspace] = Entry{std::make_shared<const T>(std::move(v)), ++clock_};
    if (map_.size() > cap_) {
      auto oldest = map_.begin();
      for (auto it = map_.begin(); it != map_.end(); ++it)
        if (it->second.age < oldest->second.age) oldest = it;
      map_.erase(oldest);
    }
  }
  // (shared, and the lock held for the lookup alone: a run makes its launches outside it, also while a prepare replaces the entry)
  std::shared_ptr<const T> find(const void* d_workspace) {
    std::lock_guard<std::mutex> lock(mutex_);
    auto it = map_.find(d_workspace);
    return it == map_.end() ? nullptr : it->second.v;
  }

 private:
  struct Entry {
    std::shared_ptr<const T> v;
    uint64_t age;
  };
  const size_t cap_;
  std::mutex mutex_;
  uint64_t clock_ = 0;
  std::unordered_map<const void*, Entry> map_;
};

#ifdef HIP_TRY   // ---- the drivers' part (qs_common.h, qs_stage.h) ----

// describe() of qs_encode_job.cpp for the progressive driver, which judges the MCU size scan by scan
int qs_enc_describe(const qs_hip_job* job, QsEncJob* D, QsEncPtrs* P, bool need_arrays, const char* who);

static inline int qs_enc_check_restart(int restart_interval, int restart_in_rows, const char* who, int job) {
  if (restart_interval < 0 || restart_interval > 65535 || restart_in_rows < 0)
    return qs_fail(QS_HIP_EINVAL, "%s: job %d: restart_interval %d (0 .. 65535), restart_in_rows %d (0 or more)", who, job,
                   restart_interval, restart_in_rows);
  return QS_HIP_OK;
}

// The workspace arrays of one coded scan (J.g, J.two, J.ri filled in): block code lengths, workgroup sums and offsets,
// the unstuffed stream at its worst-case size, the stuffing counts, the restart intervals' offsets.  nblocks / nint: the
// blocks and the restart intervals of the scan at most (over its variants), maxbits: the longest code of one block;
// wgs / swgs: the workgroups of the launch chunk so far.  swg_of_raw: the stuffing grid follows raw_cap (false:
// the size without the intervals' padding, for a run call that derives its grid without the options)
static inline int qs_enc_scan_layout(Layout& L, QsEncJob& J, long long& wgs, long long& swgs, int nblocks, uint64_t nint,
                                     uint64_t maxbits, bool swg_of_raw, const char* who) {
  J.nwg = ceil_div(nblocks, QS_ENC_WG);
  J.wg0 = (int)wgs;
  wgs += J.nwg;
  const uint64_t slots = (uint64_t)J.nwg * QS_ENC_WG;
  const uint64_t plain_cap = align_up((slots * maxbits + 7) / 8, 16) + 16;
  J.raw_cap = plain_cap + align_up(nint - 1, 16);                   // less than a byte of padding per interval end
  const uint64_t chunks = (J.raw_cap + QS_ENC_SCHUNK - 1) / QS_ENC_SCHUNK;
  J.nswg = (int)std::min<uint64_t>(swg_of_raw ? chunks : (plain_cap + QS_ENC_SCHUNK - 1) / QS_ENC_SCHUNK, QS_ENC_SWG_MAX);
  J.swg0 = (int)swgs;
  swgs += J.nswg;
  if (wgs > 0x7fffffffLL) return qs_fail(QS_HIP_EINVAL, "%s: more than 2^31 workgroups in one launch", who);
  J.off_state = L.take(sizeof(QsEncState));
  J.off_bits = L.take(slots * 2);
  J.off_wgsum = L.take((uint64_t)J.nwg * 4);
  J.off_wgoff = L.take((uint64_t)J.nwg * 8);
  J.off_raw = L.take(J.raw_cap);
  J.off_ffcnt = L.take(chunks * 4);
  J.off_ffoff = L.take(chunks * 8);
  J.off_rrel = L.take(nint * 4);
  J.off_rd = L.take((nint + 1) * 8);
  J.off_rp = L.take((nint + 1) * 8);
  return QS_HIP_OK;
}

// the whole-file run's scratch: byte offsets of its arrays, each indexed by coded scan (a route with more arrays takes
// them from L and sets total again)
struct QsEncScratch {
  uint64_t counts, codes, tables, prefix, tstatus, total;
  Layout L;
  explicit QsEncScratch(uint64_t n) {
    counts = L.take(n * 4 * 257 * 4);
    codes = L.take(n * QS_ENC_CODES * 4);
    tables = L.take(n * QS_ENC_TABLES_BYTES);
    prefix = L.take(n * 8);
    tstatus = L.take(n * 4);
    total = L.total;
  }
};

static inline void qs_enc_huff_scratch(QsHuffArgs& h, uint8_t* sc, const QsEncScratch& S) {
  h.counts = reinterpret_cast<uint32_t*>(sc + S.counts);
  h.codes = reinterpret_cast<uint32_t*>(sc + S.codes);
  h.tables = sc + S.tables;
  h.prefix = reinterpret_cast<uint64_t*>(sc + S.prefix);
  h.tstatus = reinterpret_cast<int32_t*>(sc + S.tstatus);
}
#endif
