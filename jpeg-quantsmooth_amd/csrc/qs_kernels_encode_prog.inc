// qs_kernels_encode_prog.inc -- the progressive run's own kernels (qs_hip_encode_progressive_device_batch_files),
// included at the end of qs_kernels_encode.hip: they stand on its staging, sinks and scans, and the run drives its
// restart instantiations of qe_scan_bits, qe_ff_count and qe_stuff, and qe_init and qe_ff_scan, unchanged.  DESIGN.md
// section 17.
//
// The unit of work is a (job, scan) pair, a "scan job": a QsEncJob with the scan's own geometry, interval and workspace
// arrays, beside a QpScan with its band, point transform and framing.  Every array the shared kernels index by job
// (d_stop, d_len, d_status, codes, prefix, tstatus) is here an array of the scratch indexed by scan job.
//   qp_begin     per job: its d_stop for each of its scan jobs
//   qp_flags     AC scans: per block whether it writes and whether it ends in zeros; per workgroup its last head
//   qp_headscan  one workgroup per scan job: the last head in front of each workgroup
//   qp_runs      per block the EOB-run piece that ends there (qp_eob_after): written, counted and sized by that lane
//   qp_size      qe_size<HIST, true> with the DC-first / AC-first block coders and the run piece
//   qp_emit      qe_emit<true> with them
//   qp_frame     per job: scan offsets from the scans' lengths, d_len, d_status, and every byte outside the segments
//   qp_nofile    a workspace the run finds no prepare for: status 4
// Refinement scans (Ah > 0, section 17.1) have kernels of their own, launched for a chunk that holds one; the Ah = 0
// kernels above pass their scan jobs by, and the other way round:
//   qr_flags     AC refinement: per block QP_F_* and the number of correction bits it leaves buffered (its tail)
//   qr_wsum      per block its cut weight -- the tail, and QR_CORR_MAX + 1 where the next block is a head -- scanned
//                inside the workgroup
//   qr_wscan     one workgroup per scan job: the weights in front of each workgroup
//   qr_next      per block, by binary search on the scanned weights: where a run piece that starts there ends
//   qr_hop       pointer doubling from the run starts, one launch per round: marks where pieces do start
//   qp_size / qp_emit <REFINE>   the DC and AC refinement coders; a piece's symbol is written by its FIRST block
#include "qs_encode_prog.h"

void qs_launch_huff_tables(const QsHuffArgs& a, hipStream_t s);   // qs_kernels_huff.hip

namespace {

__device__ __forceinline__ int qp_per(const QsEncJob& J, int variant) {
  const QsEncGeom& g = J.g[variant];
  return (J.ri[variant] ? J.ri[variant] : g.mcus) * g.bpm;
}

__global__ void __launch_bounds__(64) qp_begin(QpJobArgs a) {
  const QpJob& Q = a.jobs[blockIdx.x];
  const int stop = a.d_stop ? a.d_stop[a.job0 + blockIdx.x] : 0;
  for (int s = threadIdx.x; s < Q.nscans; s += 64) a.sstop[Q.sj0 + s] = stop;
}

__global__ void __launch_bounds__(256) qp_nofile(uint64_t* d_len, int32_t* d_status, int njobs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < njobs) {
    d_len[i] = 0;
    d_status[i] = 4;
  }
}

// inclusive maximum over the workgroup's 256 lanes
__device__ int qp_maxscan(int v, uint32_t* sc) {
  const int t = threadIdx.x;
  int* m = reinterpret_cast<int*>(sc);
  m[t] = v;
  __syncthreads();
  for (int d = 1; d < QS_ENC_WG; d <<= 1) {
    const int x = t >= d ? m[t - d] : -1;
    __syncthreads();
    m[t] = max(m[t], x);
    __syncthreads();
  }
  const int r = m[t];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(QS_ENC_WG) qp_flags(QsEncArgs a, const QpScan* xs) {
  __shared__ QeShared S;
  const int wg = blockIdx.x, t = threadIdx.x;
  const int k = qe_find_job<false>(a, wg);
  const QsEncJob& J = a.jobs[k];
  const QpScan& X = xs[k];
  const int lw = wg - J.wg0;
  if (lw >= J.nwg || X.Ss == 0 || X.Ah) return;
  const int variant = qe_variant(a, J, k);
  qe_stage(a, J, k, variant, S);
  const int b = lw * QS_ENC_WG + t;
  uint32_t f = 0;
  int head = -1;
  if (b < S.g.nblocks) {
    QeBlock B;
    qe_load(S, J, b, 0, B);
    f = qp_ac_flags(B.v, X.Ss, X.Se, X.Al);
    if ((f & QP_F_WRITES) || b % qp_per(J, variant) == 0) head = b;
  }
  (a.ws + X.off_flags)[b] = (uint8_t)f;
  const int last = qp_maxscan(head, S.sc);
  if (t == QS_ENC_WG - 1) reinterpret_cast<int32_t*>(a.ws + X.off_wghead)[lw] = last;
}

__global__ void __launch_bounds__(QS_ENC_WG) qp_headscan(QsEncArgs a, const QpScan* xs) {
  __shared__ uint32_t sc[QS_ENC_WG];
  const int k = blockIdx.x, t = threadIdx.x;
  const QsEncJob& J = a.jobs[k];
  const QpScan& X = xs[k];
  if (X.Ss == 0 || X.Ah) return;
  const int32_t* wghead = reinterpret_cast<const int32_t*>(a.ws + X.off_wghead);
  int32_t* wgcarry = reinterpret_cast<int32_t*>(a.ws + X.off_wgcarry);
  int carry = -1;
  for (int base = 0; base < J.nwg; base += QS_ENC_WG) {
    const int i = base + t;
    const int mine = i < J.nwg ? wghead[i] : -1;
    const int inc = qp_maxscan(mine, sc);
    sc[t] = (uint32_t)inc;                             // the exclusive value: the inclusive one of the lane before
    __syncthreads();
    const int prev = t > 0 ? (int)sc[t - 1] : -1;
    const int total = (int)sc[QS_ENC_WG - 1];
    __syncthreads();
    if (i < J.nwg) wgcarry[i] = max(carry, prev);
    carry = max(carry, total);
  }
}

__global__ void __launch_bounds__(QS_ENC_WG) qp_runs(QsEncArgs a, const QpScan* xs) {
  __shared__ uint32_t sc[QS_ENC_WG];
  const int wg = blockIdx.x, t = threadIdx.x;
  const int k = qe_find_job<false>(a, wg);
  const QsEncJob& J = a.jobs[k];
  const QpScan& X = xs[k];
  const int lw = wg - J.wg0;
  if (lw >= J.nwg || X.Ss == 0 || X.Ah) return;
  const int variant = qe_variant(a, J, k);
  const int nblocks = J.g[variant].nblocks, per = qp_per(J, variant);
  const uint8_t* flags = a.ws + X.off_flags;
  const int b = lw * QS_ENC_WG + t;
  const bool live = b < nblocks;
  const uint32_t f = live ? flags[b] : 0;
  const int mine = (live && ((f & QP_F_WRITES) || b % per == 0)) ? b : -1;
  const int head = max(qp_maxscan(mine, sc), reinterpret_cast<const int32_t*>(a.ws + X.off_wgcarry)[lw]);
  int eob = 0;
  if (live && head >= 0) {                            // (block 0 starts an interval: a live block always has a head)
    const bool next_writes = b + 1 < nblocks && (flags[b + 1] & QP_F_WRITES);
    eob = qp_eob_after(b, head, flags[head], per, nblocks, next_writes);
  }
  reinterpret_cast<uint16_t*>(a.ws + X.off_eob)[b] = (uint16_t)eob;
}

// ---- refinement scans ----

__device__ __forceinline__ void qr_raw(QeSizeSink& s, uint32_t, int nb) { s.bits += (uint32_t)nb; }
__device__ __forceinline__ void qr_raw(QeHistSink&, uint32_t, int) {}
__device__ __forceinline__ void qr_raw(QeEmitSink& s, uint32_t val, int nb) { s.raw(val, nb); }
// the coder's sinks with raw(): bits without a symbol
template <class Base>
struct QrSink {
  Base& base;
  __device__ __forceinline__ void ac(int tb, int sym, uint32_t bits, int nb) { base.ac(tb, sym, bits, nb); }
  __device__ __forceinline__ void raw(uint32_t val, int nb) { qr_raw(base, val, nb); }
};

// the DC libjpeg sees at scan block b: a dummy block repeats the one before it (qe_dc)
__device__ __forceinline__ int qr_dc(const QeShared& S, int b) {
  const QsEncGeom& g = S.g;
  const int m = b / g.bpm, k = b - m * g.bpm;
  int c = 0;
  for (int ci = 1; ci < g.ncomp; ++ci)
    if (k >= g.first[ci]) c = ci;
  return qe_dc(S, m, c, k - g.first[c]);
}

// this workgroup's place in an AC refinement scan job of the chunk: false when it has none
struct QrAt {
  int k, lw, variant, nblocks, per;
};
__device__ __forceinline__ bool qr_at(const QsEncArgs& a, const QpScan* xs, QrAt& q) {
  q.k = qe_find_job<false>(a, blockIdx.x);
  const QsEncJob& J = a.jobs[q.k];
  const QpScan& X = xs[q.k];
  q.lw = (int)blockIdx.x - J.wg0;
  if (q.lw >= J.nwg || X.Ss == 0 || !X.Ah) return false;
  q.variant = qe_variant(a, J, q.k);
  q.nblocks = J.g[q.variant].nblocks;
  q.per = qp_per(J, q.variant);
  return true;
}

__global__ void __launch_bounds__(QS_ENC_WG) qr_flags(QsEncArgs a, const QpScan* xs) {
  __shared__ QeShared S;
  QrAt q;
  if (!qr_at(a, xs, q)) return;
  const QsEncJob& J = a.jobs[q.k];
  const QpScan& X = xs[q.k];
  qe_stage(a, J, q.k, q.variant, S);
  const int b = q.lw * QS_ENC_WG + threadIdx.x;
  uint32_t f = 0;
  if (b < q.nblocks) {
    QeBlock B;
    qe_load(S, J, b, 0, B);
    QrNullSink none;
    QrBits tail;
    f = qr_ac_refine(B.v, X.Ss, X.Se, X.Al, 0, none, &tail);
    f |= (uint32_t)tail.n << 2;
  }
  (a.ws + X.off_flags)[b] = (uint8_t)f;
}

// a head: a block that writes or starts a restart interval; no piece runs into it
__device__ __forceinline__ bool qr_head(const uint8_t* flags, int b, int per) {
  return (flags[b] & QP_F_WRITES) || b % per == 0;
}

__global__ void __launch_bounds__(QS_ENC_WG) qr_wsum(QsEncArgs a, const QpScan* xs) {
  __shared__ uint32_t sc[QS_ENC_WG];
  QrAt q;
  if (!qr_at(a, xs, q)) return;
  const QpScan& X = xs[q.k];
  const uint8_t* flags = a.ws + X.off_flags;
  const int b = q.lw * QS_ENC_WG + threadIdx.x;
  uint32_t w = 0;
  if (b < q.nblocks) {
    const uint32_t f = flags[b];
    if (f & QP_F_ENDZ) w = f >> 2;
    if (b + 1 < q.nblocks && qr_head(flags, b + 1, q.per)) w += QR_CORR_MAX + 1;   // any piece that reaches b ends there
  }
  uint32_t total;
  const uint32_t ex = qe_exscan(w, sc, &total);
  reinterpret_cast<uint32_t*>(a.ws + X.off_w)[b] = ex;
  if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(a.ws + X.off_wghead)[q.lw] = total;
}

// (sums modulo 2^32: qr_next takes differences over at most QP_EOB_MAX blocks, which are far below that)
__global__ void __launch_bounds__(QS_ENC_WG) qr_wscan(QsEncArgs a, const QpScan* xs) {
  __shared__ uint32_t sc[QS_ENC_WG];
  const int k = blockIdx.x, t = threadIdx.x;
  const QsEncJob& J = a.jobs[k];
  const QpScan& X = xs[k];
  if (X.Ss == 0 || !X.Ah) return;
  const uint32_t* wsum = reinterpret_cast<const uint32_t*>(a.ws + X.off_wghead);
  uint32_t* woff = reinterpret_cast<uint32_t*>(a.ws + X.off_wgcarry);
  uint32_t carry = 0;
  for (int base = 0; base < J.nwg; base += QS_ENC_WG) {
    const int i = base + t;
    uint32_t total;
    const uint32_t ex = qe_exscan(i < J.nwg ? wsum[i] : 0, sc, &total);
    if (i < J.nwg) woff[i] = carry + ex;
    carry += total;
  }
}

// A piece that starts at block b takes blocks until the EOB run reaches QP_EOB_MAX or the buffered bits pass QR_CORR_MAX
// (jchuff.c: the check follows the block that was added), and never runs into a head: the first j >= b whose weights
// from b on pass QR_CORR_MAX, at most QP_EOB_MAX blocks on.  The search takes 15 steps whatever the data.
__global__ void __launch_bounds__(QS_ENC_WG) qr_next(QsEncArgs a, const QpScan* xs) {
  QrAt q;
  if (!qr_at(a, xs, q)) return;
  const QpScan& X = xs[q.k];
  const uint8_t* flags = a.ws + X.off_flags;
  const uint32_t* W = reinterpret_cast<const uint32_t*>(a.ws + X.off_w);
  const uint32_t* woff = reinterpret_cast<const uint32_t*>(a.ws + X.off_wgcarry);
  const int b = q.lw * QS_ENC_WG + threadIdx.x;
  int jump = b, len = 0, start = 0;
  if (b < q.nblocks && (flags[b] & QP_F_ENDZ)) {
    const uint32_t w0 = W[b] + woff[b / QS_ENC_WG];
    int lo = b, hi = min(b + QP_EOB_MAX - 1, q.nblocks - 1);
    for (int it = 0; it < 15; ++it)
      if (lo < hi) {
        const int mid = (lo + hi) >> 1;             // (mid + 1 <= hi: a block of the scan)
        if (W[mid + 1] + woff[(mid + 1) / QS_ENC_WG] - w0 > QR_CORR_MAX) hi = mid;
        else lo = mid + 1;
      }
    len = lo - b + 1;
    const int nx = lo + 1;
    if (nx < q.nblocks && !qr_head(flags, nx, q.per)) jump = nx;   // (else the run ends with this piece: it points at itself)
    // a run starts at a head that leaves a tail, or behind one that leaves none (every other block leaves one)
    start = qr_head(flags, b, q.per) || !(flags[b - 1] & QP_F_ENDZ);
  }
  if (b < q.nblocks) {
    reinterpret_cast<int32_t*>(a.ws + X.off_jump[0])[b] = jump;
    reinterpret_cast<uint16_t*>(a.ws + X.off_eob)[b] = (uint16_t)len;
    (a.ws + X.off_reach)[b] = (uint8_t)start;
  }
}

// Round `round`: in[b] is 2^round pieces on from b.  Every marked block marks in[b], then the distance doubles.  A block
// marked in this same round may or may not be seen: whatever it marks is a piece start too, 2^round pieces on from one
__global__ void __launch_bounds__(QS_ENC_WG) qr_hop(QsEncArgs a, const QpScan* xs, int round) {
  QrAt q;
  if (!qr_at(a, xs, q)) return;
  const QpScan& X = xs[q.k];
  const int32_t* in = reinterpret_cast<const int32_t*>(a.ws + X.off_jump[round & 1]);
  int32_t* out = reinterpret_cast<int32_t*>(a.ws + X.off_jump[(round & 1) ^ 1]);
  uint8_t* reach = a.ws + X.off_reach;
  const int b = q.lw * QS_ENC_WG + threadIdx.x;
  if (b >= q.nblocks) return;
  const int j = in[b];
  out[b] = in[j];
  if (j != b && reach[b]) reach[j] = 1;
}

template <class Sink>
__device__ __forceinline__ uint32_t qr_encode(const uint8_t* ws, const QpScan& X, const QeShared& S, const QeBlock& B, int b,
                                              Sink& base) {
  QrSink<Sink> s{base};
  if (X.Ss == 0) {
    qr_dc_refine(qr_dc(S, b), X.Al, s);
    return 0;
  }
  const int piece = (ws + X.off_reach)[b] ? reinterpret_cast<const uint16_t*>(ws + X.off_eob)[b] : 0;
  qr_ac_block(B.v, X.Ss, X.Se, X.Al, X.actb, piece, s);
  return 0;                                          // (no range check in a refinement scan)
}

// the block's own symbols and the run piece behind them, on any sink
template <class Sink>
__device__ __forceinline__ uint32_t qp_encode(const QsEncArgs& a, const QpScan& X, const QeBlock& B, int b, Sink& s) {
  if (X.Ss == 0) {
    // qe_load's difference is DC - previous DC (0 for a dummy block, which repeats it): shift both
    const int cur = B.v[0], prev = cur - B.diff;
    return qp_dc_first((cur >> X.Al) - (prev >> X.Al), B.tb, s);
  }
  const uint32_t flags = qp_ac_first(B.v, X.Ss, X.Se, X.Al, X.actb, s);
  const int eob = reinterpret_cast<const uint16_t*>(a.ws + X.off_eob)[b];
  if (eob) qp_eobrun(eob, X.actb, s);
  return flags;
}

template <bool REFINE, class Sink>
__device__ __forceinline__ uint32_t qp_code(const QsEncArgs& a, const QpScan& X, const QeShared& S, const QeBlock& B, int b,
                                            Sink& s) {
  if constexpr (REFINE) return qr_encode(a.ws, X, S, B, b, s);
  else return qp_encode(a, X, B, b, s);
}

template <bool HIST, bool REFINE>
__global__ void __launch_bounds__(QS_ENC_WG) qp_size(QsEncArgs a, const QpScan* xs) {
  __shared__ QeShared S;
  __shared__ uint32_t hist[HIST ? 4 * 257 : 1];
  const int wg = blockIdx.x, t = threadIdx.x;
  const int k = qe_find_job<false>(a, wg);
  const QsEncJob& J = a.jobs[k];
  const QpScan& X = xs[k];
  const int lw = wg - J.wg0;
  if (lw >= J.nwg || (X.Ah != 0) != REFINE) return;
  if (HIST)
    for (int i = t; i < 4 * 257; i += QS_ENC_WG) hist[i] = 0;
  const int variant = qe_variant(a, J, k);
  qe_stage(a, J, k, variant, S);
  const int b = lw * QS_ENC_WG + t;
  uint32_t bits = 0, flags = 0;
  if (b < S.g.nblocks) {
    QeBlock B;
    if (!REFINE || X.Ss != 0) qe_load(S, J, b, J.ri[variant], B);   // (a DC refinement reads the DC alone: qr_dc)
    if (HIST) {
      QeHistSink s{hist};
      flags = qp_code<REFINE>(a, X, S, B, b, s);
    } else {
      QeSizeSink s(S);
      flags = qp_code<REFINE>(a, X, S, B, b, s) | s.flags;
      bits = s.bits;
    }
  }
  if (flags) atomicOr(&qe_state(a, J)->flags, flags);
  if (HIST) {
    __syncthreads();
    uint32_t* h = a.d_counts + (size_t)(a.job0 + k) * 4 * 257;
    for (int i = t; i < 4 * 257; i += QS_ENC_WG)
      if (hist[i] && i % 257 != 256) atomicAdd(&h[i], hist[i]);
  } else {
    reinterpret_cast<uint16_t*>(a.ws + J.off_bits)[b] = (uint16_t)bits;      // at most QP_MAXBITS
    uint32_t total;
    const uint32_t ex = qe_exscan(bits, S.sc, &total);
    if (t == 0) reinterpret_cast<uint32_t*>(a.ws + J.off_wgsum)[lw] = total;
    if (b < S.g.nblocks) {                           // where an interval starts inside its workgroup
      const int per = qe_per(S, J, variant);
      if (b % per == 0) reinterpret_cast<uint32_t*>(a.ws + J.off_rrel)[b / per] = ex;
    }
  }
}

template <bool REFINE>
__global__ void __launch_bounds__(QS_ENC_WG) qp_emit(QsEncArgs a, const QpScan* xs) {
  constexpr uint32_t LDS_WORDS = QP_LDS_WORDS;
  __shared__ QeShared S;
  __shared__ uint32_t words[LDS_WORDS];
  const int wg = blockIdx.x, t = threadIdx.x;
  const int k = qe_find_job<false>(a, wg);
  const QsEncJob& J = a.jobs[k];
  const QpScan& X = xs[k];
  const int lw = wg - J.wg0;
  if (lw >= J.nwg || (X.Ah != 0) != REFINE) return;
  if (qe_state(a, J)->dead) return;
  uint32_t wgbits = reinterpret_cast<const uint32_t*>(a.ws + J.off_wgsum)[lw];
  if (wgbits == 0) return;
  uint64_t s0 = reinterpret_cast<const uint64_t*>(a.ws + J.off_wgoff)[lw];
  const int variant = qe_variant(a, J, k);
  const uint64_t* rd = reinterpret_cast<const uint64_t*>(a.ws + J.off_rd);
  const QsEncGeom& g = J.g[variant];
  const int per = qp_per(J, variant);
  auto ends = [&](int blk, int nblocks) { return (blk + 1) % per == 0 || blk == nblocks - 1; };
  const int b0 = lw * QS_ENC_WG, bl = min(b0 + QS_ENC_WG, g.nblocks) - 1;
  const uint64_t d0 = rd[b0 / per];
  s0 += d0;
  wgbits += (uint32_t)(rd[bl / per + (ends(bl, g.nblocks) ? 1 : 0)] - d0);
  const uint32_t lead = (uint32_t)(s0 & 31);
  const uint32_t nwords = (lead + wgbits + 31) >> 5;          // <= LDS_WORDS: a block has at most QP_MAXBITS
  for (uint32_t i = t; i < nwords && i < LDS_WORDS; i += QS_ENC_WG) words[i] = 0;
  qe_stage(a, J, k, variant, S);                              // (its barrier also covers the zeroing)
  const int b = b0 + t;
  const uint32_t mine = reinterpret_cast<const uint16_t*>(a.ws + J.off_bits)[b];
  uint32_t total;
  const uint32_t ex = qe_exscan(mine, S.sc, &total);
  if (b < S.g.nblocks && (mine || ends(b, S.g.nblocks))) {    // (a block without bits can still own an interval's padding)
    const int r = b / per;
    const uint64_t d = rd[r];
    const uint32_t shift = (uint32_t)(d - d0);
    const uint32_t pad = ends(b, S.g.nblocks) ? (uint32_t)(rd[r + 1] - d) : 0;
    QeEmitSink s(S, words, lead + ex + shift, LDS_WORDS);
    if (mine) {
      QeBlock B;
      if (!REFINE || X.Ss != 0) qe_load(S, J, b, J.ri[variant], B);
      qp_code<REFINE>(a, X, S, B, b, s);
    }
    if (pad) s.raw((1u << pad) - 1u, (int)pad);
    s.flush();
  }
  __syncthreads();
  uint32_t* raw = reinterpret_cast<uint32_t*>(a.ws + J.off_raw);
  const uint64_t w0 = s0 >> 5;
  const bool tail_shared = ((s0 + wgbits) & 31) != 0;
  for (uint32_t i = t; i < nwords && i < LDS_WORDS; i += QS_ENC_WG) {
    const uint64_t gw = w0 + i;
    if (gw * 4 + 4 > J.raw_cap) continue;
    const uint32_t v = __builtin_bswap32(words[i]);           // the stream is bytes, most significant bit first
    if ((i == 0 && lead) || (i == nwords - 1 && tail_shared)) atomicOr(&raw[gw], v);
    else raw[gw] = v;
  }
}

// bytes of the DHT marker of table w of a scan job's tables (the table kernel's: bits[17], huffval[256] each)
__device__ uint32_t qp_dht_bytes(const uint8_t* tabs, int w) {
  uint32_t n = 0;
  for (int l = 1; l <= 16; ++l) n += tabs[w * QS_ENC_TABLE_BYTES + l];
  return 5 + 16 + (n > 256 ? 256 : n);
}

__global__ void __launch_bounds__(256) qp_frame(QpJobArgs a) {
  __shared__ uint64_t at[QP_MAX_SCANS];               // where each scan's first DHT marker starts
  __shared__ uint64_t len_s;
  __shared__ int status_s;
  const int k = blockIdx.x, t = threadIdx.x;
  const QpJob& Q = a.jobs[k];
  const size_t job = (size_t)(a.job0 + k);
  const QpFramePtrs& F = a.f[k];
  const int v = (Q.two && a.d_stop && a.d_stop[job] != 0) ? 1 : 0;
  const int ns = min(Q.nscans, QP_MAX_SCANS);
  if (t == 0) {
    // the files call's precedence: 1, then 5, then 3 (which optimal tables cannot give), then capacity
    int st = 0;
    for (int s = 0; s < ns; ++s) {
      const int x = a.sstatus[Q.sj0 + s];
      const int rank_x = x == 1 ? 4 : x == 5 ? 3 : x == 3 ? 2 : x ? 1 : 0, rank_s = st == 1 ? 4 : st == 5 ? 3 : st == 3 ? 2 : st ? 1 : 0;
      if (rank_x > rank_s) st = x;
    }
    uint64_t pos = F.head_bytes[v];
    for (int s = 0; s < ns; ++s) {
      const int sj = Q.sj0 + s;
      const QpScan& X = a.scans[sj];
      at[s] = pos;
      const uint8_t* tabs = a.tables + (size_t)sj * QS_ENC_TABLES_BYTES;
      for (int i = 0; i < X.ntab; ++i) pos += qp_dht_bytes(tabs, X.tab[i]);
      pos += X.mid_bytes[v];
      a.prefix[sj] = (st != 0 && st != 2) ? F.cap : pos;   // a job without a file: its segments are stored nowhere
      pos += a.seglen[sj];
    }
    pos += 2;
    if (!st && pos > F.cap) st = 2;
    a.d_len[job] = (st == 0 || st == 2) ? pos : 0;
    a.d_status[job] = st;
    len_s = pos;
    status_s = st;
  }
  __syncthreads();
  if (status_s != 0 && status_s != 2) return;
  const uint64_t cap = F.cap;
  auto put = [&](uint64_t p, uint8_t b) {
    if (p < cap) F.out[p] = b;                       // nothing is written at or beyond the capacity
  };
  for (uint32_t p = t; p < F.head_bytes[v]; p += 256) put(p, F.head[v][p]);
  for (int s = 0; s < ns; ++s) {
    const int sj = Q.sj0 + s;
    const QpScan& X = a.scans[sj];
    const uint8_t* tabs = a.tables + (size_t)sj * QS_ENC_TABLES_BYTES;
    uint64_t pos = at[s];
    for (int i = 0; i < X.ntab; ++i) {
      const int w = X.tab[i];
      const uint8_t* tb = tabs + w * QS_ENC_TABLE_BYTES;
      const uint32_t nb = qp_dht_bytes(tabs, w), nsym = nb - 21, len = 2 + 1 + 16 + nsym;
      for (uint32_t p = t; p < nb; p += 256) {
        const uint8_t byte = p == 0 ? 0xff : p == 1 ? 0xc4 : p == 2 ? (uint8_t)(len >> 8) : p == 3 ? (uint8_t)len
                           : p == 4 ? (uint8_t)(((w >> 1) << 4) | (w & 1)) : p < 21 ? tb[1 + (p - 5)] : tb[17 + (p - 21)];
        put(pos + p, byte);
      }
      pos += nb;
    }
    const uint8_t* mid = a.ws + X.off_mid[v];
    for (uint32_t p = t; p < X.mid_bytes[v]; p += 256) put(pos + p, mid[p]);
  }
  if (t < 2) put(len_s - 2 + t, t ? 0xd9 : 0xff);
}

}  // namespace

// The progressive run.  Per chunk of scan jobs (`a`, with d_counts / codes / tstatus / d_len / d_status / d_stop set to
// the scratch arrays): everything up to each scan's stuffed length; qs_launch_encode_prog_stuff stores the segments once
// qp_frame has placed them.
// refine: -1 when the chunk holds no refinement scan, else the rounds of qr_hop its longest run of an AC refinement scan
// needs (from the geometry: qp_refine_rounds)
void qs_launch_encode_prog(const QsEncArgs& a, const QpScan* xs, const QsHuffArgs& h, int wgs, int swgs, int refine,
                           hipStream_t s) {
  const dim3 lanes(QS_ENC_WG);
  QsEncArgs hist = a;                                // the histogram pass: counts, and no code words yet
  hist.codes = nullptr;
  hist.tstatus = nullptr;
  hipLaunchKernelGGL(qe_init, dim3(a.n), lanes, 0, s, hist);
  if (wgs > 0) {
    hipLaunchKernelGGL(qp_flags, dim3(wgs), lanes, 0, s, a, xs);
    hipLaunchKernelGGL(qp_headscan, dim3(a.n), lanes, 0, s, a, xs);
    hipLaunchKernelGGL(qp_runs, dim3(wgs), lanes, 0, s, a, xs);
    hipLaunchKernelGGL((qp_size<true, false>), dim3(wgs), lanes, 0, s, hist, xs);
  }
  if (wgs > 0 && refine >= 0) {
    hipLaunchKernelGGL(qr_flags, dim3(wgs), lanes, 0, s, a, xs);
    hipLaunchKernelGGL(qr_wsum, dim3(wgs), lanes, 0, s, a, xs);
    hipLaunchKernelGGL(qr_wscan, dim3(a.n), lanes, 0, s, a, xs);
    hipLaunchKernelGGL(qr_next, dim3(wgs), lanes, 0, s, a, xs);
    for (int r = 0; r < refine; ++r) hipLaunchKernelGGL(qr_hop, dim3(wgs), lanes, 0, s, a, xs, r);
    hipLaunchKernelGGL((qp_size<true, true>), dim3(wgs), lanes, 0, s, hist, xs);
  }
  qs_launch_huff_tables(h, s);
  QsEncArgs code = a;
  code.d_counts = nullptr;
  if (wgs > 0) hipLaunchKernelGGL((qp_size<false, false>), dim3(wgs), lanes, 0, s, code, xs);
  if (wgs > 0 && refine >= 0) hipLaunchKernelGGL((qp_size<false, true>), dim3(wgs), lanes, 0, s, code, xs);
  hipLaunchKernelGGL(qe_scan_bits<true>, dim3(a.n), lanes, 0, s, code);
  if (wgs > 0) hipLaunchKernelGGL(qp_emit<false>, dim3(wgs), lanes, 0, s, code, xs);
  if (wgs > 0 && refine >= 0) hipLaunchKernelGGL(qp_emit<true>, dim3(wgs), lanes, 0, s, code, xs);
  if (swgs > 0) hipLaunchKernelGGL(qe_ff_count<true>, dim3(swgs), lanes, 0, s, code);
  hipLaunchKernelGGL(qe_ff_scan, dim3(a.n), lanes, 0, s, code);
}

void qs_launch_encode_prog_stuff(const QsEncArgs& a, int swgs, hipStream_t s) {
  if (swgs > 0) hipLaunchKernelGGL(qe_stuff<true>, dim3(swgs), dim3(QS_ENC_WG), 0, s, a);
}

void qs_launch_encode_prog_begin(const QpJobArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(qp_begin, dim3(a.n), dim3(64), 0, s, a);
}

void qs_launch_encode_prog_frame(const QpJobArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(qp_frame, dim3(a.n), dim3(256), 0, s, a);
}

void qs_launch_encode_prog_nofile(uint64_t* d_len, int32_t* d_status, int njobs, hipStream_t s) {
  hipLaunchKernelGGL(qp_nofile, dim3((njobs + 255) / 256), dim3(256), 0, s, d_len, d_status, njobs);
}
