// qs_kernels_read_split.hip -- the split route of the device scan reader (gfx950): every restart interval, or the
// whole scan of a file without markers, cut into segments of QS_RD_SPLIT_BYTES bytes, one lane per segment.  Same
// output as qs_kernels_read.hip; qs_read_split.h states the method and the bounds, DESIGN.md section 14 the numbers.
//
// Behind the init and marker kernels of qs_kernels_read.hip (the scan's end, status 1, P[r]) a run enqueues, per chunk
// of jobs and with every dependency between workgroups at a kernel boundary:
//   qrs_map        one workgroup per job: the segments of each interval and their exclusive scan, seg0[r]
//   qrs_decode     a lane per segment, QS_RD_SPLIT_ROUNDS + 1 launches: the speculative pass from the guessed entries,
//                  then the rounds -- a lane takes the exit its left neighbour wrote in the launch before and decodes
//                  again only if that differs from the entry it used; exits are double-buffered, so the result does
//                  not depend on the order the workgroups run in
//   qrs_count      every link checked (status 4); per tile of 256 segments the blocks completed behind the tile's
//                  last interval start
//   qrs_tile_scan  one workgroup per job: the segmented scan of the tiles' sums (also used by the DC pass)
//   qrs_write      a lane per segment, from its proved entry and its first block index: non-zero AC values into the
//                  arrays, DC differences into the scan-order side buffer; statuses 2 and 3
//   qrs_dc_tiles, qrs_tile_scan, qrs_dc_write   a lane per MCU: the differences summed per component from the
//                  interval's start, mod 2^16, and stored as the blocks' DC
// No lane waits for another, no loop's trip count depends on decoded data, and a workgroup behind a job's segments
// returns at once.
#include <hip/hip_runtime.h>
#include "qs_read_split.h"

void qs_launch_read_markers(const QrArgs& a, int zwgs, int mwgs, hipStream_t s);

namespace {

__device__ int qrs_find_job(const int32_t* first, int n, int wg) {
  int k = 0;
  for (int i = 1; i < n; ++i)
    if (wg >= first[i]) k = i;
  return k;
}

__device__ QrState* qrs_state(const QrsArgs& x, const QrJob& J) { return reinterpret_cast<QrState*>(x.a.ws + J.off_state); }

// the bytes of job k up to the scan's end
__device__ QrSrc qrs_src(const QrsArgs& x, const QrJob& J, int k) {
  QrSrc s;
  s.p = x.a.p[k].scan;
  s.n = x.a.p[k].scan_bytes < J.max_scan ? x.a.p[k].scan_bytes : J.max_scan;
  const uint64_t end = qrs_state(x, J)->end;
  if (end < s.n) s.n = end;
  return s;
}

__device__ QrsBufs qrs_bufs(const QrsArgs& x, const QrsJob& S) {
  QrsBufs B;
  uint8_t* ws = x.a.ws;
  B.nseg = reinterpret_cast<uint32_t*>(ws + S.off_nseg);
  B.seg0 = reinterpret_cast<uint32_t*>(ws + S.off_seg0);
  B.entry = reinterpret_cast<uint64_t*>(ws + S.off_entry);
  B.exit[0] = reinterpret_cast<uint64_t*>(ws + S.off_exit);
  B.exit[1] = B.exit[0] + S.max_segments;
  B.cnt = reinterpret_cast<uint32_t*>(ws + S.off_cnt);
  B.dcd = reinterpret_cast<int16_t*>(ws + S.off_dcd);
  return B;
}

// Inclusive scan over the workgroup's lanes; a lane whose flag is set starts a new sum.  Leaves the inclusive sums in
// sv and, in sf, whether a flag lies at or in front of the lane.
__device__ void qrs_wg_scan(uint32_t v, uint32_t f, uint32_t* sv, uint32_t* sf) {
  const int t = threadIdx.x;
  __syncthreads();                                                // (whoever still reads what the call before left)
  sv[t] = v;
  sf[t] = f;
  __syncthreads();
  for (int d = 1; d < QS_RD_SPLIT_WG; d <<= 1) {
    const uint32_t xv = t >= d ? sv[t - d] : 0, xf = t >= d ? sf[t - d] : 0;
    __syncthreads();
    if (!sf[t]) sv[t] += xv;
    sf[t] |= xf;
    __syncthreads();
  }
}

// the sum in front of the lane (flag f) behind the last flag, `carry` being that sum in front of the workgroup
__device__ uint32_t qrs_before(const uint32_t* sv, const uint32_t* sf, uint32_t f, uint32_t carry) {
  const int t = threadIdx.x;
  if (f) return 0;
  if (t == 0) return carry;
  return sf[t - 1] ? sv[t - 1] : carry + sv[t - 1];
}

// the descriptors and the job's code tables into LDS
__device__ void qrs_load(const QrJob& J, const QrsJob& Sg, QrTable* tab, QsEncGeom* g, QrsJob* S) {
  const int t = threadIdx.x;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(J.tab);
  uint32_t* dst = reinterpret_cast<uint32_t*>(tab);
  for (int i = t; i < (int)(8 * sizeof(QrTable) / 4); i += QS_RD_SPLIT_WG) dst[i] = src[i];
  const uint32_t* gs = reinterpret_cast<const uint32_t*>(&J.g);
  for (int i = t; i < (int)(sizeof(QsEncGeom) / 4); i += QS_RD_SPLIT_WG) reinterpret_cast<uint32_t*>(g)[i] = gs[i];
  const uint32_t* ss = reinterpret_cast<const uint32_t*>(&Sg);
  for (int i = t; i < (int)(sizeof(QrsJob) / 4); i += QS_RD_SPLIT_WG) reinterpret_cast<uint32_t*>(S)[i] = ss[i];
  __syncthreads();
}

__global__ void __launch_bounds__(QS_RD_SPLIT_WG) qrs_map(QrsArgs x) {
  __shared__ uint32_t sv[QS_RD_SPLIT_WG], sf[QS_RD_SPLIT_WG];
  const int k = blockIdx.x, t = threadIdx.x;
  const QrJob& J = x.a.jobs[k];
  const QrsJob& S = x.sjobs[k];
  const QrsBufs B = qrs_bufs(x, S);
  QrState* st = qrs_state(x, J);
  if (st->dead) {                                                 // status 1 (written by the launches before): no P to go by
    if (t == 0) *B.nseg = 0;
    return;
  }
  const uint64_t end = qrs_src(x, J, k).n;
  const uint64_t* P = reinterpret_cast<const uint64_t*>(x.a.ws + J.off_p);
  uint32_t carry = 0;
  for (int r0 = 0; r0 < J.intervals; r0 += QS_RD_SPLIT_WG) {
    const int r = r0 + t;
    uint32_t v = 0;
    if (r < J.intervals) {
      uint64_t a, z;
      qrs_interval_bytes(P, r, end, &a, &z);
      v = (uint32_t)qrs_segments(a, z);
    }
    qrs_wg_scan(v, 0, sv, sf);
    if (r < J.intervals) B.seg0[r] = carry + sv[t] - v;
    carry += sv[QS_RD_SPLIT_WG - 1];
  }
  if (t == 0) {
    B.seg0[J.intervals] = carry;
    // (disjoint byte ranges in front of `end`: never more than the workspace was sized for)
    *B.nseg = carry <= S.max_segments ? carry : 0;
    if (carry > S.max_segments) atomicMax(&x.a.d_status[x.a.job0 + k], QS_RD_LENGTH);
  }
}

__global__ void __launch_bounds__(QS_RD_SPLIT_WG) qrs_decode(QrsArgs x) {
  __shared__ QrTable tab[8];
  __shared__ QsEncGeom g;
  __shared__ QrsJob S;
  const int k = qrs_find_job(x.swg0, x.a.n, (int)blockIdx.x), t = threadIdx.x;
  const QrJob& J = x.a.jobs[k];
  const QrsBufs B = qrs_bufs(x, x.sjobs[k]);
  const uint32_t nseg = *B.nseg;
  const uint64_t j = (uint64_t)((int)blockIdx.x - x.swg0[k]) * QS_RD_SPLIT_WG + t;
  if (j - t >= nseg) return;                                      // (the whole workgroup)
  qrs_load(J, x.sjobs[k], tab, &g, &S);
  if (j >= nseg) return;
  const QrSrc s = qrs_src(x, J, k);
  qrs_lane(J, S, tab, s, s.n, reinterpret_cast<const uint64_t*>(x.a.ws + J.off_p), B, (uint32_t)j, x.round);
}

__global__ void __launch_bounds__(QS_RD_SPLIT_WG) qrs_count(QrsArgs x) {
  __shared__ uint32_t sv[QS_RD_SPLIT_WG], sf[QS_RD_SPLIT_WG];
  const int k = qrs_find_job(x.swg0, x.a.n, (int)blockIdx.x), t = threadIdx.x;
  const QrJob& J = x.a.jobs[k];
  const QrsJob& S = x.sjobs[k];
  const QrsBufs B = qrs_bufs(x, S);
  const uint32_t nseg = *B.nseg;
  const uint32_t wg = (uint32_t)((int)blockIdx.x - x.swg0[k]);
  const uint64_t j = (uint64_t)wg * QS_RD_SPLIT_WG + t;
  if (j - t >= nseg) return;                                      // (the whole workgroup)
  uint32_t v = 0, head = 0;
  if (j < nseg) {
    const int r = qrs_find_interval(B.seg0, J.intervals, (uint32_t)j);
    head = j == B.seg0[r];
    v = B.cnt[j];
    if (!head && B.entry[j] != B.exit[QS_RD_SPLIT_ROUNDS & 1][j - 1]) {
      qrs_state(x, J)->pad = 1;                                   // (read by the launches behind this one)
      atomicMax(&x.a.d_status[x.a.job0 + k], QS_RD_NOSYNC);
    }
  }
  qrs_wg_scan(v, head, sv, sf);
  if (t == QS_RD_SPLIT_WG - 1) {
    uint32_t* tile = reinterpret_cast<uint32_t*>(x.a.ws + S.off_stile);
    tile[2 * wg] = sv[t];
    tile[2 * wg + 1] = sf[t];
  }
}

// x.round 0: the tiles of segments, one column; 1: the tiles of MCUs, four.  rec: [tiles][columns + 1], the flag last;
// behind `most` tiles of them the result, [tiles][columns]: what lies in front of each tile behind the last flag
__global__ void __launch_bounds__(QS_RD_SPLIT_WG) qrs_tile_scan(QrsArgs x) {
  __shared__ uint32_t sv[QS_RD_SPLIT_WG], sf[QS_RD_SPLIT_WG];
  const int k = blockIdx.x, t = threadIdx.x;
  const QrJob& J = x.a.jobs[k];
  const QrsJob& S = x.sjobs[k];
  const uint32_t nseg = *reinterpret_cast<const uint32_t*>(x.a.ws + S.off_nseg);
  if (nseg == 0 || qrs_state(x, J)->pad) return;
  const bool dc = x.round != 0;
  if (dc && x.a.d_status[x.a.job0 + k] != 0) return;
  const int ncol = dc ? 4 : 1;
  const uint64_t tiles = dc ? ((uint64_t)J.g.mcus + QS_RD_SPLIT_WG - 1) / QS_RD_SPLIT_WG
                            : ((uint64_t)nseg + QS_RD_SPLIT_WG - 1) / QS_RD_SPLIT_WG;
  const uint64_t most = dc ? tiles : (S.max_segments + QS_RD_SPLIT_WG - 1) / QS_RD_SPLIT_WG;
  const uint32_t* rec = reinterpret_cast<const uint32_t*>(x.a.ws + (dc ? S.off_mtile : S.off_stile));
  uint32_t* res = const_cast<uint32_t*>(rec) + most * (ncol + 1);
  for (int col = 0; col < ncol; ++col) {
    uint32_t carry = 0;
    for (uint64_t i0 = 0; i0 < tiles; i0 += QS_RD_SPLIT_WG) {
      const uint64_t i = i0 + t;
      const uint32_t v = i < tiles ? rec[i * (ncol + 1) + col] : 0, f = i < tiles ? rec[i * (ncol + 1) + ncol] : 0;
      qrs_wg_scan(v, f, sv, sf);
      if (i < tiles) res[i * ncol + col] = qrs_before(sv, sf, 0, carry);
      carry = sf[QS_RD_SPLIT_WG - 1] ? sv[QS_RD_SPLIT_WG - 1] : carry + sv[QS_RD_SPLIT_WG - 1];
    }
  }
}

__global__ void __launch_bounds__(QS_RD_SPLIT_WG) qrs_write(QrsArgs x) {
  __shared__ QrTable tab[8];
  __shared__ QsEncGeom g;
  __shared__ QrsJob S;
  __shared__ uint32_t sv[QS_RD_SPLIT_WG], sf[QS_RD_SPLIT_WG];
  const int k = qrs_find_job(x.swg0, x.a.n, (int)blockIdx.x), t = threadIdx.x;
  const QrJob& J = x.a.jobs[k];
  const QrsBufs B = qrs_bufs(x, x.sjobs[k]);
  const uint32_t nseg = *B.nseg;
  const uint32_t wg = (uint32_t)((int)blockIdx.x - x.swg0[k]);
  const uint64_t j = (uint64_t)wg * QS_RD_SPLIT_WG + t;
  if (j - t >= nseg || qrs_state(x, J)->pad) return;              // (the whole workgroup; pad: status 4)
  qrs_load(J, x.sjobs[k], tab, &g, &S);
  uint32_t v = 0, head = 0, sg = 0;
  int r = 0;
  if (j < nseg) {
    r = qrs_find_interval(B.seg0, J.intervals, (uint32_t)j);
    sg = (uint32_t)j - B.seg0[r];
    head = sg == 0;
    v = B.cnt[j];
  }
  qrs_wg_scan(v, head, sv, sf);
  const uint32_t* carry = reinterpret_cast<const uint32_t*>(x.a.ws + S.off_stile)
                          + 2 * ((S.max_segments + QS_RD_SPLIT_WG - 1) / QS_RD_SPLIT_WG);
  const uint32_t first = qrs_before(sv, sf, head, carry[wg]);
  if (j >= nseg) return;
  const int m0 = r * J.ri, m1 = (m0 + J.ri < g.mcus) ? m0 + J.ri : g.mcus;
  const bool last = j + 1 == B.seg0[r + 1];
  QrsSink w;
  w.g = &g;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    w.out.coef[c] = x.a.p[k].coef[c];
    w.out.nblk[c] = x.a.p[k].nblk[c];
  }
  w.dcd = B.dcd;
  w.blk0 = (long long)m0 * g.bpm;
  w.nblk = (long long)(m1 - m0) * g.bpm;
  w.bi = first;
  w.status = QS_RD_OK;
  // the interval ran out of bytes before its blocks were done
  if (last && (long long)first + v < w.nblk) w.status = QS_RD_LENGTH;
  const QrSrc s = qrs_src(x, J, k);
  uint64_t a, z;
  qrs_interval_bytes(reinterpret_cast<const uint64_t*>(x.a.ws + J.off_p), r, s.n, &a, &z);
  const uint64_t lo = qrs_bound(s, a, z, sg), hi = last ? z : qrs_bound(s, a, z, (uint64_t)sg + 1);
  uint64_t ex;
  uint32_t cnt;
  int status = w.status;
  qrs_walk<true>(tab, S, s, z, lo, hi, B.entry[j], &ex, &cnt, &w);
  if (w.status > status) status = w.status;
  if (status) atomicMax(&x.a.d_status[x.a.job0 + k], status);
}

// the lane's MCU: the sum of the DC differences of each component, and whether an interval starts with it
__device__ void qrs_mcu_sums(const QrJob& J, const QrsJob& S, const int16_t* dcd, uint64_t m, uint32_t* sum, uint32_t* head) {
  sum[0] = sum[1] = sum[2] = sum[3] = 0;
  *head = 0;
  if (m >= (uint64_t)J.g.mcus) return;
  *head = m % (uint64_t)J.ri == 0;
  for (int u = 0; u < J.g.bpm && u < 10; ++u) {
    const int c = S.comp[u] & 3;
    const uint32_t d = (uint32_t)(int32_t)dcd[m * J.g.bpm + u];
#pragma unroll
    for (int i = 0; i < 4; ++i) sum[i] += i == c ? d : 0u;       // (no indexed private array: that would be scratch)
  }
}

__global__ void __launch_bounds__(QS_RD_SPLIT_WG) qrs_dc_tiles(QrsArgs x) {
  __shared__ uint32_t sv[QS_RD_SPLIT_WG], sf[QS_RD_SPLIT_WG];
  const int k = qrs_find_job(x.twg0, x.a.n, (int)blockIdx.x), t = threadIdx.x;
  const QrJob& J = x.a.jobs[k];
  const QrsJob& S = x.sjobs[k];
  const uint32_t wg = (uint32_t)((int)blockIdx.x - x.twg0[k]);
  if (x.a.d_status[x.a.job0 + k] != 0) return;                   // (settled by the launches before; the whole workgroup)
  uint32_t sum[4], head;
  qrs_mcu_sums(J, S, reinterpret_cast<const int16_t*>(x.a.ws + S.off_dcd), (uint64_t)wg * QS_RD_SPLIT_WG + t, sum, &head);
  uint32_t* tile = reinterpret_cast<uint32_t*>(x.a.ws + S.off_mtile) + 5 * (uint64_t)wg;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    qrs_wg_scan(sum[c], head, sv, sf);
    if (t == QS_RD_SPLIT_WG - 1) {
      tile[c] = sv[t];
      tile[4] = sf[t];
    }
  }
}

__global__ void __launch_bounds__(QS_RD_SPLIT_WG) qrs_dc_write(QrsArgs x) {
  __shared__ uint32_t sv[QS_RD_SPLIT_WG], sf[QS_RD_SPLIT_WG];
  const int k = qrs_find_job(x.twg0, x.a.n, (int)blockIdx.x), t = threadIdx.x;
  const QrJob& J = x.a.jobs[k];
  const QrsJob& S = x.sjobs[k];
  const uint32_t wg = (uint32_t)((int)blockIdx.x - x.twg0[k]);
  if (x.a.d_status[x.a.job0 + k] != 0) return;                   // (the whole workgroup)
  const int16_t* dcd = reinterpret_cast<const int16_t*>(x.a.ws + S.off_dcd);
  const uint64_t m = (uint64_t)wg * QS_RD_SPLIT_WG + t;
  const uint64_t tiles = ((uint64_t)J.g.mcus + QS_RD_SPLIT_WG - 1) / QS_RD_SPLIT_WG;
  const uint32_t* carry = reinterpret_cast<const uint32_t*>(x.a.ws + S.off_mtile) + 5 * tiles + 4 * (uint64_t)wg;
  uint32_t sum[4], head, pred[4];
  qrs_mcu_sums(J, S, dcd, m, sum, &head);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    qrs_wg_scan(sum[c], head, sv, sf);
    pred[c] = qrs_before(sv, sf, head, carry[c]);
  }
  if (m >= (uint64_t)J.g.mcus) return;
  QrsSink w;
  w.g = &J.g;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    w.out.coef[c] = x.a.p[k].coef[c];
    w.out.nblk[c] = x.a.p[k].nblk[c];
  }
  w.blk0 = 0;
  for (int u = 0; u < J.g.bpm && u < 10; ++u) {
    const int c = S.comp[u] & 3;
    const long long gi = (long long)m * J.g.bpm + u;
    const uint32_t d = (uint32_t)(int32_t)dcd[gi];
#pragma unroll
    for (int i = 0; i < 4; ++i) pred[i] += i == c ? d : 0u;
    int16_t* blk = qrs_block(S, w, gi);
    if (blk) blk[0] = (int16_t)qrs_pick4(pred, c);               // the prediction runs as int, JCOEF is a short
  }
}

}  // namespace

// what one run enqueues for a chunk of jobs: zwgs / mwgs as qs_launch_read takes them, swgs / twgs = workgroups of
// the launches over segments and over MCUs
void qs_launch_read_split(QrsArgs& x, int zwgs, int mwgs, int swgs, int twgs, hipStream_t s) {
  qs_launch_read_markers(x.a, zwgs, mwgs, s);
  const dim3 wg(QS_RD_SPLIT_WG);
  hipLaunchKernelGGL(qrs_map, dim3(x.a.n), wg, 0, s, x);
  for (int round = 0; round <= QS_RD_SPLIT_ROUNDS; ++round) {
    x.round = round;
    hipLaunchKernelGGL(qrs_decode, dim3(swgs), wg, 0, s, x);
  }
  hipLaunchKernelGGL(qrs_count, dim3(swgs), wg, 0, s, x);
  x.round = 0;
  hipLaunchKernelGGL(qrs_tile_scan, dim3(x.a.n), wg, 0, s, x);
  hipLaunchKernelGGL(qrs_write, dim3(swgs), wg, 0, s, x);
  hipLaunchKernelGGL(qrs_dc_tiles, dim3(twgs), wg, 0, s, x);
  x.round = 1;
  hipLaunchKernelGGL(qrs_tile_scan, dim3(x.a.n), wg, 0, s, x);
  hipLaunchKernelGGL(qrs_dc_write, dim3(twgs), wg, 0, s, x);
}
