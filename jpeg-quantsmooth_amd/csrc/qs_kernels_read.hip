// qs_kernels_read.hip -- reading a sequential Huffman scan with restart intervals into device-resident coefficient
// arrays (gfx950): what libjpeg 9 leaves behind jpeg_read_coefficients (jdhuff.c decode_mcu, jdcoefct.c consume_data).
// DESIGN.md section 14.
//
// One lane per restart interval: an interval starts on a byte, behind a marker a byte search finds, with every DC
// prediction at 0 -- no lane needs anything from another.  Every dependency between workgroups is a kernel boundary:
//   qr_init        the job's state and status; the coefficient arrays zeroed with 16-byte stores
//   qr_mark_count  a lane per 16 bytes of the scan (and one byte of look-ahead): RSTn markers per 4 KiB chunk, and an
//                  atomicMin of the first terminating marker's offset -- the scan's end
//   qr_mark_scan   one workgroup per job: the chunk that holds the end counted again up to it, the chunks behind it
//                  dropped, the exclusive scan of the counts; the total against intervals - 1 (status 1)
//   qr_mark_place  the byte each interval starts at, P[r]; each marker's number against (k - 1) & 7 (status 1)
//   qr_decode      a lane per interval: qr_decode_interval of qs_read.h, the job's code tables in LDS
// No loop's trip count depends on decoded data; the bounds are stated in qs_read.h.
#include <hip/hip_runtime.h>
#include "qs_read.h"

namespace {

// which job of the chunk owns workgroup `wg` of a launch whose jobs start at first[i]
__device__ int qr_find_job(const int32_t* first, int n, int wg) {
  int k = 0;
  for (int i = 1; i < n; ++i)
    if (wg >= first[i]) k = i;
  return k;
}

__device__ QrState* qr_state(const QrArgs& a, const QrJob& J) { return reinterpret_cast<QrState*>(a.ws + J.off_state); }

// the bytes of job k the kernels look at
__device__ QrSrc qr_src(const QrArgs& a, const QrJob& J, int k) {
  QrSrc s;
  s.p = a.p[k].scan;
  s.n = a.p[k].scan_bytes < J.max_scan ? a.p[k].scan_bytes : J.max_scan;
  return s;
}

// The marker kernels cut the scan into 16-byte units of ALIGNED memory: lane `unit` of the job owns scan positions
// [16 * unit - shift, 16 * unit - shift + 16), shift = the scan's address modulo 16.  -> bit i of *rst: an RSTn marker
// starts at the lane's byte i; bit i of *term: another marker does (the look-ahead byte belongs to the next lane).
// *pos0: the scan position of byte 0 (negative in the first unit of an unaligned scan)
__device__ void qr_unit_markers(const QrSrc& s, uint64_t unit, int64_t* pos0, uint32_t* rst, uint32_t* term, uint32_t* codes) {
  const int shift = (int)(reinterpret_cast<uintptr_t>(s.p) & 15);
  const int64_t p0 = (int64_t)(unit * 16) - shift;
  *pos0 = p0;
  uint8_t b[17];
  if (p0 >= 0 && (uint64_t)p0 + 16 <= s.n) {
    const uint4 q = *reinterpret_cast<const uint4*>(s.p + p0);   // aligned: p + p0 = (p - shift) + 16 * unit
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) b[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) b[i] = (p0 + i >= 0) ? (uint8_t)qr_byte(s, (uint64_t)(p0 + i)) : 0;
  }
  b[16] = (p0 + 16 >= 0) ? (uint8_t)qr_byte(s, (uint64_t)(p0 + 16)) : 0;
  uint32_t r = 0, t = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int m = (p0 + i >= 0) ? qr_marker(b[i], b[i + 1]) : 0;
    if (m == 1) r |= 1u << i;
    if (m == 2) t |= 1u << i;
  }
  *rst = r;
  *term = t;
  if (codes) {                                                    // the marker numbers, 3 bits per byte position
    // (two words: 16 positions x 3 bits)
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t n = b[i + 1] & 7u;
      if (i < 8) lo |= n << (3 * i); else hi |= n << (3 * (i - 8));
    }
    codes[0] = lo;
    codes[1] = hi;
  }
}

// 16-byte units of job k's scan in aligned memory, and the marker workgroups (4 KiB chunks) that hold them.  The run
// call launches at least that many per job (it bounds the scan from the geometry alone): the others return at once
__device__ uint64_t qr_units(const QrSrc& s) {
  const uint64_t shift = reinterpret_cast<uintptr_t>(s.p) & 15;
  return (shift + s.n + 15) / 16;
}
__device__ uint64_t qr_chunks(const QrSrc& s) { return (qr_units(s) + QS_RD_WG - 1) / QS_RD_WG; }

__global__ void __launch_bounds__(QS_RD_WG) qr_init(QrArgs a) {
  const int k = qr_find_job(a.zwg0, a.n, (int)blockIdx.x), t = threadIdx.x;
  const QrJob& J = a.jobs[k];
  const int wg = (int)blockIdx.x - a.zwg0[k];
  if (wg == 0 && t == 0) {
    QrState* st = qr_state(a, J);
    st->end = qr_src(a, J, k).n;
    st->dead = 0;
    st->pad = 0;
    a.d_status[a.job0 + k] = 0;
  }
  const uint4 zero = make_uint4(0, 0, 0, 0);
  for (int c = 0; c < J.g.ncomp && c < 4; ++c) {
    uint4* dst = reinterpret_cast<uint4*>(a.p[k].coef[c]);
    const long long n16 = (long long)a.p[k].nblk[c] * 8;         // a block is 128 bytes
    for (long long i = (long long)wg * QS_RD_WG + t; i < n16; i += (long long)J.nzwg * QS_RD_WG) dst[i] = zero;
  }
}

__global__ void __launch_bounds__(QS_RD_WG) qr_mark_count(QrArgs a) {
  __shared__ uint32_t cnt;
  const int k = qr_find_job(a.mwg0, a.n, (int)blockIdx.x), t = threadIdx.x;
  const QrJob& J = a.jobs[k];
  const uint64_t chunk = (uint64_t)((int)blockIdx.x - a.mwg0[k]);
  const QrSrc s = qr_src(a, J, k);
  if (chunk >= qr_chunks(s)) return;                              // (the whole workgroup)
  if (t == 0) cnt = 0;
  __syncthreads();
  const uint64_t unit = chunk * QS_RD_WG + t;
  if (unit < qr_units(s)) {
    int64_t p0;
    uint32_t rst, term;
    qr_unit_markers(s, unit, &p0, &rst, &term, nullptr);
    if (rst) atomicAdd(&cnt, (uint32_t)__popc(rst));
    if (term) atomicMin(&qr_state(a, J)->end, (unsigned long long)(p0 + (__ffs(term) - 1)));
  }
  __syncthreads();
  if (t == 0) reinterpret_cast<uint32_t*>(a.ws + J.off_cnt)[chunk] = cnt;
}

__global__ void __launch_bounds__(QS_RD_WG) qr_mark_scan(QrArgs a) {
  __shared__ uint32_t sc[QS_RD_WG];
  __shared__ uint32_t recount;
  const int k = blockIdx.x, t = threadIdx.x;
  const QrJob& J = a.jobs[k];
  const QrSrc s = qr_src(a, J, k);
  QrState* st = qr_state(a, J);
  const uint64_t end = st->end;
  const uint64_t shift = reinterpret_cast<uintptr_t>(s.p) & 15;
  const uint64_t units = qr_units(s);
  const uint64_t chunks = qr_chunks(s);
  const uint64_t ce = (end + shift) / QS_RD_MCHUNK;               // the chunk that holds the end (== chunks: none does)
  uint32_t* cnt = reinterpret_cast<uint32_t*>(a.ws + J.off_cnt);
  uint32_t* off = reinterpret_cast<uint32_t*>(a.ws + J.off_off);
  if (t == 0) recount = 0;
  __syncthreads();
  if (ce < chunks) {                                              // count that chunk again, up to the end
    const uint64_t unit = ce * QS_RD_WG + t;
    if (unit < units) {
      int64_t p0;
      uint32_t rst, term;
      qr_unit_markers(s, unit, &p0, &rst, &term, nullptr);
      uint32_t n = 0;
      for (int i = 0; i < 16; ++i)
        if (((rst >> i) & 1u) && p0 + i >= 0 && (uint64_t)(p0 + i) < end) ++n;
      if (n) atomicAdd(&recount, n);
    }
  }
  __syncthreads();
  uint32_t carry = 0;
  for (uint64_t c0 = 0; c0 < chunks; c0 += QS_RD_WG) {            // exclusive scan, 256 chunks a step
    const uint64_t c = c0 + t;
    const uint32_t v = c >= chunks ? 0u : c < ce ? cnt[c] : c == ce ? recount : 0u;
    sc[t] = v;
    __syncthreads();
    for (int d = 1; d < QS_RD_WG; d <<= 1) {
      const uint32_t x = t >= d ? sc[t - d] : 0;
      __syncthreads();
      sc[t] += x;
      __syncthreads();
    }
    if (c < chunks) off[c] = carry + sc[t] - v;
    carry += sc[QS_RD_WG - 1];
    __syncthreads();
  }
  if (t == 0) {
    uint64_t* P = reinterpret_cast<uint64_t*>(a.ws + J.off_p);
    P[0] = 0;
    P[J.intervals] = end + 2;                                     // as if a marker stood at the end: interval r is [P[r], P[r + 1] - 2)
    if (carry != (uint32_t)(J.intervals - 1)) {
      st->dead = 1;
      a.d_status[a.job0 + k] = QS_RD_MARKERS;
    }
  }
}

__global__ void __launch_bounds__(QS_RD_WG) qr_mark_place(QrArgs a) {
  __shared__ uint32_t sc[QS_RD_WG];
  const int k = qr_find_job(a.mwg0, a.n, (int)blockIdx.x), t = threadIdx.x;
  const QrJob& J = a.jobs[k];
  const uint64_t chunk = (uint64_t)((int)blockIdx.x - a.mwg0[k]);
  const QrSrc s = qr_src(a, J, k);
  QrState* st = qr_state(a, J);
  if (chunk >= qr_chunks(s)) return;                              // (the whole workgroup)
  // (a job the scan kernel gave status 1 is walked all the same: other workgroups of this launch write st->dead, so a
  // return on it in front of the barriers below would not be uniform; the P index is checked at each store)
  const uint64_t end = st->end;
  const uint64_t unit = chunk * QS_RD_WG + t;
  int64_t p0 = 0;
  uint32_t rst = 0, term = 0, codes[2] = {0, 0};
  if (unit < qr_units(s)) qr_unit_markers(s, unit, &p0, &rst, &term, codes);
  uint32_t mine = 0;                                              // the lane's markers in front of the end
  for (int i = 0; i < 16; ++i)
    if (((rst >> i) & 1u) && p0 + i >= 0 && (uint64_t)(p0 + i) < end) mine |= 1u << i;
  const uint32_t v = (uint32_t)__popc(mine);
  sc[t] = v;
  __syncthreads();
  for (int d = 1; d < QS_RD_WG; d <<= 1) {
    const uint32_t x = t >= d ? sc[t - d] : 0;
    __syncthreads();
    sc[t] += x;
    __syncthreads();
  }
  if (!mine) return;
  uint32_t r = reinterpret_cast<const uint32_t*>(a.ws + J.off_off)[chunk] + sc[t] - v;   // markers in front of the lane's
  uint64_t* P = reinterpret_cast<uint64_t*>(a.ws + J.off_p);
  bool bad = false;
  for (int i = 0; i < 16; ++i) {
    if (!((mine >> i) & 1u)) continue;
    const uint32_t n = (i < 8 ? codes[0] >> (3 * i) : codes[1] >> (3 * (i - 8))) & 7u;
    if (r + 1 < (uint32_t)J.intervals) P[r + 1] = (uint64_t)(p0 + i) + 2;   // marker k = r + 1 opens interval k
    else bad = true;
    if (n != (r & 7u)) bad = true;
    ++r;
  }
  if (bad) {
    st->dead = 1;
    a.d_status[a.job0 + k] = QS_RD_MARKERS;
  }
}

__global__ void __launch_bounds__(QS_RD_DWG) qr_decode(QrArgs a) {
  __shared__ QrTable tab[8];
  __shared__ QsEncGeom g;
  __shared__ int32_t tbl[8];
  const int k = qr_find_job(a.dwg0, a.n, (int)blockIdx.x), t = threadIdx.x;
  const QrJob& J = a.jobs[k];
  const QrState* st = qr_state(a, J);
  if (st->dead) return;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(J.tab);
    uint32_t* dst = reinterpret_cast<uint32_t*>(tab);
    for (int i = t; i < (int)(sizeof(tab) / 4); i += QS_RD_DWG) dst[i] = src[i];
    const uint32_t* gs = reinterpret_cast<const uint32_t*>(&J.g);
    for (int i = t; i < (int)(sizeof(QsEncGeom) / 4); i += QS_RD_DWG) reinterpret_cast<uint32_t*>(&g)[i] = gs[i];
    if (t < 4) tbl[t] = J.dc_tbl[t];
    else if (t < 8) tbl[t] = J.ac_tbl[t - 4];
  }
  __syncthreads();
  const int r = ((int)blockIdx.x - a.dwg0[k]) * QS_RD_DWG + t;
  if (r >= J.intervals) return;
  const uint64_t* P = reinterpret_cast<const uint64_t*>(a.ws + J.off_p);
  QrSrc s = qr_src(a, J, k);
  const uint64_t end = st->end < s.n ? st->end : s.n;
  s.n = end;                                                      // nothing behind the job's end is read
  uint64_t start = P[r], stop = P[r + 1] - 2;
  if (stop > end) stop = end;
  if (start > stop) start = stop;
  QrOut out;
  for (int c = 0; c < 4; ++c) {
    out.coef[c] = a.p[k].coef[c];
    out.nblk[c] = a.p[k].nblk[c];
  }
  const int m0 = r * J.ri, m1 = (m0 + J.ri < g.mcus) ? m0 + J.ri : g.mcus;
  const int status = qr_decode_interval(g, tbl, tbl + 4, tab, s, start, stop, m0, m1, out);
  if (status) atomicMax(&a.d_status[a.job0 + k], status);
}

}  // namespace

// the init and marker launches of a chunk of jobs: what both routes decode behind (the split route:
// qs_kernels_read_split.hip).  zwgs / mwgs = workgroups of the init and marker launches
void qs_launch_read_markers(const QrArgs& a, int zwgs, int mwgs, hipStream_t s) {
  hipLaunchKernelGGL(qr_init, dim3(zwgs), dim3(QS_RD_WG), 0, s, a);
  if (mwgs > 0) hipLaunchKernelGGL(qr_mark_count, dim3(mwgs), dim3(QS_RD_WG), 0, s, a);
  hipLaunchKernelGGL(qr_mark_scan, dim3(a.n), dim3(QS_RD_WG), 0, s, a);
  if (mwgs > 0) hipLaunchKernelGGL(qr_mark_place, dim3(mwgs), dim3(QS_RD_WG), 0, s, a);
}

// what one run enqueues for a chunk of jobs: dwgs = workgroups of the decode launch
void qs_launch_read(const QrArgs& a, int zwgs, int mwgs, int dwgs, hipStream_t s) {
  qs_launch_read_markers(a, zwgs, mwgs, s);
  hipLaunchKernelGGL(qr_decode, dim3(dwgs), dim3(QS_RD_DWG), 0, s, a);
}
