// qs_kernels_read_prog.hip -- reading a progressive Huffman file (SOF2) into device-resident coefficient arrays (gfx950):
// what libjpeg 9 leaves behind jpeg_read_coefficients (jdhuff.c decode_mcu_DC_first / _AC_first / _DC_refine /
// _AC_refine, jdcoefct.c consume_data).  DESIGN.md section 18.
//
// The unit of work is a (job, scan) pair; one lane decodes one restart interval of one scan.  Every dependency between
// workgroups is a kernel boundary:
//   qrp_init    the job's status; its coefficient arrays zeroed with 16-byte stores, once
//   (markers)   per pair, the scan's end and its RSTn markers found, checked and placed: the four launches of the
//               interval route on the pair's QrJob (qs_kernels_read.hip: qs_launch_read_markers), 32 pairs a launch set
//   qrp_check   a lane per pair: the SOS header in front of the prepared offset and the marker kernels' verdict, folded
//               into the job's status (1: no scan of the job is decoded)
//   qrp_decode  one launch per LEVEL of the script over all pairs of that level in the chunk of jobs: a workgroup of 64
//               lanes (= intervals) belongs to one pair, whose code tables sit in LDS (four DC tables, or one AC table,
//               or none); qrp_decode_interval of qs_read_prog.h.  Two pairs of one level never touch the same int16.
// No workgroup waits on another, and no loop's trip count depends on decoded data; the bounds are stated in
// qs_read_prog.h.
#include <hip/hip_runtime.h>
#include "qs_read_prog.h"

namespace {

__device__ QrSrc qrp_file(const QrpArgs& a, int k) {
  QrSrc f;
  f.p = a.file[k];
  f.n = a.file_bytes[k];
  return f;
}

__global__ void __launch_bounds__(QS_RD_WG) qrp_init(QrpArgs a) {
  int k = 0;
  for (int i = 1; i < a.n; ++i)
    if ((int)blockIdx.x >= a.zwg0[i]) k = i;
  const int t = threadIdx.x, wg = (int)blockIdx.x - a.zwg0[k], nzwg = a.zwg0[k + 1] - a.zwg0[k];
  if (wg == 0 && t == 0) a.d_status[a.job0 + k] = 0;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  for (int c = 0; c < 4; ++c) {
    uint4* dst = reinterpret_cast<uint4*>(a.coef[k][c]);
    if (!dst) continue;
    const long long n16 = (long long)a.nblk[k][c] * 8;             // a block is 128 bytes
    for (long long i = (long long)wg * QS_RD_WG + t; i < n16; i += (long long)nzwg * QS_RD_WG) dst[i] = zero;
  }
}

__global__ void __launch_bounds__(QS_RD_WG) qrp_check(QrpArgs a) {
  const int i = (int)(blockIdx.x * QS_RD_WG + threadIdx.x);
  if (i >= a.npairs) return;
  const QrJob& J = a.pairs[a.pair0 + i];
  const QrpScan& X = a.scans[a.pair0 + i];
  const int k = X.job - a.job0;
  if (k < 0 || k >= a.n) return;
  const QrSrc file = qrp_file(a, k);
  const QrState* st = reinterpret_cast<const QrState*>(a.ws + J.off_state);
  // (only status 1 is written here: the decode launches leave a job alone on it, whatever else its scans would report)
  if (st->dead || !qrp_header_ok(file, X)) atomicMax(&a.d_status[a.job0 + k], QS_RD_MARKERS);
}

// the entry of the launch that owns workgroup wg: the last one whose first workgroup is not behind it
__device__ int qrp_find_entry(const QrpEntry* list, int n, int wg) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (list[mid].wg0 <= wg) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(QS_RD_DWG) qrp_decode(QrpArgs a) {
  __shared__ QrTable tab[4];
  __shared__ QsEncGeom g;
  __shared__ QrpScan x;
  __shared__ int32_t tbl[4];
  const int t = threadIdx.x;
  const QrpEntry e = a.list[qrp_find_entry(a.list, a.nlist, (int)blockIdx.x)];
  const QrJob& J = a.pairs[e.pair];
  const QrpScan& X = a.scans[e.pair];
  const int k = X.job - a.job0;
  if (k < 0 || k >= a.n) return;
  // a job with status 1 is left alone (qrp_check wrote it; no pair of such a job runs, so it stays 1: the same for every lane)
  if (a.d_status[a.job0 + k] == QS_RD_MARKERS) return;
  {
    const bool dc = X.Ss == 0;
    if (!(dc && X.Ah)) {                                             // a DC refinement has no symbols
      const int ntab = dc ? 4 : 1;
      const uint32_t* src = reinterpret_cast<const uint32_t*>(dc ? J.tab : J.tab + 4 + (J.ac_tbl[0] & 3));
      uint32_t* dst = reinterpret_cast<uint32_t*>(tab);
      for (int i = t; i < ntab * (int)(sizeof(QrTable) / 4); i += QS_RD_DWG) dst[i] = src[i];
    }
    const uint32_t* gs = reinterpret_cast<const uint32_t*>(&J.g);
    for (int i = t; i < (int)(sizeof(QsEncGeom) / 4); i += QS_RD_DWG) reinterpret_cast<uint32_t*>(&g)[i] = gs[i];
    const uint32_t* xs = reinterpret_cast<const uint32_t*>(&X);
    for (int i = t; i < (int)(sizeof(QrpScan) / 4); i += QS_RD_DWG) reinterpret_cast<uint32_t*>(&x)[i] = xs[i];
    if (t < 4) tbl[t] = J.dc_tbl[t];
  }
  __syncthreads();
  const int r = ((int)blockIdx.x - e.wg0) * QS_RD_DWG + t;
  if (r >= J.intervals) return;
  const QrState* st = reinterpret_cast<const QrState*>(a.ws + J.off_state);
  const uint64_t* P = reinterpret_cast<const uint64_t*>(a.ws + J.off_p);
  QrSrc s = qrp_scan_src(qrp_file(a, k), J, X);
  const uint64_t end = st->end < s.n ? st->end : s.n;
  if (r == 0 && st->end >= s.n) atomicMax(&a.d_status[a.job0 + k], QS_RD_LENGTH);   // no marker ends the scan: the file stops inside it
  s.n = end;                                                       // nothing behind the scan's end is read
  uint64_t start = P[r], stop = P[r + 1] - 2;
  if (stop > end) stop = end;
  if (start > stop) start = stop;
  const int m0 = r * J.ri, m1 = (m0 + J.ri < g.mcus) ? m0 + J.ri : g.mcus;
  const int status = qrp_decode_interval(g, x, tbl, tab, tab, s, start, stop, m0, m1, a.coef[k], a.nblk[k]);
  if (status) atomicMax(&a.d_status[a.job0 + k], status);
}

}  // namespace

void qs_launch_read_prog_init(const QrpArgs& a, int zwgs, hipStream_t s) {
  hipLaunchKernelGGL(qrp_init, dim3(zwgs), dim3(QS_RD_WG), 0, s, a);
}

void qs_launch_read_prog_check(const QrpArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(qrp_check, dim3((a.npairs + QS_RD_WG - 1) / QS_RD_WG), dim3(QS_RD_WG), 0, s, a);
}

// one level: a.list / a.nlist are its entries, dwgs its workgroups
void qs_launch_read_prog_decode(const QrpArgs& a, int dwgs, hipStream_t s) {
  hipLaunchKernelGGL(qrp_decode, dim3(dwgs), dim3(QS_RD_DWG), 0, s, a);
}
