// qs_kernels_huff.hip -- optimal Huffman tables and whole JPEG files on the device (gfx950).  DESIGN.md section 16.
//   qh_optimal   qs_hip_huff_optimal_device: one wave per table (csrc/qs_huff.h), four tables per workgroup
//   qh_tables    the whole-file run with optimize: per job its four tables (DC 0, DC 1, AC 0, AC 1; one wave each) from
//                the histogram in the scratch -> the tables, their code words in the descriptors' form, the bytes of the
//                file in front of the segment (head + DHT markers + mid) and the job's table status
//   qh_frame     the whole-file run: head, DHT markers, mid and EOI around the segment the coder stored behind the prefix
// Every store of qh_frame is checked against the job's capacity; qh_optimal and qh_tables store into arrays whose size
// follows from the table / job count alone.
#include <hip/hip_runtime.h>
#include "qs_encode.h"
#include "qs_huff.h"

namespace {

constexpr int QH_WAVES = 4;

// S.outbits / S.huffval -> a qs_hip_huff_table at `dst` (any alignment: byte stores)
__device__ void qh_store_table(const QsHuffShared& S, uint8_t* dst) {
  const int lane = threadIdx.x & 63;
  if (lane < 17) dst[lane] = S.outbits[lane];
#pragma unroll
  for (int k = 0; k < 4; ++k) dst[17 + k * 64 + lane] = S.huffval[k * 64 + lane];
}

__global__ void __launch_bounds__(64 * QH_WAVES) qh_optimal(const uint32_t* d_counts, int ntables, uint8_t* d_tables,
                                                            int32_t* d_status) {
  __shared__ QsHuffShared S[QH_WAVES];
  const int w = threadIdx.x >> 6;
  const long long tb = (long long)blockIdx.x * QH_WAVES + w;
  const bool live = tb < ntables;                   // (a wave without a table runs on zero counts: it meets the barriers)
  const int status = qs_huff_wave(live ? d_counts + tb * 257 : nullptr, S[w]);
  if (!live) return;
  qh_store_table(S[w], d_tables + tb * QS_ENC_TABLE_BYTES);
  if ((threadIdx.x & 63) == 0) d_status[tb] = status;
}

__device__ int qh_variant(const QsHuffArgs& a, const QsEncJob& J, int k) {
  return (J.two && a.d_stop && a.d_stop[a.job0 + k] != 0) ? 1 : 0;
}

__device__ bool qh_uses_table1(const QsEncJob& J) {
  bool used = false;
  for (int c = 0; c < J.g[0].ncomp && c < 4; ++c) used |= J.tbl[c] == 1;
  return used;
}

__global__ void __launch_bounds__(64 * QH_WAVES) qh_tables(QsHuffArgs a) {
  __shared__ QsHuffShared S[QH_WAVES];
  const int k = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const QsEncJob& J = a.jobs[k];
  const size_t job = (size_t)(a.job0 + k);
  const bool used = (w & 1) == 0 || qh_uses_table1(J);       // wave w: DC 0, DC 1, AC 0, AC 1
  const int status = qs_huff_wave(used ? a.counts + (job * 4 + w) * 257 : nullptr, S[w]);
  uint8_t* tabs = a.tables + job * QS_ENC_TABLES_BYTES;
  qh_store_table(S[w], tabs + w * QS_ENC_TABLE_BYTES);
  if (lane == 0) tabs[4 * QS_ENC_TABLE_BYTES + w] = used ? 1 : 0;              // has_dc[0 .. 1], has_ac[0 .. 1]
  if (a.d_tables) {
    uint8_t* out = a.d_tables + job * QS_ENC_TABLES_BYTES;
    qh_store_table(S[w], out + w * QS_ENC_TABLE_BYTES);
    if (lane == 0) out[4 * QS_ENC_TABLE_BYTES + w] = used ? 1 : 0;
  }
  // jpeg_make_c_derived_tbl: (size << 16) | code by symbol, 0 where the table has none.  The code at place p of
  // huffval: the first code of its length plus its place among the codes of that length
  const bool is_ac = w >= 2;
  const int nsyms = is_ac ? 256 : 16;
  uint32_t* cw = a.codes + job * QS_ENC_CODES + (is_ac ? 2 * 16 + (w & 1) * 256 : (w & 1) * 16);
  for (int i = lane; i < nsyms; i += 64) cw[i] = 0;
  __syncthreads();                                  // (a wave's own stores, in order for its own lanes)
  if (status == QS_HF_OK)
    for (int p = lane; p < S[w].nsym && p < 256; p += 64) {
      uint32_t code = 0;
      int first = 0, len = 0;
      for (int l = 1; l <= 16; ++l) {
        const int n = S[w].outbits[l];
        if (p < first + n) {
          len = l;
          code += (uint32_t)(p - first);
          break;
        }
        first += n;
        code = (code + (uint32_t)n) << 1;
      }
      const int sym = S[w].huffval[p];
      if (len && sym < nsyms) cw[sym] = ((uint32_t)len << 16) | code;
    }
  __syncthreads();
  if (threadIdx.x == 0) {
    // the DHT markers: FF C4, length, Tc / Th, 16 counts, the symbols -- one per table in use
    uint32_t dht = 0;
    int bad = 0;
    for (int t = 0; t < QH_WAVES; ++t) {
      bad |= S[t].status;
      if ((t & 1) == 0 || qh_uses_table1(J)) dht += 5 + 16 + (uint32_t)S[t].nsym;
    }
    const int v = qh_variant(a, J, k);
    a.tstatus[job] = bad ? QS_HF_CLEN : 0;
    a.prefix[job] = (uint64_t)(a.framed ? a.f[k].head_bytes[v] + a.f[k].mid_bytes[v] : 0u) + dht;
  }
}

__global__ void __launch_bounds__(256) qh_frame(QsHuffArgs a) {
  __shared__ uint8_t dht[QS_ENC_DHT_MAX];
  __shared__ uint32_t off[5];
  const int k = blockIdx.x, t = threadIdx.x;
  const QsEncJob& J = a.jobs[k];
  const size_t job = (size_t)(a.job0 + k);
  const int status = a.d_status[job];
  if (status != 0 && status != 2) return;           // no file: the buffer is unspecified
  const int v = qh_variant(a, J, k);
  const QsFramePtrs& F = a.f[k];
  const uint8_t* tabs = a.tables + job * QS_ENC_TABLES_BYTES;
  if (t == 0) {
    // jcmarker.c: per component DC then AC, each table once -- DC 0, AC 0, DC 1, AC 1 (table w of the scratch: DC 0, DC 1,
    // AC 0, AC 1)
    uint32_t at = 0;
    const int order[4] = {0, 2, 1, 3};
    for (int i = 0; i < 4; ++i) {
      const int w = order[i];
      off[w] = at;
      if (a.optimize && tabs[4 * QS_ENC_TABLE_BYTES + w]) {
        uint32_t n = 0;
        for (int l = 1; l <= 16; ++l) n += tabs[w * QS_ENC_TABLE_BYTES + l];
        at += 5 + 16 + (n > 256 ? 256 : n);
      }
    }
    off[4] = at;
  }
  __syncthreads();
  const uint32_t dl = off[4];
  {
    const int w = t >> 6, lane = t & 63;
    const uint32_t end = w == 0 ? off[2] : w == 2 ? off[1] : w == 1 ? off[3] : off[4];
    if (end > off[w]) {                             // the table is written: end - off[w] = 21 + its symbols
      const uint8_t* tb = tabs + w * QS_ENC_TABLE_BYTES;
      const uint32_t nsym = end - off[w] - 21, len = 2 + 1 + 16 + nsym;
      uint8_t* m = dht + off[w];
      if (lane == 0) {
        m[0] = 0xff;
        m[1] = 0xc4;
        m[2] = (uint8_t)(len >> 8);
        m[3] = (uint8_t)len;
        m[4] = (uint8_t)(((w >> 1) << 4) | (w & 1));
      }
      if (lane < 16) m[5 + lane] = tb[1 + lane];
      for (uint32_t i = lane; i < nsym; i += 64) m[21 + i] = tb[17 + i];
    }
  }
  __syncthreads();
  const uint64_t cap = F.cap;
  const uint32_t hb = a.framed ? F.head_bytes[v] : 0, mb = a.framed ? F.mid_bytes[v] : 0;
  const uint32_t prefix = hb + dl + mb;
  for (uint32_t p = t; p < prefix && p < cap; p += 256)       // nothing is written at or beyond the capacity
    F.out[p] = p < hb ? F.head[v][p] : p < hb + dl ? dht[p - hb] : F.mid[v][p - hb - dl];
  if (a.framed && t < 2) {
    const uint64_t len = a.d_len[job];
    const uint64_t p = len - 2 + t;
    if (len >= 2 && p < cap) F.out[p] = t ? 0xd9 : 0xff;
  }
}

}  // namespace

void qs_launch_huff_optimal(const uint32_t* d_counts, int ntables, uint8_t* d_tables, int32_t* d_status, hipStream_t s) {
  hipLaunchKernelGGL(qh_optimal, dim3((ntables + QH_WAVES - 1) / QH_WAVES), dim3(64 * QH_WAVES), 0, s, d_counts, ntables,
                     d_tables, d_status);
}

void qs_launch_huff_tables(const QsHuffArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(qh_tables, dim3(a.n), dim3(64 * QH_WAVES), 0, s, a);
}

void qs_launch_huff_frame(const QsHuffArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(qh_frame, dim3(a.n), dim3(256), 0, s, a);
}
