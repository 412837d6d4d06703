// qs_kernels_encode.hip -- baseline sequential Huffman coding of device-resident coefficient arrays (gfx950): the
// entropy-coded segment libjpeg 9 writes for jpeg_write_coefficients (jchuff.c: encode_mcu_huff / encode_one_block,
// jctrans.c: compress_output for the dummy blocks of edge MCUs).  DESIGN.md section 13.
//
// One lane per block in scan order.  Every dependency between workgroups is a kernel boundary:
//   qe_init      zeroes the per-job state (and the histogram)
//   qe_size      code length of every block (or, histogram run, its symbol counts), summed per workgroup
//   qe_scan_bits one workgroup per job: exclusive 64-bit scan of the workgroup sums, zeroes the words of the
//                unstuffed stream that two workgroups share
//   qe_emit      code words, staged as whole 32-bit words in LDS, stored with consecutive lanes on consecutive words;
//                only a workgroup's first and last word can be shared with a neighbour and go through atomicOr
//   qe_ff_count / qe_ff_scan / qe_stuff   0xFF bytes per 4 KiB chunk, their scan, and the scatter with 0x00 inserted
#include <hip/hip_runtime.h>
#include "qs_encode.h"

namespace {

// jpeg_natural_order: zigzag position -> natural index
constexpr unsigned char QE_ZZ[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct QeShared {
  QsEncGeom g;
  QsEncPtrs p;
  uint32_t dc[2][16];
  uint32_t ac[2][256];
  uint32_t sc[QS_ENC_WG];
};

// exclusive scan over the workgroup's 256 lanes; *total = the sum
__device__ uint32_t qe_exscan(uint32_t v, uint32_t* sc, uint32_t* total) {
  const int t = threadIdx.x;
  sc[t] = v;
  __syncthreads();
  for (int d = 1; d < QS_ENC_WG; d <<= 1) {
    const uint32_t x = t >= d ? sc[t - d] : 0;
    __syncthreads();
    sc[t] += x;
    __syncthreads();
  }
  const uint32_t inc = sc[t];
  *total = sc[QS_ENC_WG - 1];
  __syncthreads();
  return inc - v;
}

// which job of the chunk owns workgroup `wg` (wg0 / nwg or swg0 / nswg: STUFF)
template <bool STUFF>
__device__ int qe_find_job(const QsEncArgs& a, int wg) {
  int k = 0;
  for (int i = 1; i < a.n; ++i)
    if (wg >= (STUFF ? a.swg0[i] : a.wg0[i])) k = i;
  return k;
}

__device__ int qe_variant(const QsEncArgs& a, const QsEncJob& J, int k) {
  return (J.two && a.d_stop && a.d_stop[a.job0 + k] != 0) ? 1 : 0;
}

// geometry of the chosen variant, the job's addresses and its code tables into LDS
__device__ void qe_stage(const QsEncArgs& a, const QsEncJob& J, int k, int variant, QeShared& S) {
  const int t = threadIdx.x;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&J.g[variant]);
  if (t < (int)(sizeof(QsEncGeom) / 4)) reinterpret_cast<uint32_t*>(&S.g)[t] = src[t];
  if (t == 0) S.p = a.p[k];
  if (t < 32) S.dc[t >> 4][t & 15] = J.dc[t >> 4][t & 15];
  S.ac[0][t] = J.ac[0][t];
  S.ac[1][t] = J.ac[1][t];
  __syncthreads();
}

// the DC libjpeg sees at block kk of component c in MCU m: the block's own where it exists, else (a dummy block of an
// edge MCU) the DC of the block before it in the MCU, which belongs to the same component (block 0 always exists)
__device__ int qe_dc(const QeShared& S, int m, int c, int kk) {
  const QsEncGeom& g = S.g;
  const int hs = g.hs[c], mx = m % g.mcus_x, my = m / g.mcus_x, slot = g.slot[c];
  for (; kk >= 0; --kk) {
    const int y = kk / hs, x = kk - y * hs;
    const int bx = mx * hs + x, by = my * g.vs[c] + y;
    if (bx < g.nw[c] && by < g.nh[c]) {
      const long long idx = (long long)by * g.stride[c] + bx;
      return idx < S.p.nblk[slot] ? S.p.coef[slot][idx * 64] : 0;
    }
  }
  return 0;
}

struct QeBlock {
  int16_t v[64];                   // natural order; all zero for a dummy block
  int diff;                        // DC difference to the previous block of the component in scan order
  int tb;                          // Huffman table of the component
};

// scan block b of the staged geometry
__device__ __forceinline__ void qe_load(const QeShared& S, const QsEncJob& J, int b, QeBlock& B) {
  const QsEncGeom& g = S.g;
  const int m = b / g.bpm, k = b - m * g.bpm;
  int c = 0;
  for (int ci = 1; ci < g.ncomp; ++ci)
    if (k >= g.first[ci]) c = ci;
  const int kk = k - g.first[c], hs = g.hs[c], slot = g.slot[c];
  const int y = kk / hs, x = kk - y * hs;
  const int bx = (m % g.mcus_x) * hs + x, by = (m / g.mcus_x) * g.vs[c] + y;
  B.tb = J.tbl[c];
  const long long idx = (long long)by * g.stride[c] + bx;
  const bool real = bx < g.nw[c] && by < g.nh[c] && idx < S.p.nblk[slot];
  if (real) {
    const uint4* p = reinterpret_cast<const uint4*>(S.p.coef[slot] + idx * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint4 q = p[i];
      B.v[8 * i + 0] = (int16_t)(q.x & 0xffff); B.v[8 * i + 1] = (int16_t)(q.x >> 16);
      B.v[8 * i + 2] = (int16_t)(q.y & 0xffff); B.v[8 * i + 3] = (int16_t)(q.y >> 16);
      B.v[8 * i + 4] = (int16_t)(q.z & 0xffff); B.v[8 * i + 5] = (int16_t)(q.z >> 16);
      B.v[8 * i + 6] = (int16_t)(q.w & 0xffff); B.v[8 * i + 7] = (int16_t)(q.w >> 16);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 64; ++i) B.v[i] = 0;
  }
  int prev = 0;
  if (kk > 0) prev = qe_dc(S, m, c, kk - 1);
  else if (m > 0) prev = qe_dc(S, m - 1, c, hs * g.vs[c] - 1);
  B.diff = real ? (int)B.v[0] - prev : 0;
}

// magnitude category and the bits libjpeg appends: v for v > 0, v - 1 for v < 0, in nb bits
__device__ __forceinline__ int qe_nbits(int v, uint32_t* bits) {
  const int t = v < 0 ? -v : v;
  const int nb = 32 - __clz(t);
  *bits = (uint32_t)(v + (v >> 31)) & ((1u << nb) - 1u);
  return nb;
}

template <int K, class Sink>
__device__ __forceinline__ void qe_ac_steps(const QeBlock& B, int& run, uint32_t& flags, Sink& s) {
  if constexpr (K < 64) {
    constexpr int z = QE_ZZ[K];
    const int v = B.v[z];
    if (v == 0) {
      ++run;
    } else {
      while (run > 15) {
        s.ac(B.tb, 0xF0, 0, 0);
        run -= 16;
      }
      uint32_t bits;
      int nb = qe_nbits(v, &bits);
      if (nb > 10) {                               // JERR_BAD_DCT_COEF (jchuff.c: nbits > MAX_COEF_BITS)
        flags |= QS_ENC_F_BADCOEF;
        nb = 10;
        bits &= 1023u;
      }
      s.ac(B.tb, (run << 4) | nb, bits, nb);
      run = 0;
    }
    qe_ac_steps<K + 1>(B, run, flags, s);
  }
}

// encode_one_block of jchuff.c on a sink that either measures or writes
template <class Sink>
__device__ __forceinline__ uint32_t qe_encode(const QeBlock& B, Sink& s) {
  uint32_t flags = 0, bits;
  int nb = qe_nbits(B.diff, &bits);
  if (nb > 11) {                                   // nbits > MAX_COEF_BITS + 1
    flags |= QS_ENC_F_BADCOEF;
    nb = 11;
    bits &= 2047u;
  }
  s.dc(B.tb, nb, bits);
  int run = 0;
  qe_ac_steps<1>(B, run, flags, s);
  if (run > 0) s.ac(B.tb, 0, 0, 0);
  return flags;
}

struct QeSizeSink {
  const QeShared& S;
  uint32_t bits = 0, flags = 0;
  __device__ explicit QeSizeSink(const QeShared& s) : S(s) {}
  __device__ __forceinline__ void put(uint32_t e, int nb) {
    const uint32_t sz = e >> 16;
    if (sz == 0) flags |= QS_ENC_F_NOCODE;
    bits += sz + nb;
  }
  __device__ __forceinline__ void dc(int tb, int cat, uint32_t) { put(S.dc[tb][cat], cat); }
  __device__ __forceinline__ void ac(int tb, int sym, uint32_t, int nb) { put(S.ac[tb][sym], nb); }
};

struct QeHistSink {
  uint32_t* h;                                     // LDS uint32[4][257]
  __device__ __forceinline__ void dc(int tb, int cat, uint32_t) { atomicAdd(&h[tb * 257 + cat], 1u); }
  __device__ __forceinline__ void ac(int tb, int sym, uint32_t, int) { atomicAdd(&h[(2 + tb) * 257 + sym], 1u); }
};

struct QeEmitSink {
  const QeShared& S;
  uint32_t* lds;                                   // the workgroup's words, zeroed
  uint64_t acc = 0;
  int n;                                           // pending bits in acc (< 32)
  uint32_t w;                                      // the word they belong to
  __device__ QeEmitSink(const QeShared& s, uint32_t* l, uint32_t bitpos) : S(s), lds(l), n(bitpos & 31), w(bitpos >> 5) {}
  __device__ __forceinline__ void put(uint32_t e, uint32_t val, int nb) {
    const int sz = (int)(e >> 16);
    acc = (acc << (sz + nb)) | ((uint64_t)(e & 0xffffu) << nb) | val;
    n += sz + nb;
    if (n >= 32) {
      n -= 32;
      if (w < QS_ENC_LDS_WORDS) atomicOr(&lds[w], (uint32_t)(acc >> n));
      ++w;
    }
  }
  __device__ __forceinline__ void dc(int tb, int cat, uint32_t bits) { put(S.dc[tb][cat], bits, cat); }
  __device__ __forceinline__ void ac(int tb, int sym, uint32_t bits, int nb) { put(S.ac[tb][sym], bits, nb); }
  __device__ __forceinline__ void flush() {
    if (n > 0 && w < QS_ENC_LDS_WORDS) atomicOr(&lds[w], (uint32_t)(acc << (32 - n)));
  }
};

__device__ QsEncState* qe_state(const QsEncArgs& a, const QsEncJob& J) {
  return reinterpret_cast<QsEncState*>(a.ws + J.off_state);
}

__global__ void __launch_bounds__(QS_ENC_WG) qe_init(QsEncArgs a) {
  const int k = blockIdx.x, t = threadIdx.x;
  const QsEncJob& J = a.jobs[k];
  if (t < (int)(sizeof(QsEncState) / 4)) reinterpret_cast<uint32_t*>(qe_state(a, J))[t] = 0;
  if (a.d_counts) {
    uint32_t* h = a.d_counts + (size_t)(a.job0 + k) * 4 * 257;
    for (int i = t; i < 4 * 257; i += QS_ENC_WG) h[i] = (i % 257 == 256) ? 1u : 0u;   // libjpeg's reserved symbol
  }
}

// histogram run: the only status it can meet is a coefficient out of range
__global__ void __launch_bounds__(64) qe_hist_status(QsEncArgs a) {
  const int k = blockIdx.x;
  if (threadIdx.x == 0 && a.d_status)
    a.d_status[a.job0 + k] = (qe_state(a, a.jobs[k])->flags & QS_ENC_F_BADCOEF) ? 1 : 0;
}

template <bool HIST>
__global__ void __launch_bounds__(QS_ENC_WG) qe_size(QsEncArgs a) {
  __shared__ QeShared S;
  __shared__ uint32_t hist[HIST ? 4 * 257 : 1];
  const int wg = blockIdx.x, t = threadIdx.x;
  const int k = qe_find_job<false>(a, wg);
  const QsEncJob& J = a.jobs[k];
  const int lw = wg - J.wg0;
  if (lw >= J.nwg) return;
  if (HIST)
    for (int i = t; i < 4 * 257; i += QS_ENC_WG) hist[i] = 0;
  qe_stage(a, J, k, qe_variant(a, J, k), S);
  const int b = lw * QS_ENC_WG + t;
  uint32_t bits = 0, flags = 0;
  if (b < S.g.nblocks) {
    QeBlock B;
    qe_load(S, J, b, B);
    if (HIST) {
      QeHistSink s{hist};
      flags = qe_encode(B, s);
    } else {
      QeSizeSink s(S);
      flags = qe_encode(B, s) | s.flags;
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
    reinterpret_cast<uint16_t*>(a.ws + J.off_bits)[b] = (uint16_t)bits;
    uint32_t total;
    qe_exscan(bits, S.sc, &total);
    if (t == 0) reinterpret_cast<uint32_t*>(a.ws + J.off_wgsum)[lw] = total;
  }
}

__global__ void __launch_bounds__(QS_ENC_WG) qe_scan_bits(QsEncArgs a) {
  __shared__ uint32_t sc[QS_ENC_WG];
  const int k = blockIdx.x, t = threadIdx.x;
  const QsEncJob& J = a.jobs[k];
  QsEncState* st = qe_state(a, J);
  if (st->flags) {                                 // (uniform: written by the kernel before this one)
    if (t == 0) st->dead = 1;
    return;
  }
  const uint32_t* wgsum = reinterpret_cast<const uint32_t*>(a.ws + J.off_wgsum);
  uint64_t* wgoff = reinterpret_cast<uint64_t*>(a.ws + J.off_wgoff);
  uint32_t* raw = reinterpret_cast<uint32_t*>(a.ws + J.off_raw);
  uint64_t carry = 0;
  for (int base = 0; base < J.nwg; base += QS_ENC_WG) {
    const int i = base + t;
    uint32_t total;
    const uint32_t ex = qe_exscan(i < J.nwg ? wgsum[i] : 0, sc, &total);
    if (i < J.nwg) {
      const uint64_t x = carry + ex;
      wgoff[i] = x;
      if ((x & 31) && (x >> 5) * 4 + 4 <= J.raw_cap) raw[x >> 5] = 0;      // the word two workgroups write into
    }
    carry += total;
  }
  if (t == 0) {
    if ((carry & 31) && (carry >> 5) * 4 + 4 <= J.raw_cap) raw[carry >> 5] = 0;
    st->total_bits = carry;
    st->raw_bytes = (carry + 7) >> 3;
    st->nchunks = (uint32_t)((st->raw_bytes + QS_ENC_SCHUNK - 1) / QS_ENC_SCHUNK);
  }
}

__global__ void __launch_bounds__(QS_ENC_WG) qe_emit(QsEncArgs a) {
  __shared__ QeShared S;
  __shared__ uint32_t words[QS_ENC_LDS_WORDS];
  const int wg = blockIdx.x, t = threadIdx.x;
  const int k = qe_find_job<false>(a, wg);
  const QsEncJob& J = a.jobs[k];
  const int lw = wg - J.wg0;
  if (lw >= J.nwg) return;
  if (qe_state(a, J)->dead) return;
  const uint32_t wgbits = reinterpret_cast<const uint32_t*>(a.ws + J.off_wgsum)[lw];
  if (wgbits == 0) return;
  const uint64_t s0 = reinterpret_cast<const uint64_t*>(a.ws + J.off_wgoff)[lw];
  const uint32_t lead = (uint32_t)(s0 & 31);
  const uint32_t nwords = (lead + wgbits + 31) >> 5;          // <= QS_ENC_LDS_WORDS: a block has at most QS_ENC_MAXBITS
  for (uint32_t i = t; i < nwords && i < QS_ENC_LDS_WORDS; i += QS_ENC_WG) words[i] = 0;
  qe_stage(a, J, k, qe_variant(a, J, k), S);                  // (its barrier also covers the zeroing)
  const int b = lw * QS_ENC_WG + t;
  const uint32_t mine = reinterpret_cast<const uint16_t*>(a.ws + J.off_bits)[b];
  uint32_t total;
  const uint32_t ex = qe_exscan(mine, S.sc, &total);
  if (b < S.g.nblocks && mine) {
    QeBlock B;
    qe_load(S, J, b, B);
    QeEmitSink s(S, words, lead + ex);
    qe_encode(B, s);
    s.flush();
  }
  __syncthreads();
  uint32_t* raw = reinterpret_cast<uint32_t*>(a.ws + J.off_raw);
  const uint64_t w0 = s0 >> 5;
  const bool tail_shared = ((s0 + wgbits) & 31) != 0;
  for (uint32_t i = t; i < nwords && i < QS_ENC_LDS_WORDS; i += QS_ENC_WG) {
    const uint64_t gw = w0 + i;
    if (gw * 4 + 4 > J.raw_cap) continue;
    const uint32_t v = __builtin_bswap32(words[i]);           // the stream is bytes, most significant bit first
    if ((i == 0 && lead) || (i == nwords - 1 && tail_shared)) atomicOr(&raw[gw], v);
    else raw[gw] = v;
  }
}

// the unstuffed byte at index idx (< U), the one-bits of the final byte's padding included
__device__ __forceinline__ uint32_t qe_raw_byte(uint32_t word, int j, uint64_t idx, uint64_t U, uint32_t padmask) {
  uint32_t b = (word >> (8 * j)) & 0xffu;
  if (idx == U - 1) b |= padmask;
  return b;
}

__global__ void __launch_bounds__(QS_ENC_WG) qe_ff_count(QsEncArgs a) {
  __shared__ uint32_t sc[QS_ENC_WG];
  const int wg = blockIdx.x, t = threadIdx.x;
  const int k = qe_find_job<true>(a, wg);
  const QsEncJob& J = a.jobs[k];
  const int lw = wg - J.swg0;
  if (lw >= J.nswg) return;
  const QsEncState* st = qe_state(a, J);
  if (st->dead) return;
  const uint64_t U = st->raw_bytes;
  const uint32_t rem = (uint32_t)(st->total_bits & 7), padmask = rem ? (1u << (8 - rem)) - 1u : 0u;
  const uint8_t* raw = a.ws + J.off_raw;
  uint32_t* ffcnt = reinterpret_cast<uint32_t*>(a.ws + J.off_ffcnt);
  for (uint32_t c = lw; c < st->nchunks; c += J.nswg) {
    const uint64_t off = (uint64_t)c * QS_ENC_SCHUNK + (uint64_t)t * 16;
    uint32_t cnt = 0;
    if (off < U && off + 16 <= J.raw_cap) {
      const uint4 q = *reinterpret_cast<const uint4*>(raw + off);
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (off + j < U) cnt += qe_raw_byte(w[j >> 2], j & 3, off + j, U, padmask) == 0xffu;
    }
    uint32_t total;
    qe_exscan(cnt, sc, &total);
    if (t == 0) ffcnt[c] = total;
  }
}

__global__ void __launch_bounds__(QS_ENC_WG) qe_ff_scan(QsEncArgs a) {
  __shared__ uint32_t sc[QS_ENC_WG];
  const int k = blockIdx.x, t = threadIdx.x;
  const QsEncJob& J = a.jobs[k];
  const QsEncState* st = qe_state(a, J);
  if (st->dead) {
    if (t == 0) {
      a.d_len[a.job0 + k] = 0;
      a.d_status[a.job0 + k] = (st->flags & QS_ENC_F_BADCOEF) ? 1 : 3;
    }
    return;
  }
  const uint32_t* ffcnt = reinterpret_cast<const uint32_t*>(a.ws + J.off_ffcnt);
  uint64_t* ffoff = reinterpret_cast<uint64_t*>(a.ws + J.off_ffoff);
  const uint32_t n = st->nchunks;
  uint64_t carry = 0;
  for (uint32_t base = 0; base < n; base += QS_ENC_WG) {
    const uint32_t i = base + t;
    uint32_t total;
    const uint32_t ex = qe_exscan(i < n ? ffcnt[i] : 0, sc, &total);
    if (i < n) ffoff[i] = carry + ex;
    carry += total;
  }
  if (t == 0) {
    const uint64_t len = st->raw_bytes + carry;
    a.d_len[a.job0 + k] = len;
    a.d_status[a.job0 + k] = len > a.p[k].cap ? 2 : 0;
  }
}

__global__ void __launch_bounds__(QS_ENC_WG) qe_stuff(QsEncArgs a) {
  __shared__ uint32_t sc[QS_ENC_WG];
  __shared__ uint8_t sb[2 * QS_ENC_SCHUNK];
  const int wg = blockIdx.x, t = threadIdx.x;
  const int k = qe_find_job<true>(a, wg);
  const QsEncJob& J = a.jobs[k];
  const int lw = wg - J.swg0;
  if (lw >= J.nswg) return;
  const QsEncState* st = qe_state(a, J);
  if (st->dead) return;
  const uint64_t U = st->raw_bytes, cap = a.p[k].cap;
  const uint32_t rem = (uint32_t)(st->total_bits & 7), padmask = rem ? (1u << (8 - rem)) - 1u : 0u;
  const uint8_t* raw = a.ws + J.off_raw;
  const uint64_t* ffoff = reinterpret_cast<const uint64_t*>(a.ws + J.off_ffoff);
  uint8_t* out = a.p[k].out;
  for (uint32_t c = lw; c < st->nchunks; c += J.nswg) {
    const uint64_t off = (uint64_t)c * QS_ENC_SCHUNK + (uint64_t)t * 16;
    uint32_t w[4] = {0, 0, 0, 0}, cnt = 0, nb = 0;
    if (off < U && off + 16 <= J.raw_cap) {
      const uint4 q = *reinterpret_cast<const uint4*>(raw + off);
      w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
      nb = (uint32_t)(U - off < 16 ? U - off : 16);
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (j < (int)nb) cnt += qe_raw_byte(w[j >> 2], j & 3, off + j, U, padmask) == 0xffu;
    }
    uint32_t total;
    const uint32_t ex = qe_exscan(cnt, sc, &total);
    uint32_t o = t * 16 + ex;                                  // < 2 * QS_ENC_SCHUNK with every byte stuffed
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < (int)nb) {
        const uint32_t b = qe_raw_byte(w[j >> 2], j & 3, off + j, U, padmask);
        sb[o++] = (uint8_t)b;
        if (b == 0xffu) sb[o++] = 0;
      }
    __syncthreads();
    const uint64_t c0 = (uint64_t)c * QS_ENC_SCHUNK;
    const uint64_t base = c0 + ffoff[c];
    uint64_t n = (U - c0 < QS_ENC_SCHUNK ? U - c0 : QS_ENC_SCHUNK) + total;
    if (base >= cap) n = 0;
    else if (n > cap - base) n = cap - base;                   // nothing is written at or beyond the capacity
    uint8_t* dst = out + base;
    uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
    if (head > n) head = (uint32_t)n;
    const uint32_t nw = (uint32_t)((n - head) >> 2), tail = (uint32_t)(n - head - 4 * (uint64_t)nw);
    if ((uint32_t)t < head) dst[t] = sb[t];
    for (uint32_t i = t; i < nw; i += QS_ENC_WG) {
      const uint8_t* s = sb + head + 4 * i;
      *reinterpret_cast<uint32_t*>(dst + head + 4 * i) =
          (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
    }
    if ((uint32_t)t < tail) dst[head + 4 * nw + t] = sb[head + 4 * nw + t];
    __syncthreads();
  }
}

}  // namespace

// what one run enqueues for a chunk of jobs: wgs / swgs = workgroups of the block kernels / the stuffing kernels
void qs_launch_encode(const QsEncArgs& a, int wgs, int swgs, hipStream_t s) {
  const dim3 lanes(QS_ENC_WG);
  hipLaunchKernelGGL(qe_init, dim3(a.n), lanes, 0, s, a);
  if (a.d_counts) {
    if (wgs > 0) hipLaunchKernelGGL(qe_size<true>, dim3(wgs), lanes, 0, s, a);
    hipLaunchKernelGGL(qe_hist_status, dim3(a.n), dim3(64), 0, s, a);
    return;
  }
  if (wgs > 0) hipLaunchKernelGGL(qe_size<false>, dim3(wgs), lanes, 0, s, a);
  hipLaunchKernelGGL(qe_scan_bits, dim3(a.n), lanes, 0, s, a);
  if (wgs > 0) hipLaunchKernelGGL(qe_emit, dim3(wgs), lanes, 0, s, a);
  if (swgs > 0) hipLaunchKernelGGL(qe_ff_count, dim3(swgs), lanes, 0, s, a);
  hipLaunchKernelGGL(qe_ff_scan, dim3(a.n), lanes, 0, s, a);
  if (swgs > 0) hipLaunchKernelGGL(qe_stuff, dim3(swgs), lanes, 0, s, a);
}
