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
//
// Restart intervals ("Restart intervals"): a chunk with a restart job runs the RST instantiations
// of the same seven kernels.  Every interval starts byte-aligned, so its padding follows from its own length; qe_size
// notes where each interval starts inside its workgroup, qe_scan_bits turns that into the paddings before each interval
// (D) and the byte each one starts at (P), qe_emit shifts every block by its interval's D and appends the pad one-bits
// behind an interval's last block, and the stuffing kernels put FF Dn in front of the byte an interval starts at.  A job
// without an interval in such a chunk is one interval: the same bytes.
//
// The whole-file run (qs_kernels_huff.hip) drives the same kernels with three pointers into its
// scratch set in QsEncArgs: qe_stage takes the code words from there, qe_ff_scan and qe_stuff place the segment behind a
// per-job prefix.  All three are null in every other run, which reads the descriptors and a prefix of 0 as before.
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
// (this and the three helpers below are inlined by force: the compiler stops inlining into a kernel of more than 1100
// basic blocks, which the AC refinement's emit kernel is, and a helper that is called takes the kernel's arguments by
// address -- a copy of all of them in scratch)
__device__ __forceinline__ uint32_t qe_exscan(uint32_t v, uint32_t* sc, uint32_t* total) {
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
__device__ __forceinline__ int qe_find_job(const QsEncArgs& a, int wg) {
  int k = 0;
  for (int i = 1; i < a.n; ++i)
    if (wg >= (STUFF ? a.swg0[i] : a.wg0[i])) k = i;
  return k;
}

__device__ __forceinline__ int qe_variant(const QsEncArgs& a, const QsEncJob& J, int k) {
  return (J.two && a.d_stop && a.d_stop[a.job0 + k] != 0) ? 1 : 0;
}

// geometry of the chosen variant, the job's addresses and its code tables into LDS
__device__ __forceinline__ void qe_stage(const QsEncArgs& a, const QsEncJob& J, int k, int variant, QeShared& S) {
  const int t = threadIdx.x;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&J.g[variant]);
  if (t < (int)(sizeof(QsEncGeom) / 4)) reinterpret_cast<uint32_t*>(&S.g)[t] = src[t];
  if (t == 0) S.p = a.p[k];
  // the code words: the descriptor's, or (whole-file run with optimize) what the table kernel left in the scratch
  const uint32_t* dc = a.codes ? a.codes + (size_t)(a.job0 + k) * QS_ENC_CODES : &J.dc[0][0];
  const uint32_t* ac = a.codes ? dc + 2 * 16 : &J.ac[0][0];
  if (t < 32) S.dc[t >> 4][t & 15] = dc[t];
  S.ac[0][t] = ac[t];
  S.ac[1][t] = ac[256 + t];
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

// blocks per restart interval of the chosen variant (the whole scan without one)
__device__ __forceinline__ int qe_per(const QeShared& S, const QsEncJob& J, int variant) {
  const int ri = J.ri[variant];
  return (ri ? ri : S.g.mcus) * S.g.bpm;
}

// scan block b of the staged geometry; ri: the restart interval in MCUs (0: none) -- DC prediction starts at 0 there
__device__ __forceinline__ void qe_load(const QeShared& S, const QsEncJob& J, int b, int ri, QeBlock& B) {
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
  else if (m > 0 && !(ri && m % ri == 0)) prev = qe_dc(S, m - 1, c, hs * g.vs[c] - 1);
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
  uint32_t limit;                                  // words the workgroup staged
  __device__ QeEmitSink(const QeShared& s, uint32_t* l, uint32_t bitpos, uint32_t lim)
      : S(s), lds(l), n(bitpos & 31), w(bitpos >> 5), limit(lim) {}
  __device__ __forceinline__ void raw(uint64_t val, int nb) {   // nb <= 32 bits
    acc = (acc << nb) | val;
    n += nb;
    if (n >= 32) {
      n -= 32;
      if (w < limit) atomicOr(&lds[w], (uint32_t)(acc >> n));
      ++w;
    }
  }
  __device__ __forceinline__ void put(uint32_t e, uint32_t val, int nb) {
    raw(((uint64_t)(e & 0xffffu) << nb) | val, (int)(e >> 16) + nb);
  }
  __device__ __forceinline__ void dc(int tb, int cat, uint32_t bits) { put(S.dc[tb][cat], bits, cat); }
  __device__ __forceinline__ void ac(int tb, int sym, uint32_t bits, int nb) { put(S.ac[tb][sym], bits, nb); }
  __device__ __forceinline__ void flush() {
    if (n > 0 && w < limit) atomicOr(&lds[w], (uint32_t)(acc << (32 - n)));
  }
};

__device__ QsEncState* qe_state(const QsEncArgs& a, const QsEncJob& J) {
  return reinterpret_cast<QsEncState*>(a.ws + J.off_state);
}

__global__ void __launch_bounds__(QS_ENC_WG) qe_init(QsEncArgs a) {
  const int k = blockIdx.x, t = threadIdx.x;
  const QsEncJob& J = a.jobs[k];
  if (t < (int)(sizeof(QsEncState) / 4)) reinterpret_cast<uint32_t*>(qe_state(a, J))[t] = 0;
  if (t == 0 && a.prefix && !a.codes) a.prefix[a.job0 + k] = a.fixed[k][qe_variant(a, J, k)];
  if (a.d_counts) {
    uint32_t* h = a.d_counts + (size_t)(a.job0 + k) * 4 * 257;
    for (int i = t; i < 4 * 257; i += QS_ENC_WG) h[i] = (i % 257 == 256) ? 1u : 0u;   // libjpeg's reserved symbol
  }
}

// histogram run: the only status it can meet is a coefficient out of range
__global__ void __launch_bounds__(64) qe_hist_status(QsEncArgs a) {
  const int k = blockIdx.x;
  if (threadIdx.x == 0 && a.d_status) {
    const QsEncJob& J = a.jobs[k];
    a.d_status[a.job0 + k] = (!a.restart && (J.ri[0] | J.ri[1])) ? 4 : (qe_state(a, J)->flags & QS_ENC_F_BADCOEF) ? 1 : 0;
  }
}

template <bool HIST, bool RST>
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
  const int variant = qe_variant(a, J, k);
  qe_stage(a, J, k, variant, S);
  const int b = lw * QS_ENC_WG + t;
  uint32_t bits = 0, flags = 0;
  if (b < S.g.nblocks) {
    QeBlock B;
    qe_load(S, J, b, RST ? J.ri[variant] : 0, B);
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
    const uint32_t ex = qe_exscan(bits, S.sc, &total);
    if (t == 0) reinterpret_cast<uint32_t*>(a.ws + J.off_wgsum)[lw] = total;
    if (RST && b < S.g.nblocks) {                    // where an interval starts inside its workgroup
      const int per = qe_per(S, J, variant);
      if (b % per == 0) reinterpret_cast<uint32_t*>(a.ws + J.off_rrel)[b / per] = ex;
    }
  }
}

// intervals one lane of qe_scan_bits<true> takes per step of its scan over the intervals
constexpr int QE_RST_RUN = 16;

template <bool RST>
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
      if (!RST && (x & 31) && (x >> 5) * 4 + 4 <= J.raw_cap) raw[x >> 5] = 0;   // the word two workgroups write into
    }
    carry += total;
  }
  if (RST) {
    // C(r): the unpadded bits before interval r.  Interval r is padded by (-(C(r + 1) - C(r))) mod 8, since it starts
    // on a byte; D(r) = the paddings before it, P(r) = (C(r) + D(r)) / 8 the byte it starts at
    const int variant = qe_variant(a, J, k);
    const QsEncGeom& g = J.g[variant];
    const int per = (J.ri[variant] ? J.ri[variant] : g.mcus) * g.bpm;
    const int nint = (g.nblocks + per - 1) / per;
    const uint32_t* rrel = reinterpret_cast<const uint32_t*>(a.ws + J.off_rrel);
    uint64_t* rd = reinterpret_cast<uint64_t*>(a.ws + J.off_rd);
    uint64_t* rp = reinterpret_cast<uint64_t*>(a.ws + J.off_rp);
    const uint64_t bits = carry;
    __syncthreads();                                 // wgoff is read back below
    auto C = [&](int r) -> uint64_t {
      return r < nint ? wgoff[((long long)r * per) / QS_ENC_WG] + rrel[r] : bits;
    };
    uint64_t dcarry = 0;
    for (long long base = 0; base < nint; base += (long long)QS_ENC_WG * QE_RST_RUN) {
      const long long r0 = base + (long long)t * QE_RST_RUN;
      uint64_t c[QE_RST_RUN + 1];
      uint32_t sum = 0;
      if (r0 < nint) c[0] = C((int)r0);
#pragma unroll
      for (int e = 0; e < QE_RST_RUN; ++e)
        if (r0 + e < nint) {
          c[e + 1] = C((int)(r0 + e + 1));
          sum += (uint32_t)(0 - (c[e + 1] - c[e])) & 7u;
        }
      uint32_t total;
      uint64_t d = dcarry + qe_exscan(sum, sc, &total);
#pragma unroll
      for (int e = 0; e < QE_RST_RUN; ++e)
        if (r0 + e < nint) {
          rd[r0 + e] = d;
          rp[r0 + e] = (c[e] + d) >> 3;
          d += (uint32_t)(0 - (c[e + 1] - c[e])) & 7u;
        }
      dcarry += total;
    }
    if (t == 0) {
      rd[nint] = dcarry;
      rp[nint] = (bits + dcarry) >> 3;
    }
    __syncthreads();                                 // rd is read back below
    for (int i = t; i < J.nwg; i += QS_ENC_WG) {
      const long long b0 = (long long)i * QS_ENC_WG;
      if (b0 >= g.nblocks) break;
      const uint64_t x = wgoff[i] + rd[b0 / per];
      if ((x & 31) && (x >> 5) * 4 + 4 <= J.raw_cap) raw[x >> 5] = 0;          // the word two workgroups write into
    }
    carry += dcarry;                                 // a whole number of bytes: no padding left for the stuffing kernels
  }
  if (t == 0) {
    if ((carry & 31) && (carry >> 5) * 4 + 4 <= J.raw_cap) raw[carry >> 5] = 0;
    st->total_bits = carry;
    st->raw_bytes = (carry + 7) >> 3;
    st->nchunks = (uint32_t)((st->raw_bytes + QS_ENC_SCHUNK - 1) / QS_ENC_SCHUNK);
  }
}

template <bool RST>
__global__ void __launch_bounds__(QS_ENC_WG) qe_emit(QsEncArgs a) {
  constexpr uint32_t LDS_WORDS = RST ? QS_ENC_LDS_WORDS_RST : QS_ENC_LDS_WORDS;
  __shared__ QeShared S;
  __shared__ uint32_t words[LDS_WORDS];
  const int wg = blockIdx.x, t = threadIdx.x;
  const int k = qe_find_job<false>(a, wg);
  const QsEncJob& J = a.jobs[k];
  const int lw = wg - J.wg0;
  if (lw >= J.nwg) return;
  if (qe_state(a, J)->dead) return;
  uint32_t wgbits = reinterpret_cast<const uint32_t*>(a.ws + J.off_wgsum)[lw];
  if (wgbits == 0) return;
  uint64_t s0 = reinterpret_cast<const uint64_t*>(a.ws + J.off_wgoff)[lw];
  const int variant = qe_variant(a, J, k);
  // restart variant: the blocks of interval r lie D(r) bits further on, and the last block of an interval is followed
  // by its padding, D(r + 1) - D(r) one-bits
  const uint64_t* rd = reinterpret_cast<const uint64_t*>(a.ws + J.off_rd);
  int per = 1;
  uint64_t d0 = 0;
  auto ends = [&](int blk, int nblocks) { return (blk + 1) % per == 0 || blk == nblocks - 1; };
  if (RST) {
    const QsEncGeom& g = J.g[variant];
    per = (J.ri[variant] ? J.ri[variant] : g.mcus) * g.bpm;
    const int b0 = lw * QS_ENC_WG, bl = min(b0 + QS_ENC_WG, g.nblocks) - 1;
    d0 = rd[b0 / per];
    s0 += d0;
    wgbits += (uint32_t)(rd[bl / per + (ends(bl, g.nblocks) ? 1 : 0)] - d0);
  }
  const uint32_t lead = (uint32_t)(s0 & 31);
  const uint32_t nwords = (lead + wgbits + 31) >> 5;          // <= LDS_WORDS: a block has at most QS_ENC_MAXBITS
  for (uint32_t i = t; i < nwords && i < LDS_WORDS; i += QS_ENC_WG) words[i] = 0;
  qe_stage(a, J, k, variant, S);                              // (its barrier also covers the zeroing)
  const int b = lw * QS_ENC_WG + t;
  const uint32_t mine = reinterpret_cast<const uint16_t*>(a.ws + J.off_bits)[b];
  uint32_t total;
  const uint32_t ex = qe_exscan(mine, S.sc, &total);
  if (b < S.g.nblocks && mine) {
    QeBlock B;
    qe_load(S, J, b, RST ? J.ri[variant] : 0, B);
    uint32_t shift = 0, pad = 0;
    if (RST) {
      const int r = b / per;
      const uint64_t d = rd[r];
      shift = (uint32_t)(d - d0);
      if (ends(b, S.g.nblocks)) pad = (uint32_t)(rd[r + 1] - d);
    }
    QeEmitSink s(S, words, lead + ex + shift, LDS_WORDS);
    qe_encode(B, s);
    if (RST && pad) s.raw((1u << pad) - 1u, (int)pad);
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

// the unstuffed byte at index idx (< U), the one-bits of the final byte's padding included
__device__ __forceinline__ uint32_t qe_raw_byte(uint32_t word, int j, uint64_t idx, uint64_t U, uint32_t padmask) {
  uint32_t b = (word >> (8 * j)) & 0xffu;
  if (idx == U - 1) b |= padmask;
  return b;
}

// Restart markers in the stuffing stage.  rp[1 .. nint - 1] are the bytes of the unstuffed stream that start an interval
// after the first, strictly increasing (an interval holds at least one byte); FF Dn goes in front of each.
// -> the first r in [lo, hi] with rp[r] >= off (hi: none), for 1 <= lo <= hi <= nint
__device__ __forceinline__ int qe_rst_first(const uint64_t* rp, int lo, int hi, uint64_t off) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (rp[mid] < off) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// interval starts among the 16 bytes at off, r the first candidate (never more than 16, whatever rp holds: the staging
// buffer of qe_stuff is sized by it)
__device__ __forceinline__ uint32_t qe_rst_count(const uint64_t* rp, int nint, int r, uint64_t off) {
  uint32_t n = 0;
  for (; n < 16 && r < nint && rp[r] < off + 16; ++r) ++n;
  return n;
}

__device__ __forceinline__ int qe_nint(const QsEncArgs& a, const QsEncJob& J, int k) {
  const int variant = qe_variant(a, J, k);
  const QsEncGeom& g = J.g[variant];
  const int per = (J.ri[variant] ? J.ri[variant] : g.mcus) * g.bpm;
  return (g.nblocks + per - 1) / per;
}

template <bool RST>
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
  const uint64_t* rp = reinterpret_cast<const uint64_t*>(a.ws + J.off_rp);
  const int nint = RST ? qe_nint(a, J, k) : 1;
  for (uint32_t c = lw; c < st->nchunks; c += J.nswg) {
    const uint64_t off = (uint64_t)c * QS_ENC_SCHUNK + (uint64_t)t * 16;
    uint32_t cnt = 0;
    int rlo = 1, rhi = 1;                                       // the interval starts of this chunk: one search for all lanes
    if (RST && nint > 1) {
      rlo = qe_rst_first(rp, 1, nint, (uint64_t)c * QS_ENC_SCHUNK);
      rhi = qe_rst_first(rp, rlo, nint, (uint64_t)(c + 1) * QS_ENC_SCHUNK);
    }
    if (off < U && off + 16 <= J.raw_cap) {
      const uint4 q = *reinterpret_cast<const uint4*>(raw + off);
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (off + j < U) cnt += qe_raw_byte(w[j >> 2], j & 3, off + j, U, padmask) == 0xffu;
      if (RST && nint > 1)                                      // two bytes per marker in front of one of these bytes
        cnt += 2 * qe_rst_count(rp, nint, qe_rst_first(rp, rlo, rhi, off), off);
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
  if (!a.restart && (J.ri[0] | J.ri[1])) {         // prepared with a restart interval, run by the kernels without: the
    if (t == 0) {                                  // host did not know the workspace (qs_encode_job.cpp, prepared())
      a.d_len[a.job0 + k] = 0;
      a.d_status[a.job0 + k] = 4;
    }
    return;
  }
  const bool clen = a.tstatus && a.tstatus[a.job0 + k] != 0;     // a table with a code length above 32: status 5
  if (st->dead || clen) {
    if (t == 0) {
      a.d_len[a.job0 + k] = 0;
      a.d_status[a.job0 + k] = (st->flags & QS_ENC_F_BADCOEF) ? 1 : clen ? 5 : 3;
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
    // (whole-file run: the bytes in front of the segment and behind it count)
    const uint64_t len = (a.prefix ? a.prefix[a.job0 + k] : 0) + st->raw_bytes + carry + a.tail;
    a.d_len[a.job0 + k] = len;
    a.d_status[a.job0 + k] = len > a.p[k].cap ? 2 : 0;
  }
}

template <bool RST>
__global__ void __launch_bounds__(QS_ENC_WG) qe_stuff(QsEncArgs a) {
  __shared__ uint32_t sc[QS_ENC_WG];
  __shared__ uint8_t sb[(RST ? 4 : 2) * QS_ENC_SCHUNK];        // restart variant: a marker in front of every byte at most
  const int wg = blockIdx.x, t = threadIdx.x;
  const int k = qe_find_job<true>(a, wg);
  const QsEncJob& J = a.jobs[k];
  const int lw = wg - J.swg0;
  if (lw >= J.nswg) return;
  const QsEncState* st = qe_state(a, J);
  if (st->dead || (a.tstatus && a.tstatus[a.job0 + k] != 0)) return;
  const uint64_t U = st->raw_bytes, cap = a.p[k].cap;
  const uint64_t prefix = a.prefix ? a.prefix[a.job0 + k] : 0;    // whole-file run: where the segment starts in the buffer
  const uint32_t rem = (uint32_t)(st->total_bits & 7), padmask = rem ? (1u << (8 - rem)) - 1u : 0u;
  const uint8_t* raw = a.ws + J.off_raw;
  const uint64_t* ffoff = reinterpret_cast<const uint64_t*>(a.ws + J.off_ffoff);
  uint8_t* out = a.p[k].out;
  const uint64_t* rp = reinterpret_cast<const uint64_t*>(a.ws + J.off_rp);
  const int nint = RST ? qe_nint(a, J, k) : 1;
  for (uint32_t c = lw; c < st->nchunks; c += J.nswg) {
    const uint64_t off = (uint64_t)c * QS_ENC_SCHUNK + (uint64_t)t * 16;
    uint32_t w[4] = {0, 0, 0, 0}, cnt = 0, nb = 0;
    int rnext = nint;                                          // the next interval start at or behind this lane's bytes
    int rlo = 1, rhi = 1;                                      // the interval starts of this chunk: one search for all lanes
    if (RST && nint > 1) {
      rlo = qe_rst_first(rp, 1, nint, (uint64_t)c * QS_ENC_SCHUNK);
      rhi = qe_rst_first(rp, rlo, nint, (uint64_t)(c + 1) * QS_ENC_SCHUNK);
    }
    if (off < U && off + 16 <= J.raw_cap) {
      const uint4 q = *reinterpret_cast<const uint4*>(raw + off);
      w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
      nb = (uint32_t)(U - off < 16 ? U - off : 16);
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (j < (int)nb) cnt += qe_raw_byte(w[j >> 2], j & 3, off + j, U, padmask) == 0xffu;
      if (RST && nint > 1) {
        rnext = qe_rst_first(rp, rlo, rhi, off);
        cnt += 2 * qe_rst_count(rp, nint, rnext, off);
      }
    }
    uint32_t total;
    const uint32_t ex = qe_exscan(cnt, sc, &total);
    uint32_t o = t * 16 + ex;                                  // < sizeof sb with every byte stuffed (and marked)
    uint64_t pnext = (RST && rnext < nint) ? rp[rnext] : ~0ull;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < (int)nb) {
        if (RST && off + j == pnext) {                         // RSTn, n = (intervals before this one - 1) mod 8
          sb[o++] = 0xff;
          sb[o++] = (uint8_t)(0xd0 + ((rnext - 1) & 7));
          ++rnext;
          pnext = rnext < nint ? rp[rnext] : ~0ull;
        }
        const uint32_t b = qe_raw_byte(w[j >> 2], j & 3, off + j, U, padmask);
        sb[o++] = (uint8_t)b;
        if (b == 0xffu) sb[o++] = 0;
      }
    __syncthreads();
    const uint64_t c0 = (uint64_t)c * QS_ENC_SCHUNK;
    const uint64_t base = prefix + c0 + ffoff[c];
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

namespace {

template <bool RST>
void qe_launch(const QsEncArgs& a, int wgs, int swgs, hipStream_t s) {
  const dim3 lanes(QS_ENC_WG);
  hipLaunchKernelGGL(qe_init, dim3(a.n), lanes, 0, s, a);
  if (a.d_counts) {
    if (wgs > 0) hipLaunchKernelGGL((qe_size<true, RST>), dim3(wgs), lanes, 0, s, a);
    hipLaunchKernelGGL(qe_hist_status, dim3(a.n), dim3(64), 0, s, a);
    return;
  }
  if (wgs > 0) hipLaunchKernelGGL((qe_size<false, RST>), dim3(wgs), lanes, 0, s, a);
  hipLaunchKernelGGL(qe_scan_bits<RST>, dim3(a.n), lanes, 0, s, a);
  if (wgs > 0) hipLaunchKernelGGL(qe_emit<RST>, dim3(wgs), lanes, 0, s, a);
  if (swgs > 0) hipLaunchKernelGGL(qe_ff_count<RST>, dim3(swgs), lanes, 0, s, a);
  hipLaunchKernelGGL(qe_ff_scan, dim3(a.n), lanes, 0, s, a);
  if (swgs > 0) hipLaunchKernelGGL(qe_stuff<RST>, dim3(swgs), lanes, 0, s, a);
}

}  // namespace

// what one run enqueues for a chunk of jobs: wgs / swgs = workgroups of the block kernels / the stuffing kernels;
// restart: a job of the chunk has a restart interval (the restart instantiations of the same kernels)
void qs_launch_encode(const QsEncArgs& a, int wgs, int swgs, bool restart, hipStream_t s) {
  if (restart) qe_launch<true>(a, wgs, swgs, s);
  else qe_launch<false>(a, wgs, swgs, s);
}

// the progressive run: its kernels stand on the ones above
#include "qs_kernels_encode_prog.inc"
