// qs_huff.h -- the optimal Huffman table of JPEG Annex K.2 as libjpeg 9d carries it out (jchuff.c, jpeg_gen_optimal_table):
// what the table kernel (csrc/qs_kernels_huff.hip), the host entry point qs_hip_huff_optimal (csrc/qs_encode_job.cpp)
// and a plain host build (tests/huff_host.cpp) share.  DESIGN.md section 16.
//
// One wave makes one table.  The 257 symbols (256 counted ones and libjpeg's reserved pseudo-symbol 256, which counts 1
// so that no real symbol gets the all-ones code) sit in registers: symbol s in lane s & 63, slot s >> 6, five slots.
// The procedure is written once, over "every lane": on the device that is the lane itself and the wave-wide minimum is
// a __shfl_xor butterfly; on the host it is a loop over 64 lanes and a loop for the minimum -- the CPU suite and a
// sanitizer run the statements a lane runs.
//
// A merge step of Huffman's procedure takes c1 = the live symbol of least count (the larger index on a tie) and c2 = the
// same without c1: the two smallest keys (count << 9 | 511 - index) of the wave, found in ONE butterfly that carries the
// pair.  freq[c1] += freq[c2], freq[c2] = 0.  libjpeg then walks the others[] chains of both trees and adds one to every
// member's code size; here every symbol carries the index of its tree's representative -- the index libjpeg keeps the
// tree's sum under -- and every symbol whose representative is c1 or c2 gets size + 1 and representative c1.  The same
// sets, the same sums under the same indices: the same ties, the same sizes.
//
// Bounds, for every loop here:
//   * the merge loop runs at most 256 times (257 leaves), and ends early when no second live symbol exists;
//   * the cut-back of figure K.3 moves two codes per step out of a length above 16: fewer than 257 * 16 steps, and its
//     search for a shorter length in use stops at length 1;
//   * the search for the longest length in use (the reserved symbol leaves it) stops at length 1: counts that are all
//     zero give bits all 0, no symbols and success;
//   * every other loop has a constant trip count (slots, 64 lanes, 6 butterfly steps, 257 symbols, 32 lengths).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define QS_HF_HD __host__ __device__ inline
#else
#define QS_HF_HD static inline
#endif

#define QS_HF_OK 0
#define QS_HF_CLEN 5               // a code length above 32: libjpeg's JERR_HUFF_CLEN_OVERFLOW
#define QS_HF_MAXLEN 32
#define QS_HF_DEAD (~0ull)

#if defined(__HIP_DEVICE_COMPILE__)
#define QS_HF_NL 1                 // lanes one thread of control stands for
#define QS_HF_LANES for (int li = 0, lane = (int)(threadIdx.x & 63); li < 1; ++li)
#define QS_HF_SYNC() __syncthreads()
#else
#define QS_HF_NL 64
#define QS_HF_LANES for (int li = 0, lane = 0; li < 64; ++li, ++lane)
#define QS_HF_SYNC() ((void)0)
#endif

// what one wave keeps in LDS (the host: anywhere) while it makes a table, and where it leaves the result
struct QsHuffShared {
  uint32_t cnt[256];               // the counts, for the ranks
  int32_t bits[QS_HF_MAXLEN + 1];  // codes of each length before and while they are cut back
  int32_t status;
  int32_t nsym;                    // symbols in huffval
  uint8_t size[260];               // code size of symbol 0 .. 256, 255 standing for anything longer
  uint8_t outbits[20];             // [0 .. 16]: the DHT's counts
  uint8_t huffval[256];
};

// the two smallest keys of the wave (all keys differ, or are QS_HF_DEAD), the same in every lane
QS_HF_HD void qs_huff_wave_min2(const uint64_t* a, const uint64_t* b, uint64_t* k1, uint64_t* k2) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint64_t x = a[0], y = b[0];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t ox = __shfl_xor((unsigned long long)x, d), oy = __shfl_xor((unsigned long long)y, d);
    const uint64_t lo = x < ox ? x : ox, hi = x < ox ? ox : x, m = y < oy ? y : oy;
    x = lo;
    y = hi < m ? hi : m;
  }
  *k1 = x;
  *k2 = y;
#else
  uint64_t x = QS_HF_DEAD, y = QS_HF_DEAD;
  for (int l = 0; l < 64; ++l) {
    const uint64_t v[2] = {a[l], b[l]};
    for (int e = 0; e < 2; ++e) {
      if (v[e] < x) { y = x; x = v[e]; }
      else if (v[e] < y) y = v[e];
    }
  }
  *k1 = x;
  *k2 = y;
#endif
}

// counts[0 .. 255] (null: all zero) -> S.outbits[0 .. 16], S.huffval[0 .. S.nsym), the rest of huffval 0; returns
// QS_HF_OK or QS_HF_CLEN (bits and symbols are then all 0).  Device: called by every lane of every wave of the
// workgroup (it meets barriers), each wave with its own S.
QS_HF_HD int qs_huff_wave(const uint32_t* counts, QsHuffShared& S) {
  uint64_t freq[QS_HF_NL][5];
  int32_t rep[QS_HF_NL][5], size[QS_HF_NL][5];
  QS_HF_LANES {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int s = k * 64 + lane;
      const uint32_t c = s < 256 ? (counts ? counts[s] : 0u) : (s == 256 ? 1u : 0u);
      freq[li][k] = c;
      rep[li][k] = s;
      size[li][k] = 0;
      if (s < 256) {
        S.cnt[s] = c;
        S.huffval[s] = 0;
      }
    }
    if (lane <= QS_HF_MAXLEN) S.bits[lane] = 0;
    if (lane <= 16) S.outbits[lane] = 0;
  }
  for (int m = 0; m < 256; ++m) {
    uint64_t a[QS_HF_NL], b[QS_HF_NL], k1, k2;
    QS_HF_LANES {
      uint64_t x = QS_HF_DEAD, y = QS_HF_DEAD;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const uint64_t f = freq[li][k];
        const uint64_t key = f ? (f << 9) | (uint64_t)(511 - (k * 64 + lane)) : QS_HF_DEAD;
        if (key < x) { y = x; x = key; }
        else if (key < y) y = key;
      }
      a[li] = x;
      b[li] = y;
    }
    qs_huff_wave_min2(a, b, &k1, &k2);
    if (k2 == QS_HF_DEAD) break;                     // one tree left (k1: the reserved symbol alone when nothing counts)
    const int c1 = 511 - (int)(k1 & 511), c2 = 511 - (int)(k2 & 511);
    const uint64_t f2 = k2 >> 9;
    QS_HF_LANES {
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int s = k * 64 + lane;
        if (s == c1) freq[li][k] += f2;
        if (s == c2) freq[li][k] = 0;
        if (rep[li][k] == c1 || rep[li][k] == c2) {
          ++size[li][k];
          rep[li][k] = c1;
        }
      }
    }
  }
  QS_HF_LANES {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int s = k * 64 + lane;
      if (s <= 256) S.size[s] = (uint8_t)(size[li][k] > 255 ? 255 : size[li][k]);
    }
  }
  QS_HF_SYNC();
  // lane l in 1 .. 32 counts the codes of length l, lane 0 those that are longer
  QS_HF_LANES {
    if (lane <= QS_HF_MAXLEN) {
      int n = 0;
      for (int s = 0; s <= 256; ++s) n += lane ? (S.size[s] == lane) : (S.size[s] > QS_HF_MAXLEN);
      if (lane) S.bits[lane] = n;
      else S.status = n ? QS_HF_CLEN : QS_HF_OK;
    }
  }
  QS_HF_SYNC();
  QS_HF_LANES {
    if (lane == 0 && S.status == QS_HF_OK) {
      int32_t* bits = S.bits;
      int steps = 0, i;
      for (i = QS_HF_MAXLEN; i > 16; --i)            // figure K.3
        while (bits[i] > 0) {
          int j = i - 2;
          while (j > 0 && bits[j] == 0) --j;
          if (j == 0 || ++steps >= 257 * 16) {       // (not the counts of a code tree)
            S.status = QS_HF_CLEN;
            break;
          }
          bits[i] -= 2;
          ++bits[i - 1];
          bits[j + 1] += 2;
          --bits[j];
        }
      if (S.status == QS_HF_OK) {
        for (i = 16; i > 0 && bits[i] == 0;) --i;    // the reserved symbol leaves the longest length in use
        if (i > 0) --bits[i];
        for (int l = 1; l <= 16; ++l) S.outbits[l] = (uint8_t)bits[l];
      }
    }
  }
  QS_HF_SYNC();
  // libjpeg 9d lists the counted symbols by falling count, equal counts by rising value: a symbol's place is the number
  // of symbols in front of it
  const bool ok = S.status == QS_HF_OK;
  QS_HF_LANES {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int s = k * 64 + lane;
      const uint32_t c = S.cnt[s];
      if (c && ok) {
        int r = 0;
        for (int t = 0; t < 256; ++t) {
          const uint32_t ct = S.cnt[t];
          r += (ct > c) || (ct == c && t < s);
        }
        S.huffval[r] = (uint8_t)s;
      }
    }
  }
  QS_HF_SYNC();
  QS_HF_LANES {
    if (lane == 0) {
      int n = 0;
      for (int l = 1; l <= 16; ++l) n += S.outbits[l];
      S.nsym = n;
    }
  }
  QS_HF_SYNC();
  return S.status;
}
