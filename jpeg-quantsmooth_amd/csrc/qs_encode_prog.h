// qs_encode_prog.h -- progressive JPEG files (spectral selection; refinement scans, Ah > 0, behind QS_HIP_PROG_REFINE) from
// device-resident coefficient arrays
// (qs_hip_encode_progressive_device_batch_*): what the kernels (csrc/qs_kernels_encode_prog.inc), the host driver
// (csrc/qs_encode_prog_job.cpp) and the plain host builds (tests/encode_prog_host.cpp, tests/encode_refine_host.cpp) share.
// DESIGN.md sections 17 and 17.1.
//
// The file is head (SOI .. SOF2, the caller's) | per scan: the DHT markers of the scan's own optimal tables, DRI where
// the scan's interval differs from the last one written, the SOS header, the entropy-coded segment | EOI -- what
// libjpeg 9 writes for jpeg_write_coefficients with cinfo.scan_info set (jcmaster.c validate_script / per_scan_setup,
// jchuff.c encode_mcu_DC_first / encode_mcu_AC_first / emit_eobrun, jcmarker.c write_scan_header).
//
// Worst case of one block, in bits, which sizes the unstuffed stream of a scan and the emit kernel's LDS image:
//   DC scan   16 + 11                                  (one category code and its bits)
//   AC scan   (Se - Ss + 1) * (16 + 10) + (16 + 14)    (every band coefficient a symbol of its own, plus one EOB-run
//                                                       symbol with up to 14 appended bits, written by the run's last block)
// A 1..63 band gives 1668 bits = 208.5 bytes: more than the baseline coder's 1665 bits per block.
// Refinement scans (Ah > 0; jchuff.c encode_mcu_DC_refine / encode_mcu_AC_refine /
// emit_buffered_bits):
//   DC refinement   1                                  (the bit itself: no symbol, no table)
//   AC refinement   (Se - Ss + 1) * 17 + 14            (a newly nonzero coefficient is a symbol and its sign, any other at
//                                                       most one bit -- a correction bit, or its share of a 0xF0; the run
//                                                       symbol of the piece the block starts, which needs a coefficient
//                                                       that is not newly nonzero: 16 + 14 in place of that one's 16)
#pragma once
#include <stdint.h>
#include <string.h>
#include "qs_encode.h"

#define QP_MAX_SCANS 256           // Ah = 0 sends a coefficient once: at most 4 x 64 scans pass the validation
#define QP_EOB_MAX 0x7FFF          // emit_eobrun is forced when the run reaches this
#define QP_DC_MAXBITS 27
#define QP_AC_MAXBITS(Ss, Se) (((Se) - (Ss) + 1) * 26 + 30)
#define QP_MAXBITS QP_AC_MAXBITS(1, 63)
#define QR_CORR_MAX 937            // MAX_CORR_BITS - DCTSIZE2 + 1: emit_eobrun is forced once more bits than this are buffered
#define QR_TAIL_MAX 63             // correction bits one block adds to the buffer
#define QR_PIECE_MIN (QR_CORR_MAX / QR_TAIL_MAX + 1)   // blocks it takes to pass QR_CORR_MAX: 15
#define QR_DC_MAXBITS 1
#define QR_AC_MAXBITS(Ss, Se) (((Se) - (Ss) + 1) * 17 + 14)
#define QR_HD QS_ENC_HD __attribute__((always_inline))   // the walk over the band keeps the block in registers only inlined
// words the emit kernel stages per workgroup: 256 blocks of QP_MAXBITS and up to 7 pad bits each behind up to 31 bits
#define QP_LDS_WORDS ((31 + QS_ENC_WG * (QP_MAXBITS + 7) + 31) / 32)
#define QP_MID_MAX (6 + 4 + 2 + 2 * 4 + 3 + 1)   // DRI marker and the longest SOS header, rounded up

// one scan of a script: jpeg_scan_info
struct QpScanRec {
  int32_t ncomp, comp[4], Ss, Se, Ah, Al;
};

#define QP_SCRIPT_OK 0
#define QP_SCRIPT_BAD 1            // libjpeg's validate_script refuses it (*scan: where, -1: the script as a whole)
#define QP_SCRIPT_REFINE 2         // valid, but scan *scan has Ah > 0
#define QP_SCRIPT_SEQUENTIAL 3     // valid, but the first scan is 0..63: libjpeg takes the script as sequential multi-scan

// validate_script of jcmaster.c (libjpeg 9) for a frame of ncomp components; *why: a short reason.  The order is
// libjpeg's: the first scan decides between progressive and sequential, then every scan is checked by that mode's rules,
// then what was sent -- so QP_SCRIPT_REFINE and QP_SCRIPT_SEQUENTIAL are given to scripts libjpeg accepts, and only to them
QS_ENC_HD int qp_validate_script(const QpScanRec* s, int nscans, int ncomp, int* scan, const char** why) {
  *scan = -1;
  *why = "";
  if (!s || nscans <= 0) { *why = "no scans"; return QP_SCRIPT_BAD; }
  const bool progressive = s[0].Ss != 0 || s[0].Se != 63;
  int8_t last[4][64];
  memset(last, -1, sizeof last);
  bool sent[4] = {false, false, false, false};
  int refine = -1;
  for (int i = 0; i < nscans; ++i) {
    const QpScanRec& r = s[i];
    *scan = i;
    if (r.ncomp <= 0 || r.ncomp > 4) { *why = "1 .. 4 components in a scan"; return QP_SCRIPT_BAD; }
    for (int c = 0; c < r.ncomp; ++c) {
      if (r.comp[c] < 0 || r.comp[c] >= ncomp) { *why = "a component index out of range"; return QP_SCRIPT_BAD; }
      if (c > 0 && r.comp[c] <= r.comp[c - 1]) { *why = "components out of frame order"; return QP_SCRIPT_BAD; }
    }
    if (!progressive) {
      if (r.Ss != 0 || r.Se != 63 || r.Ah != 0 || r.Al != 0) {
        *why = "a scan of a sequential script that is not 0 .. 63 with Ah = Al = 0";
        return QP_SCRIPT_BAD;
      }
      for (int c = 0; c < r.ncomp; ++c) {
        if (sent[r.comp[c]]) { *why = "a component sent twice in a sequential script"; return QP_SCRIPT_BAD; }
        sent[r.comp[c]] = true;
      }
      continue;
    }
    if (r.Ss < 0 || r.Ss > 63 || r.Se < r.Ss || r.Se > 63 || r.Ah < 0 || r.Ah > 10 || r.Al < 0 || r.Al > 10) {
      *why = "Ss <= Se within 0 .. 63 and Ah, Al within 0 .. 10";
      return QP_SCRIPT_BAD;
    }
    if (r.Ss == 0) {
      if (r.Se != 0) { *why = "DC and AC coefficients in one scan"; return QP_SCRIPT_BAD; }
    } else if (r.ncomp != 1) { *why = "an AC scan carries one component"; return QP_SCRIPT_BAD; }
    for (int c = 0; c < r.ncomp; ++c) {
      int8_t* lb = last[r.comp[c]];
      if (r.Ss != 0 && lb[0] < 0) { *why = "an AC scan before the component's DC scan"; return QP_SCRIPT_BAD; }
      for (int k = r.Ss; k <= r.Se; ++k) {
        if (lb[k] < 0) {
          if (r.Ah != 0) { *why = "a first scan of a coefficient with Ah > 0"; return QP_SCRIPT_BAD; }
        } else if (r.Ah != lb[k] || r.Al != r.Ah - 1) {
          *why = "a coefficient sent again without Ah = the last Al and Al = Ah - 1";
          return QP_SCRIPT_BAD;
        }
        lb[k] = (int8_t)r.Al;
      }
    }
    if (r.Ah > 0 && refine < 0) refine = i;
  }
  *scan = -1;
  for (int c = 0; c < ncomp; ++c)
    if (progressive ? last[c][0] < 0 : !sent[c]) {
      *why = progressive ? "a component without a DC scan" : "a component the sequential script does not send";
      return QP_SCRIPT_BAD;
    }
  if (!progressive) { *scan = 0; *why = "a sequential multi-scan script"; return QP_SCRIPT_SEQUENTIAL; }
  if (refine >= 0) { *scan = refine; *why = "a refinement scan (Ah > 0)"; return QP_SCRIPT_REFINE; }
  // (every scan has Ah = 0 here: each coefficient of each component was sent at most once, so nscans <= QP_MAX_SCANS)
  return QP_SCRIPT_OK;
}

// A frame whose components together exceed 10 blocks per MCU has no scan that carries them all (QS_GEOM_MCU from
// qs_enc_geometry, which has filled in everything but the MCU grid by then), yet libjpeg writes it scan by scan as long
// as no scan of the script interleaves more than 10 blocks: the frame's MCU grid, for qp_scan_geometry to cut from
QS_ENC_HD void qp_complete_frame(int W, int H, int blocks, QsEncGeom* g) {
  int mh = 1, mv = 1;
  for (int c = 0; c < g->ncomp; ++c) {
    if (g->hs[c] > mh) mh = g->hs[c];
    if (g->vs[c] > mv) mv = g->vs[c];
  }
  g->bpm = blocks;
  g->mcus_x = (int32_t)((W + 8LL * mh - 1) / (8LL * mh));
  g->mcus = (int32_t)((long long)g->mcus_x * ((H + 8LL * mv - 1) / (8LL * mv)));   // (at most 8188^2: no overflow)
  g->nblocks = 0;                                    // (no scan runs over the frame itself)
}

// per_scan_setup of jcmaster.c: the geometry of one scan of the script out of the frame's (qs_enc_geometry on all
// components).  A one-component scan runs over width_in_blocks x height_in_blocks; an interleaved one keeps the frame's
// MCU grid with the blocks of its own components.  -> QS_GEOM_OK or QS_GEOM_MCU (*detail: the blocks of an MCU)
QS_ENC_HD int qp_scan_geometry(const QsEncGeom& full, const QpScanRec& r, QsEncGeom* g, int* detail) {
  *g = QsEncGeom();
  g->ncomp = r.ncomp;
  int first = 0;
  for (int i = 0; i < r.ncomp; ++i) {
    const int c = r.comp[i];
    g->nw[i] = full.nw[c];
    g->nh[i] = full.nh[c];
    g->stride[i] = full.stride[c];
    g->slot[i] = full.slot[c];
    g->hs[i] = r.ncomp == 1 ? 1 : full.hs[c];
    g->vs[i] = r.ncomp == 1 ? 1 : full.vs[c];
    g->first[i] = first;
    first += g->hs[i] * g->vs[i];
  }
  if (first > 10) {
    *detail = first;
    return QS_GEOM_MCU;
  }
  g->bpm = first;
  g->mcus_x = r.ncomp == 1 ? g->nw[0] : full.mcus_x;
  g->mcus = r.ncomp == 1 ? g->nw[0] * g->nh[0] : full.mcus;
  g->nblocks = g->mcus * g->bpm;
  return QS_GEOM_OK;
}

// jpeg_natural_order
static constexpr unsigned char QP_ZZ[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

QS_ENC_HD int qp_bitlen(uint32_t t) {                 // bits of t: 0 for 0
#if defined(__HIP_DEVICE_COMPILE__)
  return 32 - __clz((int)t);
#else
  return t ? 32 - __builtin_clz(t) : 0;
#endif
}

// ---- the block coders, on a sink with dc(table, category, bits) and ac(table, symbol, bits, nbits) ----

// encode_mcu_DC_first for one block: diff = (DC >> Al) - (previous DC >> Al), arithmetic shifts
template <class Sink>
QS_ENC_HD uint32_t qp_dc_first(int diff, int tb, Sink& s) {
  uint32_t flags = 0;
  const uint32_t t = (uint32_t)(diff < 0 ? -diff : diff);
  int nb = qp_bitlen(t);
  uint32_t bits = (uint32_t)(diff + (diff >> 31)) & ((1u << nb) - 1u);
  if (nb > 11) {                                   // nbits > MAX_COEF_BITS + 1
    flags |= QS_ENC_F_BADCOEF;
    nb = 11;
    bits &= 2047u;
  }
  s.dc(tb, nb, bits);
  return flags;
}

#define QP_F_WRITES 1u             // the block has a value in the band after the shift: it writes symbols of its own
#define QP_F_ENDZ 2u               // it ends in zeros inside the band: it adds 1 to the EOB run

template <int K>
QS_ENC_HD void qp_flag_steps(const int16_t* v, int Ss, int Se, int Al, uint32_t& f) {
  if constexpr (K < 64) {
    if (K >= Ss && K <= Se) {
      const int c = v[QP_ZZ[K]];
      if (((c < 0 ? -c : c) >> Al) != 0) f = QP_F_WRITES;       // (a value clears ENDZ; zeros behind it set it again)
      else f |= QP_F_ENDZ;
    }
    qp_flag_steps<K + 1>(v, Ss, Se, Al, f);
  }
}
// v: the block in natural order
QS_ENC_HD uint32_t qp_ac_flags(const int16_t* v, int Ss, int Se, int Al) {
  uint32_t f = 0;
  qp_flag_steps<1>(v, Ss, Se, Al, f);
  return f;
}

template <int K, class Sink>
QS_ENC_HD void qp_ac_steps(const int16_t* v, int Ss, int Se, int Al, int tb, int& run, uint32_t& flags, Sink& s) {
  if constexpr (K < 64) {
    if (K >= Ss && K <= Se) {
      const int c = v[QP_ZZ[K]];
      const uint32_t t = (uint32_t)(c < 0 ? -c : c) >> Al;
      if (t == 0) {
        ++run;
      } else {
        while (run > 15) {
          s.ac(tb, 0xF0, 0, 0);
          run -= 16;
        }
        int nb = qp_bitlen(t);
        uint32_t bits = (c < 0 ? ~t : t) & ((1u << nb) - 1u);
        if (nb > 10) {                             // JERR_BAD_DCT_COEF: nbits > MAX_COEF_BITS after the shift
          flags |= QS_ENC_F_BADCOEF;
          nb = 10;
          bits &= 1023u;
        }
        s.ac(tb, (run << 4) | nb, bits, nb);
        run = 0;
      }
    }
    qp_ac_steps<K + 1>(v, Ss, Se, Al, tb, run, flags, s);
  }
}
// encode_mcu_AC_first for one block, without the EOB run: the symbols the block itself writes
template <class Sink>
QS_ENC_HD uint32_t qp_ac_first(const int16_t* v, int Ss, int Se, int Al, int tb, Sink& s) {
  uint32_t flags = 0;
  int run = 0;
  qp_ac_steps<1>(v, Ss, Se, Al, tb, run, flags, s);
  return flags;
}

// emit_eobrun: a run of 1 .. QP_EOB_MAX blocks
template <class Sink>
QS_ENC_HD void qp_eobrun(int run, int tb, Sink& s) {
  const int n = qp_bitlen((uint32_t)run) - 1;
  s.ac(tb, n << 4, (uint32_t)run & ((1u << n) - 1u), n);
}

// ---- refinement scans (Ah > 0); the sink also takes raw(bits, n <= 32): bits without a symbol ----

// correction bits in the order they were buffered: the first one on top
struct QrBits {
  uint64_t v;
  int n;                           // at most QR_TAIL_MAX
};
template <class Sink>
QR_HD void qr_put_bits(Sink& s, const QrBits& b) {
  if (b.n > 32) s.raw((uint32_t)(b.v >> 32), b.n - 32);
  if (b.n > 0) s.raw((uint32_t)b.v, b.n > 32 ? 32 : b.n);
}
struct QrNullSink {
  QS_ENC_HD void ac(int, int, uint32_t, int) {}
  QS_ENC_HD void raw(uint32_t, int) {}
};

// encode_mcu_DC_refine for one block: the bit Al of the DC (arithmetic shift)
template <class Sink>
QR_HD void qr_dc_refine(int dc, int Al, Sink& s) {
  s.raw((uint32_t)(dc >> Al) & 1u, 1);
}

template <int K>
QR_HD void qr_eob_steps(const int16_t* v, int Ss, int Se, int Al, int& eob) {
  if constexpr (K < 64) {
    if (K >= Ss && K <= Se) {
      const int c = v[QP_ZZ[K]];
      if (((c < 0 ? -c : c) >> Al) == 1) eob = K;
    }
    qr_eob_steps<K + 1>(v, Ss, Se, Al, eob);
  }
}
template <int K, class Sink>
QR_HD void qr_ac_steps(const int16_t* v, int Ss, int Se, int Al, int tb, int eob, int& run, QrBits& br, Sink& s) {
  if constexpr (K < 64) {
    if (K >= Ss && K <= Se) {
      const int c = v[QP_ZZ[K]];
      const uint32_t t = (uint32_t)(c < 0 ? -c : c) >> Al;
      if (t == 0) {
        ++run;
      } else {
        for (;;) {
          // 0xF0 per 16 zeros in front of it, but not behind the last new coefficient: those are folded into the EOB run
          const bool zrl = run > 15 && K <= eob;
          if (!zrl && t > 1) {                     // nonzero before this scan: one correction bit, and the run goes on
            br.v = (br.v << 1) | (t & 1u);
            ++br.n;
            break;
          }
          // either symbol takes the correction bits buffered so far behind it
          s.ac(tb, zrl ? 0xF0 : (run << 4) | 1, (zrl || c < 0) ? 0u : 1u, zrl ? 0 : 1);
          qr_put_bits(s, br);
          br.v = 0;
          br.n = 0;
          if (!zrl) {
            run = 0;
            break;
          }
          run -= 16;
        }
      }
    }
    qr_ac_steps<K + 1>(v, Ss, Se, Al, tb, eob, run, br, s);
  }
}
// encode_mcu_AC_refine for one block, without the EOB run: the symbols the block itself writes, and *tail: the correction
// bits it leaves in the buffer.  -> QP_F_WRITES: it has a newly nonzero coefficient (its first symbol is preceded by the
// pending run); QP_F_ENDZ: it adds 1 to the EOB run and *tail to the run's buffered bits (r > 0 || BR > 0)
template <class Sink>
QR_HD uint32_t qr_ac_refine(const int16_t* v, int Ss, int Se, int Al, int tb, Sink& s, QrBits* tail) {
  int eob = 0, run = 0;
  qr_eob_steps<1>(v, Ss, Se, Al, eob);
  QrBits br = {0, 0};
  qr_ac_steps<1>(v, Ss, Se, Al, tb, eob, run, br, s);
  *tail = br;
  return (eob > 0 ? QP_F_WRITES : 0u) | ((run > 0 || br.n > 0) ? QP_F_ENDZ : 0u);
}
// The same block in the form the kernels write: its own symbols, then the symbol of the run piece that STARTS with it
// (piece: its length, 0: none starts here), then its tail.  libjpeg writes a piece's symbol and then the tails of all its
// blocks, behind the symbols of a writing first block: the same bits, and each block's share of them is contiguous
template <class Sink>
QR_HD uint32_t qr_ac_block(const int16_t* v, int Ss, int Se, int Al, int tb, int piece, Sink& s) {
  QrBits tail;
  const uint32_t f = qr_ac_refine(v, Ss, Se, Al, tb, s, &tail);
  if (piece) qp_eobrun(piece, tb, s);
  if (f & QP_F_ENDZ) qr_put_bits(s, tail);
  return f;
}

// The EOB runs of an AC scan, block by block.  A "head" is a block that writes or starts a restart interval; `head` is
// the last one at or before block b, fhead its flags, per the blocks of an interval, next_writes whether block b + 1
// writes.  A run starts at the head (behind it when the head does not end in zeros), takes every block up to the next
// head and is cut every QP_EOB_MAX blocks from its start.  -> the length of the run piece that ends at block b (its
// symbol stands behind the block's own: the place libjpeg writes it, in front of the next symbol, the restart marker
// or the end of the scan), 0 when none does
QS_ENC_HD int qp_eob_after(int b, int head, uint32_t fhead, int per, int nblocks, bool next_writes) {
  const int start = head + (((fhead & QP_F_WRITES) && !(fhead & QP_F_ENDZ)) ? 1 : 0);
  if (b < start) return 0;
  const int pos = b - start + 1, rem = pos % QP_EOB_MAX;
  if (rem == 0) return QP_EOB_MAX;
  const bool last = b + 1 == nblocks || (b + 1) % per == 0 || next_writes;
  return last ? rem : 0;
}

// ---- scan order on plain arrays (the kernels stage the same through LDS: qe_load) ----

struct QpArrays {
  const int16_t* coef[6];
  int32_t nblk[6];
};

// the DC libjpeg sees at block kk of component c in MCU m (jctrans.c compress_output: a dummy block of an edge MCU
// repeats the DC of the block before it)
QS_ENC_HD int qp_dc_at(const QsEncGeom& g, const QpArrays& A, int m, int c, int kk) {
  const int hs = g.hs[c], mx = m % g.mcus_x, my = m / g.mcus_x, slot = g.slot[c];
  for (; kk >= 0; --kk) {
    const int y = kk / hs, x = kk - y * hs;
    const int bx = mx * hs + x, by = my * g.vs[c] + y;
    if (bx < g.nw[c] && by < g.nh[c]) {
      const long long idx = (long long)by * g.stride[c] + bx;
      return idx < A.nblk[slot] ? A.coef[slot][idx * 64] : 0;
    }
  }
  return 0;
}

// scan block b -> its component in the scan (*c), the block (null: a dummy) and the DC before it in scan order
QS_ENC_HD const int16_t* qp_block_at(const QsEncGeom& g, const QpArrays& A, int b, int ri, int* c_out, int* prev_dc) {
  const int m = b / g.bpm, k = b - m * g.bpm;
  int c = 0;
  for (int ci = 1; ci < g.ncomp; ++ci)
    if (k >= g.first[ci]) c = ci;
  const int kk = k - g.first[c], hs = g.hs[c], slot = g.slot[c];
  const int y = kk / hs, x = kk - y * hs;
  const int bx = (m % g.mcus_x) * hs + x, by = (m / g.mcus_x) * g.vs[c] + y;
  const long long idx = (long long)by * g.stride[c] + bx;
  const bool real = bx < g.nw[c] && by < g.nh[c] && idx < A.nblk[slot];
  *c_out = c;
  *prev_dc = 0;
  if (kk > 0) *prev_dc = qp_dc_at(g, A, m, c, kk - 1);
  else if (m > 0 && !(ri && m % ri == 0)) *prev_dc = qp_dc_at(g, A, m - 1, c, hs * g.vs[c] - 1);
  return real ? A.coef[slot] + idx * 64 : nullptr;
}

// ---- the serial restatement (host): one scan, and the file around all of them ----
#if !defined(__HIP_DEVICE_COMPILE__)

struct QpHistSink {
  uint32_t (*h)[257];                              // [4][257]: DC 0, DC 1, AC 0, AC 1
  void dc(int tb, int cat, uint32_t) { ++h[tb][cat]; }
  void ac(int tb, int sym, uint32_t, int) { ++h[2 + tb][sym]; }
  void raw(uint32_t, int) {}
};

// a byte buffer that counts past its capacity and stores below it
struct QpBytes {
  uint8_t* p;
  uint64_t cap, n;
  void put(uint32_t b) {
    if (n < cap) p[n] = (uint8_t)b;
    ++n;
  }
};

struct QpBitSink {
  const uint32_t* dcw;                             // [2][16], [2][256]: (size << 16) | code
  const uint32_t* acw;
  QpBytes* out;
  uint64_t acc = 0;
  int n = 0;
  uint32_t flags = 0;
  void bits(uint32_t e, uint32_t val, int nb) {
    const int sz = (int)(e >> 16);
    if (!sz) flags |= QS_ENC_F_NOCODE;
    acc = (acc << (sz + nb)) | ((uint64_t)(e & 0xffffu) << nb) | val;
    n += sz + nb;
    drain();
  }
  void raw(uint32_t val, int nb) {                 // nb <= 32 bits without a symbol
    acc = (acc << nb) | val;
    n += nb;
    drain();
  }
  void drain() {
    while (n >= 8) {
      n -= 8;
      const uint32_t b = (uint32_t)(acc >> n) & 0xffu;
      out->put(b);
      if (b == 0xff) out->put(0);
    }
  }
  void dc(int tb, int cat, uint32_t b) { bits(dcw[tb * 16 + cat], b, cat); }
  void ac(int tb, int sym, uint32_t b, int nb) { bits(acw[tb * 256 + sym], b, nb); }
  void pad() {                                     // to a byte with one-bits
    if (n > 0) {
      const int k = 8 - n;
      acc = (acc << k) | ((1u << k) - 1u);
      n = 0;
      const uint32_t b = (uint32_t)acc & 0xffu;
      out->put(b);
      if (b == 0xff) out->put(0);
    }
  }
};

// One scan in libjpeg's own order of events: the pending EOB run is written in front of the next symbol, at a restart
// boundary, at QP_EOB_MAX and at the end.  g: the scan's geometry, tbl[i]: the Huffman table of its component i, ri: the
// restart interval in MCUs as DRI carries it (0: none).  marker(k): called between intervals (null: the histogram pass)
template <class Sink, class Boundary>
static inline uint32_t qp_scan_serial(const QsEncGeom& g, const QpArrays& A, const QpScanRec& r, const int32_t* tbl, int ri,
                                      Sink& s, Boundary boundary) {
  uint32_t flags = 0;
  int eobrun = 0;
  // AC refinement: libjpeg's bit_buffer, the tails of the run's blocks in order, and BE, their bits
  QrBits* be = (r.Ah && r.Ss) ? new QrBits[QP_EOB_MAX] : nullptr;
  int be_bits = 0;
  auto flush = [&]() {                               // emit_eobrun
    if (!eobrun) return;
    qp_eobrun(eobrun, tbl[0], s);
    if (be)
      for (int i = 0; i < eobrun; ++i) qr_put_bits(s, be[i]);
    eobrun = 0;
    be_bits = 0;
  };
  const int rim = (ri && ri < g.mcus) ? ri : 0;
  for (int b = 0; b < g.nblocks; ++b) {
    const int m = b / g.bpm;
    if (rim && b > 0 && b % g.bpm == 0 && m % rim == 0) {
      flush();
      boundary(m / rim - 1);
    }
    int c, prev;
    const int16_t* v = qp_block_at(g, A, b, rim, &c, &prev);
    if (r.Ss == 0) {
      const int cur = v ? v[0] : prev;
      if (r.Ah) qr_dc_refine(cur, r.Al, s);
      else flags |= qp_dc_first((cur >> r.Al) - (prev >> r.Al), tbl[c], s);
      continue;
    }
    static const int16_t zero[64] = {0};
    if (!v) v = zero;
    if (r.Ah) {
      QrNullSink none;
      QrBits tail;
      const uint32_t f = qr_ac_refine(v, r.Ss, r.Se, r.Al, tbl[0], none, &tail);
      if (f & QP_F_WRITES) {                         // (its first symbol, 0xF0 or a new coefficient, is preceded by the run)
        flush();
        qr_ac_refine(v, r.Ss, r.Se, r.Al, tbl[0], s, &tail);
      }
      if (f & QP_F_ENDZ) {
        be[eobrun++] = tail;
        be_bits += tail.n;
        if (eobrun == QP_EOB_MAX || be_bits > QR_CORR_MAX) flush();
      }
      continue;
    }
    const uint32_t f = qp_ac_flags(v, r.Ss, r.Se, r.Al);
    if (f & QP_F_WRITES) {
      flush();
      flags |= qp_ac_first(v, r.Ss, r.Se, r.Al, tbl[0], s);
    }
    if (f & QP_F_ENDZ)
      if (++eobrun == QP_EOB_MAX) flush();
  }
  flush();
  delete[] be;
  return flags;
}

#endif  // host

// ---- what the kernels and the host driver share ----

// one (job, scan) pair beside its QsEncJob (workspace, written by prepare)
struct QpScan {
  int32_t Ss, Se, Al;
  int32_t job;                     // the job of the batch it belongs to
  int32_t ntab, tab[4];            // the tables its DHT markers carry, in order: 0 DC 0, 1 DC 1, 2 AC 0, 3 AC 1
  int32_t actb;                    // AC scan: the Huffman table of its component
  uint32_t mid_bytes[2];           // [DRI] SOS of each variant ...
  uint64_t off_mid[2];             // ... in the workspace
  uint64_t off_flags;              // uint8[nwg * 256]: QP_F_* of each block (AC scans)
  uint64_t off_wghead;             // int32[nwg]: the last head among a workgroup's blocks, -1: none
  uint64_t off_wgcarry;            // int32[nwg]: the last head in front of the workgroup
  uint64_t off_eob;                // uint16[nwg * 256]: the run piece that ends at each block
  // refinement scans (Ah > 0).  An AC refinement scan keeps in off_flags QP_F_* | tail bits << 2, in off_wghead the sum
  // of each workgroup's cut weights, in off_wgcarry their exclusive scan, in off_eob the piece that STARTS at each block
  // if one does
  int32_t Ah, pad;
  uint64_t off_w;                  // uint32[nwg * 256]: exclusive scan of the cut weights inside the workgroup
  uint64_t off_jump[2];            // int32[nwg * 256] each: where the piece after the one that starts here starts
  uint64_t off_reach;              // uint8[nwg * 256]: a piece starts here
};
struct QpJob {
  int32_t sj0, nscans;             // its scan jobs
  int32_t two, pad;                // 1: the geometry variant follows d_stop[job]
};

struct QpFramePtrs {
  const uint8_t* head[2];
  uint32_t head_bytes[2];
  uint8_t* out;
  uint64_t cap;
};
// arguments of the kernels that work per job (qp_begin, qp_frame), a chunk of jobs at a time
struct QpJobArgs {
  const QsEncJob* sjobs;           // all scan jobs of the batch (workspace)
  const QpScan* scans;
  const QpJob* jobs;               // the chunk's
  const uint8_t* ws;
  const int32_t* d_stop;           // the caller's, per job, or null
  int32_t* sstop;                  // scratch, per scan job: the job's d_stop
  const uint8_t* tables;           // scratch: qs_hip_huff_tables per scan job
  uint64_t* prefix;                // scratch, per scan job: where its segment starts in the file
  const uint64_t* seglen;          // scratch, per scan job: its stuffed bytes
  const int32_t* sstatus;          // scratch, per scan job
  uint64_t* d_len;
  int32_t* d_status;
  int32_t job0, n;
  QpFramePtrs f[QS_ENC_CHUNK];
};
