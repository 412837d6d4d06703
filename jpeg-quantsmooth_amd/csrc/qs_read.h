// qs_read.h -- the device scan reader (qs_hip_read_device_batch, csrc/qs_kernels_read.hip): what the kernels, the host
// driver (csrc/qs_read_job.cpp) and a plain host build (tests/read_host.cpp) share.  The input is the entropy-coded
// segment of one sequential Huffman scan with restart intervals; the output is what libjpeg 9 leaves in its coefficient
// arrays after jpeg_read_coefficients (jdhuff.c decode_mcu, jdcoefct.c consume_data): DESIGN.md section 14.
//
// The table build (jpeg_make_d_derived_tbl), the bit reader and the decode of one restart interval are functions that
// compile for the device and for the host alike: the CPU suite and a sanitizer run the very code a lane runs.
//
// Bounds, for every function here:
//   * the byte cursor never passes the interval's end (QrBits.end <= the job's end <= QrSrc.n); behind it the reader
//     yields zero bits and the interval ends with status 2;
//   * the block loop's trip count comes from the geometry (MCUs of the interval x blocks of an MCU), never from data;
//   * the coefficient index is checked before every store, the block index against the array's size (QrOut.nblk);
//   * every loop over decoded data has a constant bound (8 bytes per refill, code lengths 9..16, 63 coefficients).
#pragma once
#include <stdint.h>
#include <string.h>

#include "qs_encode.h"             // QsEncGeom: the scan's geometry means here what it means in the coder

#if defined(__HIPCC__) || defined(__HIP__)
#define QS_RD_HD __host__ __device__ inline
#else
#define QS_RD_HD static inline
#endif

#define QS_RD_CHUNK 32             // jobs per launch set (their addresses travel in the kernel arguments, 3.2 KiB)
#define QS_RD_WG 256               // lanes per workgroup of the init and marker kernels
#define QS_RD_MCHUNK 4096          // bytes of the scan per marker workgroup (16 per lane)
#define QS_RD_DWG 64               // lanes (= restart intervals) per workgroup of the decode kernel
#define QS_RD_ZWG_MAX 512          // workgroups a job's arrays get at most in the init kernel (they stride)
// the longest interval a lane decodes: one MCU row of the widest legal JPEG (65 500 pixels, 4:4:4: 24 564 blocks),
// rounded up
#define QS_RD_MAX_INTERVAL_BLOCKS 32768

// d_status values
#define QS_RD_OK 0
#define QS_RD_MARKERS 1            // the number or order of the RSTn markers does not match the restart interval
#define QS_RD_LENGTH 2             // an interval ran out of bytes, or had whole bytes left over
#define QS_RD_CODE 3               // a bit pattern without a code, or a run that passes coefficient 63

// jpeg_natural_order: zigzag position -> natural index
#define QS_RD_ZZ_INIT                                                                                                     \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// One Huffman table as jdhuff.c derives it (d_derived_tbl): an 8-bit look-ahead table, and maxcode / valoffset / huffval
// for the longer codes
struct QrTable {
  int32_t maxcode[18];             // largest code of length l, -1 where the table has none
  int32_t valoff[17];              // huffval index of the first code of length l, minus that code
  uint8_t look_nbits[256];         // length of the code the next 8 bits start with, 0: longer than 8 bits (or none)
  uint8_t look_sym[256];
  uint8_t huffval[256];
  uint8_t pad[4];
};

// One job as the kernels see it (workspace, written by prepare).  No addresses of caller memory.
struct QrJob {
  QsEncGeom g;
  int32_t dc_tbl[4], ac_tbl[4];    // Td / Ta of each component: tab[Td], tab[4 + Ta]
  int32_t ri;                      // MCUs per interval (the whole scan when the file has no restart interval)
  int32_t intervals;
  int32_t nzwg, pad;               // workgroups of this job in its chunk's init launch: qr_zero_wgs of its blocks
  uint64_t max_scan;               // no valid segment of this geometry is longer: the kernels look no further
  uint64_t off_state;              // QrState
  uint64_t off_cnt;                // uint32[chunks]: RSTn markers per QS_RD_MCHUNK bytes
  uint64_t off_off;                // uint32[chunks]: their exclusive scan
  uint64_t off_p;                  // uint64[intervals + 1]: the byte each interval starts at; [intervals]: the end
  QrTable tab[8];                  // DC 0..3, AC 0..3
};

struct QrState {
  unsigned long long end;          // offset of the first terminating marker (the scan's length when it has none)
  uint32_t dead, pad;              // 1: status 1 was set; the decode leaves the job alone
};

struct QrPtrs {
  int16_t* coef[4];
  int32_t nblk[4];                 // blocks in each array: every store is bounded by them
  const uint8_t* scan;
  uint64_t scan_bytes;
};
struct QrArgs {
  const QrJob* jobs;               // the chunk's descriptors (workspace)
  uint8_t* ws;                     // the workspace base the descriptors' offsets refer to
  int32_t* d_status;               // indexed by job0 + i
  int32_t job0, n;
  int32_t zwg0[QS_RD_CHUNK];       // each job's first workgroup in the init launch ...
  int32_t mwg0[QS_RD_CHUNK];       // ... in the marker launches (a function of scan_bytes: known to the run call only) ...
  int32_t dwg0[QS_RD_CHUNK];       // ... and in the decode launch
  QrPtrs p[QS_RD_CHUNK];
};

// ---- bytes ---------------------------------------------------------------------------------------------------------------

struct QrSrc {
  const uint8_t* p;
  uint64_t n;                      // bytes that may be read
};

QS_RD_HD uint32_t qr_byte(const QrSrc& s, uint64_t pos) { return pos < s.n ? s.p[pos] : 0u; }

// FF xx at a position: 0 no marker (data, or a stuffed FF 00), 1 RSTn, 2 anything else -- the segment ends there
QS_RD_HD int qr_marker(uint32_t b0, uint32_t b1) {
  if (b0 != 0xFF || b1 == 0) return 0;
  return (b1 >= 0xD0 && b1 <= 0xD7) ? 1 : 2;
}

// the aligned 8-byte unit of memory that holds scan position pos, first byte lowest; *first: the scan position of that
// byte (negative where the unit starts in front of the scan).  Bytes outside [0, n) read as 0 and are never loaded.
QS_RD_HD uint64_t qr_unit8(const QrSrc& s, uint64_t pos, int64_t* first) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(s.p + pos) & ~(uintptr_t)7;
  const int64_t p0 = (int64_t)pos - (int64_t)(reinterpret_cast<uintptr_t>(s.p + pos) & 7);
  *first = p0;
  uint64_t w = 0;
  if (p0 >= 0 && (uint64_t)p0 + 8 <= s.n) {
    __builtin_memcpy(&w, __builtin_assume_aligned(reinterpret_cast<const void*>(a), 8), 8);
    return w;
  }
  for (int i = 0; i < 8; ++i) {
    const int64_t q = p0 + i;
    if (q >= 0 && (uint64_t)q < s.n) w |= (uint64_t)s.p[q] << (8 * i);
  }
  return w;
}

// the bit reader of one interval: bytes [pos, end) of the scan, the 00 behind each FF dropped
struct QrBits {
  QrSrc s;
  uint64_t pos, end;               // next byte, end of the interval (end <= s.n)
  uint64_t win;                    // the aligned unit the cursor is in ...
  int64_t win0;                    // ... and the scan position of its first byte
  uint64_t buf;                    // the low `left` bits are unread, most significant first
  int left;
  int pad;                         // zero bits appended behind the interval's last byte (they lie at the end of buf)
};

QS_RD_HD void qr_bits_init(QrBits& b, const QrSrc& s, uint64_t start, uint64_t end) {
  b.s = s;
  b.end = end < s.n ? end : s.n;
  b.pos = start < b.end ? start : b.end;
  b.win = 0;
  b.win0 = -64;
  b.buf = 0;
  b.left = 0;
  b.pad = 0;
}

// at least 57 unread bits
QS_RD_HD void qr_fill(QrBits& b) {
  for (int i = 0; i < 8 && b.left <= 56; ++i) {
    uint32_t c = 0;
    if (b.pos < b.end) {
      const int64_t d = (int64_t)b.pos - b.win0;
      if (d < 0 || d >= 8) b.win = qr_unit8(b.s, b.pos, &b.win0);
      c = (uint32_t)(b.win >> (8 * ((int64_t)b.pos - b.win0))) & 0xFF;
      ++b.pos;
      // inside an interval every FF is followed by 00 (anything else is a marker, and markers bound the intervals)
      if (c == 0xFF && b.pos < b.end) ++b.pos;
    } else {
      b.pad += 8;
    }
    b.buf = (b.buf << 8) | c;
    b.left += 8;
  }
}

// the next n bits, 1 <= n <= 16 <= left
QS_RD_HD uint32_t qr_peek(const QrBits& b, int n) { return (uint32_t)(b.buf >> (b.left - n)) & ((1u << n) - 1u); }

// HUFF_EXTEND of jdhuff.c
QS_RD_HD int qr_extend(uint32_t r, int s) { return r <= ((1u << (s - 1)) - 1u) ? (int)r - (int)((1u << s) - 1u) : (int)r; }

// one symbol (jdhuff.c HUFF_DECODE / jpeg_huff_decode); needs 16 unread bits.  -1: the bits start no code
QS_RD_HD int qr_symbol(QrBits& b, const QrTable& t) {
  const uint32_t look = qr_peek(b, 8);
  const int nb = t.look_nbits[look];
  if (nb) {
    b.left -= nb;
    return t.look_sym[look];
  }
  for (int l = 9; l <= 16; ++l) {
    const int32_t code = (int32_t)qr_peek(b, l);
    if (code <= t.maxcode[l]) {
      b.left -= l;
      return t.huffval[(t.valoff[l] + code) & 255];
    }
  }
  return -1;
}

// jpeg_make_d_derived_tbl of jdhuff.c.  0: built; 1: not a valid table (JERR_BAD_HUFF_TABLE)
QS_RD_HD int qr_build_table(const uint8_t* bits, const uint8_t* huffval, int is_dc, QrTable* t) {
  uint32_t codes[256];
  int n = 0;
  for (int l = 1; l <= 16; ++l) n += bits[l];
  if (n > 256) return 1;
  int p = 0;
  uint32_t code = 0;
  for (int l = 1; l <= 16 && p < n; ++l) {
    for (int i = 0; i < bits[l]; ++i) codes[p++] = code++;
    if (code >= (1u << l)) return 1;             // (libjpeg's rule: the all-ones code of a length stays unused)
    code <<= 1;
  }
  memset(t, 0, sizeof *t);
  p = 0;
  for (int l = 1; l <= 16; ++l) {
    if (bits[l]) {
      t->valoff[l] = p - (int32_t)codes[p];
      p += bits[l];
      t->maxcode[l] = (int32_t)codes[p - 1];
    } else {
      t->maxcode[l] = -1;
    }
  }
  t->maxcode[0] = -1;
  t->maxcode[17] = 0xFFFFF;
  p = 0;
  for (int l = 1; l <= 8; ++l)
    for (int i = 0; i < bits[l]; ++i, ++p) {
      const uint32_t first = codes[p] << (8 - l);
      for (uint32_t c = 0; c < (1u << (8 - l)); ++c) {
        t->look_nbits[(first + c) & 255] = (uint8_t)l;
        t->look_sym[(first + c) & 255] = huffval[p];
      }
    }
  for (int i = 0; i < n; ++i) {
    if (is_dc && huffval[i] > 15) return 1;
    t->huffval[i] = huffval[i];
  }
  return 0;
}

// ---- geometry ------------------------------------------------------------------------------------------------------------

// The scan of a frame whose one scan carries all its components (jdinput.c per_scan_setup): the coder's QsEncGeom from
// the coder's own function (qs_encode.h: qs_enc_geometry), slot[c] = c.  stride / rows: the caller's arrays.  0 ok; 1 an
// array holds fewer blocks than libjpeg's width_in_blocks x height_in_blocks, or bad factors; 2 more than 10 blocks in
// an MCU
QS_RD_HD int qr_geometry(int ncomp, int W, int H, const int32_t* hsamp, const int32_t* vsamp, const int32_t* stride,
                         const int32_t* rows, QsEncGeom* g) {
  memset(g, 0, sizeof *g);
  if (ncomp < 1 || ncomp > 4) return 1;
  for (int c = 0; c < ncomp; ++c)
    if (hsamp[c] < 1 || hsamp[c] > 4 || vsamp[c] < 1 || vsamp[c] > 4 || stride[c] < 1 || rows[c] < 1) return 1;
  int detail;
  const int why = qs_enc_geometry(ncomp, W, H, hsamp, vsamp, stride, rows, nullptr, g, &detail);
  return why == QS_GEOM_OK ? 0 : why == QS_GEOM_MCU ? 2 : 1;
}

// the intervals of a scan with DRI value `dri` (0: none): MCUs per interval and their number
QS_RD_HD void qr_intervals(const QsEncGeom& g, int dri, int32_t* ri, int32_t* intervals) {
  *ri = (dri <= 0 || dri >= g.mcus) ? g.mcus : dri;
  *intervals = (g.mcus + *ri - 1) / *ri;
}

// workgroups that zero `blocks` blocks of coefficient arrays: four 16-byte stores a lane, QS_RD_ZWG_MAX at most
QS_RD_HD int qr_zero_wgs(long long blocks) {
  const long long w = (blocks * 8 + QS_RD_WG * 4 - 1) / (QS_RD_WG * 4);
  return (int)(w < 1 ? 1 : w > QS_RD_ZWG_MAX ? QS_RD_ZWG_MAX : w);
}

// no valid segment is longer: every block at its longest code, every byte stuffed, a pad byte that may be stuffed and
// a marker per interval end
QS_RD_HD uint64_t qr_max_scan(const QsEncGeom& g, int intervals) {
  return 2 * (((uint64_t)g.nblocks * QS_ENC_MAXBITS + 7) / 8) + 4 * (uint64_t)intervals;
}

// ---- one interval ----------------------------------------------------------------------------------------------------------

struct QrOut {
  int16_t* coef[4];
  int32_t nblk[4];
};

// MCUs [m0, m1) of the scan from bytes [start, end): what decode_mcu stores, for every block whose position lies inside
// the caller's array (the dummy blocks of edge MCUs included, as libjpeg keeps them in its padded virtual arrays).
// Only non-zero values are stored: the arrays are zero before.  -> QS_RD_OK / QS_RD_LENGTH / QS_RD_CODE
QS_RD_HD int qr_decode_interval(const QsEncGeom& g, const int32_t* dc_tbl, const int32_t* ac_tbl, const QrTable* tab,
                                const QrSrc& src, uint64_t start, uint64_t end, int m0, int m1, const QrOut& out) {
  const uint8_t zz[64] = QS_RD_ZZ_INIT;
  QrBits b;
  qr_bits_init(b, src, start, end);
  int pred[4] = {0, 0, 0, 0};                                      // DC predictions start at 0 in every interval
  int mx = m0 % g.mcus_x, my = m0 / g.mcus_x;
  for (int m = m0; m < m1; ++m) {
    for (int c = 0; c < 4; ++c) {
      if (c >= g.ncomp) break;
      const QrTable& D = tab[dc_tbl[c] & 3];
      const QrTable& A = tab[4 + (ac_tbl[c] & 3)];
      const int hs = g.hs[c], vs = g.vs[c], slot = g.slot[c] & 3, stride = g.stride[c];
      for (int kk = 0; kk < hs * vs; ++kk) {
        const int y = kk / hs, x = kk - y * hs;
        const int bx = mx * hs + x, by = my * vs + y;
        const long long idx = (long long)by * stride + bx;
        int16_t* blk = (bx < stride && idx < out.nblk[slot]) ? out.coef[slot] + idx * 64 : nullptr;
        if (b.left < 32) qr_fill(b);
        int s = qr_symbol(b, D);
        if (s < 0) return QS_RD_CODE;
        s &= 15;
        if (s) {
          const uint32_t r = qr_peek(b, s);
          b.left -= s;
          pred[c] += qr_extend(r, s);
        }
        const int16_t dc = (int16_t)pred[c];                       // the prediction runs as int, JCOEF is a short
        if (blk && dc) blk[0] = dc;
        for (int k = 1; k < 64; ++k) {
          if (b.left < 32) qr_fill(b);
          const int sym = qr_symbol(b, A);
          if (sym < 0) return QS_RD_CODE;
          const int run = sym >> 4;
          s = sym & 15;
          if (s) {
            k += run;
            if (k > 63) return QS_RD_CODE;
            const uint32_t r = qr_peek(b, s);
            b.left -= s;
            if (blk) blk[zz[k]] = (int16_t)qr_extend(r, s);
          } else {
            if (run != 15) break;                                  // EOB
            k += 15;
            if (k > 63) return QS_RD_CODE;
          }
        }
        if (b.left < b.pad) return QS_RD_LENGTH;                   // bits were taken from behind the interval's end
      }
    }
    if (++mx == g.mcus_x) {
      mx = 0;
      ++my;
    }
  }
  // a whole byte or more unread: the interval is longer than its blocks
  if (b.pos < b.end || b.left - b.pad >= 8) return QS_RD_LENGTH;
  return QS_RD_OK;
}

// ---- the whole job, one step after the other (host builds: tests/read_host.cpp) -----------------------------------------
// What the kernels compute, restated serially on top of the same functions: arrays zeroed, the end found, the markers
// counted, checked and placed, every interval decoded, the largest status kept.
QS_RD_HD int qr_read_serial(const QrJob& J, const QrSrc& scan, const QrOut& out) {
  for (int c = 0; c < J.g.ncomp; ++c)
    for (long long i = 0; i < (long long)out.nblk[c] * 64; ++i) out.coef[c][i] = 0;
  QrSrc s = scan;
  if (s.n > J.max_scan) s.n = J.max_scan;
  uint64_t end = s.n;
  for (uint64_t p = 0; p < s.n; ++p)
    if (qr_marker(qr_byte(s, p), qr_byte(s, p + 1)) == 2) {
      end = p;
      break;
    }
  int nmark = 0, status = QS_RD_OK;
  for (uint64_t p = 0; p < end; ++p)                               // RSTn k (1 ..) carries n = (k - 1) & 7
    if (qr_marker(qr_byte(s, p), qr_byte(s, p + 1)) == 1) {
      if (qr_byte(s, p + 1) != 0xD0u + (uint32_t)(nmark & 7)) status = QS_RD_MARKERS;
      ++nmark;
    }
  if (nmark != J.intervals - 1) status = QS_RD_MARKERS;
  if (status) return status;
  QrSrc body = s;
  body.n = end;
  uint64_t start = 0;
  int r = 0;
  for (uint64_t p = 0; p <= end && r < J.intervals; ++p) {
    const bool last = p == end;
    if (!last && qr_marker(qr_byte(s, p), qr_byte(s, p + 1)) != 1) continue;
    const int m0 = r * J.ri, m1 = (m0 + J.ri < J.g.mcus) ? m0 + J.ri : J.g.mcus;
    const int st = qr_decode_interval(J.g, J.dc_tbl, J.ac_tbl, J.tab, body, start, p, m0, m1, out);
    if (st > status) status = st;
    start = p + 2;
    ++r;
  }
  return status;
}
