// qs_read_prog.h -- the progressive route of the device scan reader (qs_hip_read_prog_device_batch,
// csrc/qs_kernels_read_prog.hip): what the kernels, the host driver (csrc/qs_read_prog_job.cpp) and a plain host build
// (tests/read_prog_host.cpp) share.  The input is a whole progressive Huffman file (SOF2, 8 bits); the output is what
// libjpeg 9 leaves in its coefficient arrays after jpeg_read_coefficients (jdhuff.c decode_mcu_DC_first /
// decode_mcu_AC_first / decode_mcu_DC_refine / decode_mcu_AC_refine, jdcoefct.c consume_data): DESIGN.md section 18.
//
// One lane decodes one restart interval of one scan.  A scan depends on every earlier scan of the file that shares a
// component with it and whose band [Ss, Se] overlaps its own; scans without such a relation touch disjoint int16 values.
// qrp_levels gives every scan a level (0: depends on nothing, else 1 + the largest level it depends on) and the run
// makes one decode launch per level.  There is no self-synchronisation inside an interval: an AC refinement scan cannot
// have it (how many bits a symbol consumes depends on which coefficients earlier scans made non-zero).
//
// Everything is built on qs_read.h (QrBits / qr_fill / qr_symbol / qr_build_table), which is included and not changed;
// a (job, scan) pair is described by a QrJob (the scan's own geometry, interval, tables, marker arrays) and a QrpScan.
//
// Bounds, for every function here:
//   * the byte cursor never passes the interval's end (QrBits.end <= the scan's end <= the next scan's prepared offset
//     <= the file's bytes); behind it the reader yields zero bits and the interval ends with status 2;
//   * the block loop's trip count comes from the geometry (MCUs of the interval x blocks of an MCU), never from data: an
//     EOB run is consumed one block per trip of that loop, and a run longer than the blocks left is status 3;
//   * k is checked against Se before every store, the block index against the array's size (QrOut.nblk) and the stride;
//   * every loop over decoded data has a constant bound (8 bytes per refill, code lengths 9..16, Se - Ss + 1 coefficients).
#pragma once
#include "qs_read.h"
// QpScanRec, qp_validate_script, qp_scan_geometry: the script means here what it means in the coder.  (The coder's header
// has a bit buffer named like the reader's; it keeps its name in every translation unit of the coder.)
#define QrBits QpRefineBits
#include "qs_encode_prog.h"
#undef QrBits

#define QRP_MAX_SCANS QP_MAX_SCANS
// no block of a progressive scan codes more bits than this (an AC first scan of 1..63: 63 * 26 + 30)
#define QRP_MAXBITS QP_MAXBITS

// what a (job, scan) pair needs on top of its QrJob
struct QrpScan {
  int32_t job;                     // of the batch
  int32_t ns;                      // components the SOS header names
  int32_t Ss, Se, Ah, Al;
  int32_t level, pad;
  uint64_t offset;                 // of the first byte behind the SOS header, in the file
  uint64_t limit;                  // the next scan's offset (~0 behind the last scan): this scan ends in front of it
};

// one entry of a decode launch: the pair and its first workgroup
struct QrpEntry {
  int32_t pair, wg0;
};

// the arguments of the route's own kernels, per chunk of QS_RD_CHUNK jobs: the jobs' files and arrays (caller memory);
// everything else a lane needs comes from the descriptors prepare wrote into the workspace
struct QrpArgs {
  const QrJob* pairs;              // every pair of the batch, job by job in file order (workspace)
  const QrpScan* scans;
  const QrpEntry* list;            // the entries of this decode launch (workspace), sorted by wg0
  uint8_t* ws;                     // the workspace base the descriptors' offsets refer to
  int32_t* d_status;               // indexed by job0 + i
  int32_t nlist;
  int32_t job0, n;                 // the chunk's jobs
  int32_t pair0, npairs;           // their pairs
  int32_t zwg0[QS_RD_CHUNK + 1];   // each job's first workgroup in the init launch, and the launch's size
  const uint8_t* file[QS_RD_CHUNK];
  uint64_t file_bytes[QS_RD_CHUNK];
  int16_t* coef[QS_RD_CHUNK][4];   // by frame component; null: the job has no such component
  int32_t nblk[QS_RD_CHUNK][4];    // blocks in each array: every store is bounded by them
};

// why qrp_describe refuses a scan
#define QRP_OK 0
#define QRP_MCU 1                  // more than 10 blocks in an MCU of an interleaved scan (*detail: how many)
#define QRP_CAP 2                  // more than QS_RD_MAX_INTERVAL_BLOCKS blocks in an interval (*detail: how many, clamped)
#define QRP_TABLE 3                // Td / Ta outside 0 .. 3 (*detail: the scan component)

// levels: level[i] of each scan; -> the number of levels.  A scan waits for every earlier scan that shares a component
// with it and whose band overlaps its own.  n <= QRP_MAX_SCANS
QS_RD_HD int qrp_levels(const QpScanRec* s, int n, int32_t* level) {
  int levels = 0;
  for (int i = 0; i < n; ++i) {
    int l = 0;
    for (int j = 0; j < i; ++j) {
      if (s[j].Se < s[i].Ss || s[i].Se < s[j].Ss) continue;
      bool shared = false;
      for (int a = 0; a < s[i].ncomp && a < 4; ++a)
        for (int b = 0; b < s[j].ncomp && b < 4; ++b) shared |= s[i].comp[a] == s[j].comp[b];
      if (shared && level[j] + 1 > l) l = level[j] + 1;
    }
    level[i] = l;
    if (l + 1 > levels) levels = l + 1;
  }
  return levels;
}

// the frame's geometry for qp_scan_geometry to cut scans from: qs_enc_geometry on all components; a frame of more than 10
// blocks per MCU is a frame all the same (libjpeg's limit is per scan).  -> QS_GEOM_*
QS_RD_HD int qrp_frame_geometry(int ncomp, int W, int H, const int32_t* hs, const int32_t* vs, const int32_t* stride,
                                const int32_t* rows, QsEncGeom* full, int* detail) {
  if (ncomp < 1 || ncomp > 4) return QS_GEOM_ARGS;
  for (int c = 0; c < ncomp; ++c)
    if (hs[c] < 1 || hs[c] > 4 || vs[c] < 1 || vs[c] > 4 || stride[c] < 1 || rows[c] < 1) return QS_GEOM_ARGS;
  const int why = qs_enc_geometry(ncomp, W, H, hs, vs, stride, rows, nullptr, full, detail);
  if (why == QS_GEOM_MCU) {
    qp_complete_frame(W, H, *detail, full);
    return QS_GEOM_OK;
  }
  return why;
}

// no valid segment of the scan is longer: every block at its longest code, every byte stuffed, a pad byte that may be
// stuffed and a marker per interval end
QS_RD_HD uint64_t qrp_max_scan(const QsEncGeom& g, int intervals) {
  return 2 * (((uint64_t)g.nblocks * QRP_MAXBITS + 7) / 8) + 4 * (uint64_t)intervals + 16;
}

// One scan of the script on the frame `full`: geometry (per_scan_setup: an interleaved scan keeps the frame's MCU grid,
// a one-component scan runs raster over the component's own blocks), intervals counted in the scan's own MCUs, the cap.
// The code tables and the workspace offsets are the caller's.  -> QRP_*
QS_RD_HD int qrp_describe(const QsEncGeom& full, const QpScanRec& r, const int32_t* td, const int32_t* ta, int dri,
                          uint64_t offset, int job, QrJob* J, QrpScan* X, long long* detail) {
  int d = 0;
  if (qp_scan_geometry(full, r, &J->g, &d) != QS_GEOM_OK) {
    *detail = d;
    return QRP_MCU;
  }
  qr_intervals(J->g, dri, &J->ri, &J->intervals);
  const long long per = (long long)J->ri * J->g.bpm;
  *detail = per;
  if (per > QS_RD_MAX_INTERVAL_BLOCKS) return QRP_CAP;
  for (int c = 0; c < r.ncomp; ++c) {
    // a DC scan names no AC table, an AC scan no DC table, a DC refinement none at all: what is not used is not looked at
    const bool need_dc = r.Ss == 0 && r.Ah == 0, need_ac = r.Ss != 0;
    if ((need_dc && (td[c] < 0 || td[c] > 3)) || (need_ac && (ta[c] < 0 || ta[c] > 3))) {
      *detail = c;
      return QRP_TABLE;
    }
    J->dc_tbl[c] = need_dc ? td[c] : 0;
    J->ac_tbl[c] = need_ac ? ta[c] : 0;
  }
  J->max_scan = qrp_max_scan(J->g, J->intervals);
  J->nzwg = 1;
  X->job = job;
  X->ns = r.ncomp;
  X->Ss = r.Ss;
  X->Se = r.Se;
  X->Ah = r.Ah;
  X->Al = r.Al;
  X->offset = offset;
  X->limit = ~(uint64_t)0;
  return QRP_OK;
}

// the SOS header in front of a scan's prepared offset: FF DA, the component count, Ss, Se, Ah / Al.  A file whose scans
// do not start where prepare saw them fails here (status 1), whatever its bytes decode to
QS_RD_HD bool qrp_header_ok(const QrSrc& file, const QrpScan& X) {
  const uint64_t len = 8 + 2 * (uint64_t)X.ns;
  if (X.offset < len || X.offset > file.n) return false;
  const uint64_t p = X.offset - len;
  return qr_byte(file, p) == 0xFF && qr_byte(file, p + 1) == 0xDA && qr_byte(file, p + 4) == (uint32_t)X.ns &&
         qr_byte(file, X.offset - 3) == (uint32_t)X.Ss && qr_byte(file, X.offset - 2) == (uint32_t)X.Se &&
         qr_byte(file, X.offset - 1) == (uint32_t)((X.Ah << 4) | X.Al);
}

// the bytes of the file a scan's kernels look at: from its offset to the next scan's, the file's end or the longest
// segment of the geometry, whichever comes first
QS_RD_HD QrSrc qrp_scan_src(const QrSrc& file, const QrJob& J, const QrpScan& X) {
  QrSrc s;
  uint64_t end = file.n < X.limit ? file.n : X.limit;
  const uint64_t off = X.offset < end ? X.offset : end;
  s.p = file.p + off;
  s.n = end - off;
  if (s.n > J.max_scan) s.n = J.max_scan;
  return s;
}

// ---- one block -----------------------------------------------------------------------------------------------------------
// Each returns QS_RD_OK or QS_RD_CODE; blk is null for a position outside the caller's array (nothing is stored, the
// bits are consumed all the same).  `left`: the blocks of the interval from this one on.

// decode_mcu_DC_first
QS_RD_HD int qrp_dc_first(QrBits& b, const QrTable& D, int Al, int* pred, int16_t* blk) {
  if (b.left < 32) qr_fill(b);
  int s = qr_symbol(b, D);
  if (s < 0) return QS_RD_CODE;
  s &= 15;
  if (s) {
    const uint32_t r = qr_peek(b, s);
    b.left -= s;
    *pred += qr_extend(r, s);
  }
  const int16_t dc = (int16_t)((uint32_t)*pred << Al);               // the prediction runs as int, JCOEF is a short
  if (blk && dc) blk[0] = dc;
  return QS_RD_OK;
}

// decode_mcu_DC_refine
QS_RD_HD void qrp_dc_refine(QrBits& b, int Al, int16_t* blk) {
  if (b.left < 32) qr_fill(b);
  const uint32_t bit = qr_peek(b, 1);
  b.left -= 1;
  if (bit && blk) blk[0] = (int16_t)(blk[0] | (1 << Al));
}

// decode_mcu_AC_first
QS_RD_HD int qrp_ac_first(QrBits& b, const QrTable& A, const uint8_t* zz, int Ss, int Se, int Al, uint32_t* eobrun,
                          int left, int16_t* blk) {
  if (*eobrun > 0) {
    --*eobrun;
    return QS_RD_OK;
  }
  for (int k = Ss; k <= Se; ++k) {
    if (b.left < 32) qr_fill(b);
    const int sym = qr_symbol(b, A);
    if (sym < 0) return QS_RD_CODE;
    const int r = sym >> 4, s = sym & 15;
    if (s) {
      k += r;
      if (k > Se) return QS_RD_CODE;
      const uint32_t v = qr_peek(b, s);
      b.left -= s;
      if (blk) blk[zz[k]] = (int16_t)((uint32_t)qr_extend(v, s) << Al);
    } else if (r != 15) {
      uint32_t run = 1u << r;
      if (r) {
        run += qr_peek(b, r);
        b.left -= r;
      }
      if (run > (uint32_t)left) return QS_RD_CODE;
      *eobrun = run - 1;                                             // this block is done
      break;
    } else {
      k += 15;
      if (k > Se) return QS_RD_CODE;
    }
  }
  return QS_RD_OK;
}

// one correction bit for an already non-zero coefficient: applied only if its bit Al is still clear, away from zero
QS_RD_HD void qrp_correct(QrBits& b, int p1, int16_t* c) {
  if (b.left < 32) qr_fill(b);
  const uint32_t bit = qr_peek(b, 1);
  b.left -= 1;
  if (bit && (*c & p1) == 0) *c = (int16_t)(*c >= 0 ? *c + p1 : *c - p1);   // (the guard: no accepted script gets here with the bit set -- a coefficient is refined only at Ah = its last Al, Al = Ah - 1, so every non-zero value is a multiple of 2 * p1)
}

// decode_mcu_AC_refine
QS_RD_HD int qrp_ac_refine(QrBits& b, const QrTable& A, const uint8_t* zz, int Ss, int Se, int Al, uint32_t* eobrun,
                           int left, int16_t* blk) {
  const int p1 = 1 << Al;
  int k = Ss;                                                        // (a block outside the array reads as zeros)
  if (*eobrun == 0) {
    while (k <= Se) {
      if (b.left < 32) qr_fill(b);
      const int sym = qr_symbol(b, A);
      if (sym < 0) return QS_RD_CODE;
      int r = sym >> 4, s = sym & 15;
      int val = 0;
      if (s) {
        if (s != 1) return QS_RD_CODE;
        val = qr_peek(b, 1) ? p1 : -p1;
        b.left -= 1;
      } else if (r != 15) {
        uint32_t run = 1u << r;
        if (r) {
          run += qr_peek(b, r);
          b.left -= r;
        }
        if (run > (uint32_t)left) return QS_RD_CODE;
        *eobrun = run;
        break;
      }
      // over already non-zero coefficients (a correction bit each) and r still-zero ones
      for (; k <= Se; ++k) {
        if (blk && blk[zz[k]]) qrp_correct(b, p1, blk + zz[k]);
        else if (--r < 0) break;
      }
      if (k > Se) return QS_RD_CODE;                                 // the run passes Se
      if (val && blk) blk[zz[k]] = (int16_t)val;
      ++k;
    }
  }
  if (*eobrun > 0) {
    for (; k <= Se; ++k)
      if (blk && blk[zz[k]]) qrp_correct(b, p1, blk + zz[k]);
    --*eobrun;
  }
  return QS_RD_OK;
}

// ---- one interval ----------------------------------------------------------------------------------------------------------
// MCUs [m0, m1) of the scan from bytes [start, end) of src (the scan's bytes).  dct: the DC tables by Td, act: the scan's
// AC table; coef / nblks: the job's arrays by frame component and their sizes in blocks.  First scans store non-zero values only (the arrays are zero before); a refinement rewrites its own band of
// its own blocks.  The dummy blocks of edge MCUs are written by interleaved scans where the array has room for them and
// do not exist in a one-component scan.  -> QS_RD_OK / QS_RD_LENGTH / QS_RD_CODE
QS_RD_HD int qrp_decode_interval(const QsEncGeom& g, const QrpScan& X, const int32_t* dc_tbl, const QrTable* dct,
                                 const QrTable* act, const QrSrc& src, uint64_t start, uint64_t end, int m0, int m1,
                                 int16_t* const* coef, const int32_t* nblks) {
  const uint8_t zz[64] = QS_RD_ZZ_INIT;
  QrBits b;
  qr_bits_init(b, src, start, end);
  int pred[4] = {0, 0, 0, 0};                                      // DC predictions and the EOB run start at 0 in every interval
  uint32_t eobrun = 0;
  const int Ss = X.Ss & 63, Se = X.Se & 63, Al = X.Al & 15;
  int left = (m1 - m0) * g.bpm;
  int mx = m0 % g.mcus_x, my = m0 / g.mcus_x;
  for (int m = m0; m < m1; ++m) {
    for (int c = 0; c < 4; ++c) {
      if (c >= g.ncomp) break;
      const int hs = g.hs[c], vs = g.vs[c], slot = g.slot[c] & 3, stride = g.stride[c];
      for (int kk = 0; kk < hs * vs; ++kk) {
        const int y = kk / hs, x = kk - y * hs;
        const int bx = mx * hs + x, by = my * vs + y;
        const long long idx = (long long)by * stride + bx;
        int16_t* arr = coef[slot];                                   // (null: the job has no such component)
        int16_t* blk = (arr && bx < stride && idx < nblks[slot]) ? arr + idx * 64 : nullptr;
        int st = QS_RD_OK;
        if (Ss == 0) {
          if (X.Ah == 0) st = qrp_dc_first(b, dct[dc_tbl[c] & 3], Al, &pred[c], blk);
          else qrp_dc_refine(b, Al, blk);
        } else if (X.Ah == 0) {
          st = qrp_ac_first(b, *act, zz, Ss, Se, Al, &eobrun, left, blk);
        } else {
          st = qrp_ac_refine(b, *act, zz, Ss, Se, Al, &eobrun, left, blk);
        }
        if (st) return st;
        if (b.left < b.pad) return QS_RD_LENGTH;                   // bits were taken from behind the interval's end
        --left;
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

// ---- the whole job, one step after the other (host builds: tests/read_prog_host.cpp) ---------------------------------------
// What the kernels compute, restated serially on top of the same functions: arrays zeroed; per scan the header check, the
// end found (a scan no marker ends: status 2, libjpeg's premature end of file), the markers counted and checked (status
// 1 ends the job); then every scan in file order -- an order the
// levels allow -- interval by interval, the largest status kept.  J / X: the file's pairs in file order.
QS_RD_HD int qrp_read_serial(const QrJob* J, const QrpScan* X, int nscans, int ncomp, const QrSrc& file, const QrOut& out) {
  for (int c = 0; c < ncomp; ++c)
    for (long long i = 0; i < (long long)out.nblk[c] * 64; ++i) out.coef[c][i] = 0;
  int status = QS_RD_OK;
  bool cut = false;
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = 0; i < nscans; ++i) {
      const QrSrc s = qrp_scan_src(file, J[i], X[i]);
      uint64_t end = s.n;
      for (uint64_t p = 0; p < s.n; ++p)
        if (qr_marker(qr_byte(s, p), qr_byte(s, p + 1)) == 2) {
          end = p;
          break;
        }
      if (pass == 0) {
        int nmark = 0;
        if (!qrp_header_ok(file, X[i])) status = QS_RD_MARKERS;
        if (end >= s.n) cut = true;                                    // no marker ends the scan: the file stops inside it
        for (uint64_t p = 0; p < end; ++p)                           // RSTn k (1 ..) carries n = (k - 1) & 7
          if (qr_marker(qr_byte(s, p), qr_byte(s, p + 1)) == 1) {
            if (qr_byte(s, p + 1) != 0xD0u + (uint32_t)(nmark & 7)) status = QS_RD_MARKERS;
            ++nmark;
          }
        if (nmark != J[i].intervals - 1) status = QS_RD_MARKERS;
        continue;
      }
      QrSrc body = s;
      body.n = end;
      uint64_t start = 0;
      int r = 0;
      for (uint64_t p = 0; p <= end && r < J[i].intervals; ++p) {
        const bool last = p == end;
        if (!last && qr_marker(qr_byte(s, p), qr_byte(s, p + 1)) != 1) continue;
        const int m0 = r * J[i].ri, m1 = (m0 + J[i].ri < J[i].g.mcus) ? m0 + J[i].ri : J[i].g.mcus;
        const int st = qrp_decode_interval(J[i].g, X[i], J[i].dc_tbl, J[i].tab, J[i].tab + 4 + (J[i].ac_tbl[0] & 3), body,
                                           start, p, m0, m1, out.coef, out.nblk);
        if (st > status) status = st;
        start = p + 2;
        ++r;
      }
    }
    if (pass == 0 && status) return status;                          // the markers of some scan do not fit
  }
  return (cut && status < QS_RD_LENGTH) ? QS_RD_LENGTH : status;
}
