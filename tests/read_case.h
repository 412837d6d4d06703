/*
 * read_case.h -- the case file of the sequential scan reader hosts (tests/read_host.cpp, tests/read_split_host.cpp;
 * written by tests/read_oracle.py's pack_case) and what their sanitized runs rest on:
 *
 *   - every scan lies in a heap block of exactly its length, `case index % 16` bytes behind a 16-byte boundary, so a
 *     read in front of or behind it is reported;
 *   - every array is exactly stride * rows * 64 values, filled with 0x5a5a: no slack, and an unwritten value shows.
 *
 * in.bin:  int32 ncases, then per case
 *            int32 ncomp, width, height, hsamp[4], vsamp[4], stride[4] (blocks per array row), rows[4], Td[4], Ta[4], DRI
 *            8 tables (DC 0..3, AC 0..3): uint8 present, bits[17], huffval[256]
 *            uint64 scan_bytes, the bytes behind the SOS header
 * out.bin: per case the host's int32 words, the status first -- -1 a table that is no Huffman table, -2 geometry
 *          refused, the rest the host's own -- and, for status >= 0, the arrays (stride x rows x 64 int16 per component)
 *
 * tests/read_prog_host.cpp has a layout of its own and shares get() and rc_table().
 */
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "qs_read.h"

static const size_t RC_TABLE_REC = 1 + 17 + 256;

static inline bool get(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

// a table record into `tab` -> non-zero where it is present and no Huffman table; t: 0..3 DC, 4..7 AC
static inline int rc_table(const uint8_t* rec, int t, QrTable* tab) { return rec[0] && qr_build_table(rec + 1, rec + 18, t < 4, tab); }

struct RcFile {
  FILE *in = nullptr, *out = nullptr;
  int32_t ncases = 0;
};

static inline bool rc_open(RcFile& f, const char* who, const char* src, const char* dst) {
  f.in = fopen(src, "rb");
  f.out = fopen(dst, "wb");
  if (f.in && f.out && get(f.in, &f.ncases, 4) && f.ncases >= 0) return true;
  fprintf(stderr, "%s: bad input\n", who);
  return false;
}

static inline int rc_close(RcFile& f) {
  fclose(f.in);
  return fclose(f.out) != 0;
}

struct RcCase {
  std::unique_ptr<QrJob> J{new QrJob()};
  int32_t status = 0;              // 0, or why the case never reaches the reader: -1, -2
  uint8_t* heap = nullptr;
  QrSrc src;                       // the scan
  int32_t stride[4], rows[4];
  std::vector<std::vector<int16_t>> arr;
  QrOut out;                       // over arr, once rc_arrays has made them
  ~RcCase() { free(heap); }
};

// case `ci` of the file: its tables, its scan and -- status 0 -- the job's descriptor; false: the file is short
static inline bool rc_next(RcFile& f, int ci, RcCase& c) {
  int32_t h[3 + 6 * 4 + 1];
  if (!get(f.in, h, sizeof h)) return false;
  const int32_t *hs = h + 3, *vs = h + 7, *td = h + 19, *ta = h + 23;
  memcpy(c.stride, h + 11, sizeof c.stride);
  memcpy(c.rows, h + 15, sizeof c.rows);
  QrJob& J = *c.J;
  memset(&J, 0, sizeof J);
  for (int t = 0; t < 8; ++t) {
    uint8_t rec[RC_TABLE_REC];
    if (!get(f.in, rec, sizeof rec)) return false;
    if (rc_table(rec, t, &J.tab[t])) c.status = -1;
  }
  uint64_t n = 0;
  if (!get(f.in, &n, 8) || n > (1u << 30)) return false;
  const size_t shift = (size_t)ci % 16;
  c.heap = static_cast<uint8_t*>(malloc(shift + n ? shift + n : 1));   // (malloc aligns to 16 bytes)
  if (!c.heap) return false;
  c.src.p = c.heap + shift;
  c.src.n = n;
  if (n && !get(f.in, c.heap + shift, (size_t)n)) return false;
  if (c.status == 0 && qr_geometry(h[0], h[1], h[2], hs, vs, c.stride, c.rows, &J.g)) c.status = -2;
  if (c.status == 0) {
    qr_intervals(J.g, h[27], &J.ri, &J.intervals);
    J.max_scan = qr_max_scan(J.g, J.intervals);
    for (int k = 0; k < 4; ++k) {
      J.dc_tbl[k] = td[k] & 3;
      J.ac_tbl[k] = ta[k] & 3;
    }
  }
  return true;
}

static inline void rc_arrays(RcCase& c) {
  memset(&c.out, 0, sizeof c.out);
  c.arr.resize((size_t)c.J->g.ncomp);
  for (int k = 0; k < c.J->g.ncomp; ++k) {
    c.arr[(size_t)k].assign((size_t)c.stride[k] * c.rows[k] * 64, (int16_t)0x5a5a);
    c.out.coef[k] = c.arr[(size_t)k].data();
    c.out.nblk[k] = c.stride[k] * c.rows[k];
  }
}

// the case's result: `n` words, words[0] the status, and the arrays where it is >= 0
static inline void rc_write(RcFile& f, const RcCase& c, const int32_t* words, int n) {
  fwrite(words, 4, (size_t)n, f.out);
  if (words[0] >= 0)
    for (const auto& a : c.arr) fwrite(a.data(), 2, a.size(), f.out);
}
