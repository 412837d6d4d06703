/*
 * read_host.cpp -- the device scan reader's decode (csrc/qs_read.h) compiled for the host, for tests/test_read_host.py:
 * the same table build, bit reader and interval decode a GPU lane runs, on cases read from a file.  Also built with
 * -fsanitize=address,undefined and run on a corrupt corpus: every scan lies in a heap block of exactly its size, at a
 * varying offset from 16-byte alignment, so a read in front of or behind it is reported.
 *
 *   read_host run in.bin out.bin
 *
 * in.bin:  int32 ncases, then per case
 *            int32 ncomp, width, height, hsamp[4], vsamp[4], stride[4] (blocks per array row), rows[4], Td[4], Ta[4], DRI
 *            8 tables (DC 0..3, AC 0..3): uint8 present, bits[17], huffval[256]
 *            uint64 scan_bytes, the bytes behind the SOS header
 * out.bin: per case int32 status -- 0..3 as d_status, -1 a table that is no Huffman table, -2 geometry refused, -3 over
 *          the interval cap -- and, for status >= 0, the arrays (stride x rows x 64 int16 per component)
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "qs_read.h"

static bool get(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

static int run(const char* src, const char* dst) {
  FILE *in = fopen(src, "rb"), *out = fopen(dst, "wb");
  int32_t ncases = 0;
  if (!in || !out || !get(in, &ncases, 4) || ncases < 0) {
    fprintf(stderr, "read_host: bad input\n");
    return 1;
  }
  for (int ci = 0; ci < ncases; ++ci) {
    int32_t h[3 + 6 * 4 + 1];
    if (!get(in, h, sizeof h)) return 1;
    const int32_t *hs = h + 3, *vs = h + 7, *stride = h + 11, *rows = h + 15, *td = h + 19, *ta = h + 23;
    const int32_t dri = h[27];
    QrJob* J = new QrJob();
    memset(J, 0, sizeof *J);
    int32_t status = 0;
    for (int t = 0; t < 8; ++t) {
      uint8_t rec[1 + 17 + 256];
      if (!get(in, rec, sizeof rec)) return 1;
      if (rec[0] && qr_build_table(rec + 1, rec + 18, t < 4, &J->tab[t])) status = -1;
    }
    uint64_t n = 0;
    if (!get(in, &n, 8) || n > (1u << 30)) return 1;
    // exactly n bytes, `shift` bytes behind a 16-byte boundary
    const size_t shift = (size_t)ci % 16;
    uint8_t* heap = static_cast<uint8_t*>(malloc(shift + n ? shift + n : 1));   // (malloc aligns to 16 bytes)
    if (!heap) return 1;
    uint8_t* scan = heap + shift;
    if (n && !get(in, scan, (size_t)n)) return 1;
    if (status == 0) {
      const int rc = qr_geometry(h[0], h[1], h[2], hs, vs, stride, rows, &J->g);
      if (rc) status = -2;
    }
    if (status == 0) {
      qr_intervals(J->g, dri, &J->ri, &J->intervals);
      if ((long long)J->ri * J->g.bpm > QS_RD_MAX_INTERVAL_BLOCKS) status = -3;
      J->max_scan = qr_max_scan(J->g, J->intervals);
      for (int c = 0; c < 4; ++c) {
        J->dc_tbl[c] = td[c] & 3;
        J->ac_tbl[c] = ta[c] & 3;
      }
    }
    if (status == 0) {
      std::vector<std::vector<int16_t>> arr((size_t)J->g.ncomp);
      QrOut o;
      memset(&o, 0, sizeof o);
      for (int c = 0; c < J->g.ncomp; ++c) {
        arr[(size_t)c].assign((size_t)stride[c] * rows[c] * 64, (int16_t)0x5a5a);   // exactly the array: no slack
        o.coef[c] = arr[(size_t)c].data();
        o.nblk[c] = stride[c] * rows[c];
      }
      QrSrc s;
      s.p = scan;
      s.n = n;
      status = qr_read_serial(*J, s, o);
      fwrite(&status, 4, 1, out);
      for (int c = 0; c < J->g.ncomp; ++c) fwrite(arr[(size_t)c].data(), 2, arr[(size_t)c].size(), out);
    } else {
      fwrite(&status, 4, 1, out);
    }
    free(heap);
    delete J;
  }
  fclose(in);
  return fclose(out) != 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  fprintf(stderr, "usage: read_host run in.bin out.bin\n");
  return 2;
}
