/*
 * read_split_host.cpp -- the split route of the device scan reader (csrc/qs_read_split.h) compiled for the host, for
 * tests/test_read_split_host.py: qr_split_serial runs the stages of the kernels one after the other on the functions
 * a GPU lane runs.  Also built with -fsanitize=address,undefined, with -DQS_RD_SPLIT_ROUNDS=0 (the verify step must
 * then refuse what did not synchronise) and with a small -DQS_RD_SPLIT_BYTES (many segments in small files).  Every
 * scan and every array lies in a heap block of exactly its size.
 *
 *   read_split_host run in.bin out.bin [rounds]
 *
 * in.bin:  as tests/read_host.cpp reads it.  rounds: synchronisation rounds to run instead of QS_RD_SPLIT_ROUNDS (a
 *          large number measures how many a file needs).
 * out.bin: per case int32 status -- 0..4 as d_status, -1 a table that is no Huffman table, -2 geometry refused -- then
 *          int32 rounds needed until every link held (-1: not within `rounds`, or the markers were refused), int32
 *          segments, and, for status >= 0, the arrays (stride x rows x 64 int16 per component)
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "qs_read_split.h"

static bool get(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

static int run(const char* src, const char* dst, int rounds) {
  FILE *in = fopen(src, "rb"), *out = fopen(dst, "wb");
  int32_t ncases = 0;
  if (!in || !out || !get(in, &ncases, 4) || ncases < 0) {
    fprintf(stderr, "read_split_host: bad input\n");
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
    const size_t shift = (size_t)ci % 16;                                 // `shift` bytes behind a 16-byte boundary
    uint8_t* heap = static_cast<uint8_t*>(malloc(shift + n ? shift + n : 1));
    if (!heap) return 1;
    uint8_t* scan = heap + shift;
    if (n && !get(in, scan, (size_t)n)) return 1;
    if (status == 0 && qr_geometry(h[0], h[1], h[2], hs, vs, stride, rows, &J->g)) status = -2;
    int32_t needed = -1, nseg = 0;
    if (status == 0) {
      qr_intervals(J->g, dri, &J->ri, &J->intervals);
      J->max_scan = qr_max_scan(J->g, J->intervals);
      for (int c = 0; c < 4; ++c) {
        J->dc_tbl[c] = td[c] & 3;
        J->ac_tbl[c] = ta[c] & 3;
      }
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
      // the workspace, sized for the bytes at hand (the driver sizes it for the longest scan of the geometry)
      const uint64_t bytes = n < J->max_scan ? n : J->max_scan;
      const size_t segs = (size_t)qrs_max_segments(bytes, J->intervals);
      std::vector<uint32_t> seg0((size_t)J->intervals + 1), cnt(segs), ns(1);
      std::vector<uint64_t> entry(segs), e0(segs), e1(segs), P((size_t)J->intervals + 1);
      std::vector<int16_t> dcd((size_t)J->g.nblocks);
      QrsBufs B;
      B.nseg = ns.data();
      B.seg0 = seg0.data();
      B.entry = entry.data();
      B.exit[0] = e0.data();
      B.exit[1] = e1.data();
      B.cnt = cnt.data();
      B.dcd = dcd.data();
      status = qr_split_serial(*J, s, o, B, P.data(), rounds, &needed);
      nseg = (int32_t)ns[0];
      fwrite(&status, 4, 1, out);
      fwrite(&needed, 4, 1, out);
      fwrite(&nseg, 4, 1, out);
      for (int c = 0; c < J->g.ncomp; ++c) fwrite(arr[(size_t)c].data(), 2, arr[(size_t)c].size(), out);
    } else {
      fwrite(&status, 4, 1, out);
      fwrite(&needed, 4, 1, out);
      fwrite(&nseg, 4, 1, out);
    }
    free(heap);
    delete J;
  }
  fclose(in);
  return fclose(out) != 0;
}

int main(int argc, char** argv) {
  if ((argc == 4 || argc == 5) && !strcmp(argv[1], "run"))
    return run(argv[2], argv[3], argc == 5 ? atoi(argv[4]) : QS_RD_SPLIT_ROUNDS);
  fprintf(stderr, "usage: read_split_host run in.bin out.bin [rounds]\n");
  return 2;
}
