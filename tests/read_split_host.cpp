/*
 * read_split_host.cpp -- the split route of the device scan reader (csrc/qs_read_split.h) compiled for the host, for
 * tests/test_read_split_host.py: qr_split_serial runs the stages of the kernels one after the other on the functions
 * a GPU lane runs.  Also built with -fsanitize=address,undefined, with -DQS_RD_SPLIT_ROUNDS=0 (the verify step must
 * then refuse what did not synchronise) and with a small -DQS_RD_SPLIT_BYTES (many segments in small files).  Every
 * scan and every array lies in a heap block of exactly its size.
 *
 *   read_split_host run in.bin out.bin [rounds]
 *
 * in.bin:  tests/read_case.h.  rounds: synchronisation rounds to run instead of QS_RD_SPLIT_ROUNDS (a
 *          large number measures how many a file needs).
 * out.bin: per case int32 status -- 0..4 as d_status, -1 a table that is no Huffman table, -2 geometry refused -- then
 *          int32 rounds needed until every link held (-1: not within `rounds`, or the markers were refused), int32
 *          segments, and, for status >= 0, the arrays (stride x rows x 64 int16 per component)
 */
#include "qs_read_split.h"
#include "read_case.h"

static int run(const char* src, const char* dst, int rounds) {
  RcFile f;
  if (!rc_open(f, "read_split_host", src, dst)) return 1;
  for (int ci = 0; ci < f.ncases; ++ci) {
    RcCase c;
    if (!rc_next(f, ci, c)) return 1;
    int32_t words[3] = {c.status, -1, 0};                                 // status, rounds needed, segments
    if (c.status == 0) {
      rc_arrays(c);
      const QrJob& J = *c.J;
      // the workspace, sized for the bytes at hand (the driver sizes it for the longest scan of the geometry)
      const uint64_t bytes = c.src.n < J.max_scan ? c.src.n : J.max_scan;
      const size_t segs = (size_t)qrs_max_segments(bytes, J.intervals);
      std::vector<uint32_t> seg0((size_t)J.intervals + 1), cnt(segs), ns(1);
      std::vector<uint64_t> entry(segs), e0(segs), e1(segs), P((size_t)J.intervals + 1);
      std::vector<int16_t> dcd((size_t)J.g.nblocks);
      QrsBufs B;
      B.nseg = ns.data();
      B.seg0 = seg0.data();
      B.entry = entry.data();
      B.exit[0] = e0.data();
      B.exit[1] = e1.data();
      B.cnt = cnt.data();
      B.dcd = dcd.data();
      words[0] = qr_split_serial(*c.J, c.src, c.out, B, P.data(), rounds, &words[1]);
      words[2] = (int32_t)ns[0];
    }
    rc_write(f, c, words, 3);
  }
  return rc_close(f);
}

int main(int argc, char** argv) {
  if ((argc == 4 || argc == 5) && !strcmp(argv[1], "run"))
    return run(argv[2], argv[3], argc == 5 ? atoi(argv[4]) : QS_RD_SPLIT_ROUNDS);
  fprintf(stderr, "usage: read_split_host run in.bin out.bin [rounds]\n");
  return 2;
}
