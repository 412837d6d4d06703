/*
 * read_host.cpp -- the device scan reader's decode (csrc/qs_read.h) compiled for the host, for tests/test_read_host.py:
 * the same table build, bit reader and interval decode a GPU lane runs, on cases read from a file.  Also built with
 * -fsanitize=address,undefined and run on a corrupt corpus: every scan lies in a heap block of exactly its size, at a
 * varying offset from 16-byte alignment, so a read in front of or behind it is reported.
 *
 *   read_host run in.bin out.bin
 *
 * in.bin, and what the exact-sized blocks are for: tests/read_case.h.
 * out.bin: per case int32 status -- 0..3 as d_status, -1 a table that is no Huffman table, -2 geometry refused, -3 over
 *          the interval cap -- and, for status >= 0, the arrays (stride x rows x 64 int16 per component)
 */
#include "read_case.h"

static int run(const char* src, const char* dst) {
  RcFile f;
  if (!rc_open(f, "read_host", src, dst)) return 1;
  for (int ci = 0; ci < f.ncases; ++ci) {
    RcCase c;
    if (!rc_next(f, ci, c)) return 1;
    if (c.status == 0 && (long long)c.J->ri * c.J->g.bpm > QS_RD_MAX_INTERVAL_BLOCKS) c.status = -3;
    if (c.status == 0) {
      rc_arrays(c);
      c.status = qr_read_serial(*c.J, c.src, c.out);
    }
    rc_write(f, c, &c.status, 1);
  }
  return rc_close(f);
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  fprintf(stderr, "usage: read_host run in.bin out.bin\n");
  return 2;
}
