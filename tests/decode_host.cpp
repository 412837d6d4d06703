/*
 * decode_host.cpp -- the device decode's arithmetic (csrc/qs_decode.h) compiled for the host, for
 * tests/test_decode_cases.py: the same qd_idct_block and qd_ycc_rgb the kernel runs, fed from files.
 *
 *   decode_host info                    key=value lines: the header's constants, the L1 norms of the pass-1 matrices,
 *                                       and where a job's tile fields lie in its workspace record
 *   decode_host block KIND in.bin out.bin   qd_idct_block on blocks; KIND islow, 16x16, 16x8, 8x16, or 32x8
 *                                       (16x8 with 2x replication); files as `libjpeg9_decode block` takes them:
 *                                       int32 n, then n records of int16 coef[64] + uint16 table[64]; out: n blocks
 *                                       of rows x cols samples
 *   decode_host ycc in.bin out.bin      qd_ycc_rgb on byte triples (Y, Cb, Cr) -> byte triples (R, G, B)
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "qs_decode.h"

// the largest row L1 norm of a pass-1 matrix: unit vectors through the 64-bit kernel give its columns
template <int R> static long long l1_norm() {
  long long m[16][8];
  for (int k = 0; k < 8; ++k) {
    int64_t in[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[16];
    in[k] = 1;
    if (R == 16) qd_idct16<int64_t>(in, 0, o); else qd_idct8<int64_t>(in, 0, o);
    for (int i = 0; i < R; ++i) m[i][k] = (long long)o[i];
  }
  long long best = 0;
  for (int i = 0; i < R; ++i) {
    long long s = 0;
    for (int k = 0; k < 8; ++k) s += m[i][k] < 0 ? -m[i][k] : m[i][k];
    if (s > best) best = s;
  }
  return best;
}

static int do_info() {
  printf("fast_bound=%lld\n", (long long)QS_DEC_FAST_BOUND);
  printf("chunk=%d\ntile_w=%d\ntile_h=%d\n", QS_DEC_CHUNK, QS_DEC_TW, QS_DEC_TH);
  printf("l1_8=%lld\nl1_16=%lld\n", l1_norm<8>(), l1_norm<16>());
  printf("job_size=%zu\njob_tile0=%zu\njob_tiles=%zu\njob_tiles_x=%zu\n", sizeof(QsDecJob), offsetof(QsDecJob, tile0),
         offsetof(QsDecJob, tiles), offsetof(QsDecJob, tiles_x));
  return 0;
}

static int do_block(const char* kind, const char* src, const char* dst) {
  int rows = 8, cols = 8, which;
  if (!strcmp(kind, "islow")) which = 0;
  else if (!strcmp(kind, "16x16")) { which = 1; rows = cols = 16; }
  else if (!strcmp(kind, "16x8")) { which = 2; cols = 16; }
  else if (!strcmp(kind, "8x16")) { which = 3; rows = 16; }
  else if (!strcmp(kind, "32x8")) { which = 4; cols = 32; }
  else { fprintf(stderr, "decode_host: unknown kind %s\n", kind); return 1; }
  FILE *in = fopen(src, "rb"), *out = fopen(dst, "wb");
  int32_t n;
  if (!in || !out || fread(&n, sizeof n, 1, in) != 1 || n < 0) { fprintf(stderr, "decode_host: bad input\n"); return 1; }
  std::vector<uint8_t> px((size_t)rows * cols);
  for (int b = 0; b < n; ++b) {
    int16_t coef[64];
    uint16_t q[64];
    int32_t dq[64];
    if (fread(coef, sizeof coef, 1, in) != 1 || fread(q, sizeof q, 1, in) != 1) {
      fprintf(stderr, "decode_host: short input\n");
      return 1;
    }
    qd_dequant(coef, q, dq);
    switch (which) {
      case 0: qd_idct_block<false, false>(dq, px.data(), cols); break;
      case 1: qd_idct_block<true, true>(dq, px.data(), cols); break;
      case 2: qd_idct_block<true, false>(dq, px.data(), cols); break;
      case 3: qd_idct_block<false, true>(dq, px.data(), cols); break;
      default: qd_idct_block<true, false, 2>(dq, px.data(), cols); break;
    }
    fwrite(px.data(), 1, px.size(), out);
  }
  fclose(in);
  return fclose(out) != 0;
}

static int do_ycc(const char* src, const char* dst) {
  FILE *in = fopen(src, "rb"), *out = fopen(dst, "wb");
  if (!in || !out) return 1;
  uint8_t t[3 * 4096], o[3 * 4096];
  size_t got;
  while ((got = fread(t, 3, 4096, in)) > 0) {
    for (size_t i = 0; i < got; ++i) qd_ycc_rgb(t[3 * i], t[3 * i + 1], t[3 * i + 2], o + 3 * i);
    fwrite(o, 3, got, out);
  }
  fclose(in);
  return fclose(out) != 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "info")) return do_info();
  if (argc == 5 && !strcmp(argv[1], "block")) return do_block(argv[2], argv[3], argv[4]);
  if (argc == 4 && !strcmp(argv[1], "ycc")) return do_ycc(argv[2], argv[3]);
  fprintf(stderr, "usage: decode_host info | block KIND in.bin out.bin | ycc in.bin out.bin\n");
  return 2;
}
