/*
 * compress_host.cpp -- the device compress's arithmetic (csrc/qs_compress.h) compiled for the host, for
 * tests/test_compress_host.py: the same colour conversion, edge and downsample rules, forward DCT passes and quantiser
 * the kernel runs, fed from files.  A stand-alone program: it is also built with -fsanitize=address,undefined and run
 * as a program.
 *
 *   compress_host image in.bin out.bin   a whole image; in.bin as `libjpeg9_compress image` takes it; out.bin in the
 *                                        format of `libjpeg9_decode read` (width_in_blocks x height_in_blocks blocks)
 *   compress_host block in.bin out.bin   qc_fdct_row + qc_fdct_col on blocks: int32 n, n x 64 samples -> n x 64 int32
 *   compress_host quantcheck             qc_quant against the plain division over |w| < 2^17 for a set of tables;
 *                                        prints mismatches=<count>
 *   compress_host info                   key=value lines: the header's constants
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "qs_compress.h"

#define MAGIC 0x51534a43

static int do_info() {
  printf("chunk=%d\ntile_w=%d\ntile_h=%d\njob_size=%zu\nptrs_size=%zu\nargs_size=%zu\n", QS_CMP_CHUNK, QS_CMP_TW,
         QS_CMP_TH, sizeof(QsCmpJob), sizeof(QsCmpPtrs), sizeof(QsCmpArgs));
  return 0;
}

static void fdct_block(const uint8_t* s, int stride, int32_t* w) {
  int32_t d[64], col[8], o[8];
  for (int r = 0; r < 8; ++r) qc_fdct_row(s + (size_t)r * stride, d + r * 8);
  for (int c = 0; c < 8; ++c) {
    for (int r = 0; r < 8; ++r) col[r] = d[r * 8 + c];
    qc_fdct_col(col, o);
    for (int r = 0; r < 8; ++r) w[r * 8 + c] = o[r];
  }
}

static int do_block(const char* src, const char* dst) {
  FILE *in = fopen(src, "rb"), *out = fopen(dst, "wb");
  int32_t n;
  if (!in || !out || fread(&n, sizeof n, 1, in) != 1 || n < 0) { fprintf(stderr, "compress_host: bad input\n"); return 1; }
  for (int b = 0; b < n; ++b) {
    uint8_t s[64];
    int32_t w[64];
    if (fread(s, sizeof s, 1, in) != 1) { fprintf(stderr, "compress_host: short input\n"); return 1; }
    fdct_block(s, 8, w);
    fwrite(w, sizeof w, 1, out);
  }
  fclose(in);
  return fclose(out) != 0;
}

static int do_quantcheck() {
  std::vector<uint32_t> qs;
  for (uint32_t q = 1; q <= 1024; ++q) qs.push_back(q);
  for (uint32_t q = 1025; q < 65536; q += 251) qs.push_back(q);
  for (uint32_t q : {32767u, 32768u, 65534u, 65535u}) qs.push_back(q);
  long long bad = 0;
  for (uint32_t q : qs) {
    const uint32_t d = q << 3, m = qc_recip(d);
    for (int32_t w = -(1 << 17) + 1; w < (1 << 17); ++w) {
      const int32_t a = (w < 0 ? -w : w) + (int32_t)(d >> 1);
      const int32_t t = a / (int32_t)d;
      bad += qc_quant(w, q, m) != (int16_t)(w < 0 ? -t : t);
    }
  }
  printf("mismatches=%lld\n", bad);
  return bad != 0;
}

static int do_image(const char* src, const char* dst) {
  FILE* in = fopen(src, "rb");
  int32_t hdr[5];
  if (!in || fread(hdr, sizeof hdr, 1, in) != 1 || hdr[0] != MAGIC) { fprintf(stderr, "compress_host: bad header\n"); return 1; }
  const int n = hdr[1], W = hdr[2], H = hdr[3], cs = hdr[4];
  if ((n != 1 && n != 3) || W < 1 || H < 1) { fprintf(stderr, "compress_host: bad geometry\n"); return 1; }
  int32_t samp[3][2];
  uint16_t q[3][64];
  uint32_t m[3][64];
  for (int c = 0; c < n; ++c) {
    if (fread(samp[c], sizeof samp[c], 1, in) != 1 || fread(q[c], sizeof q[c], 1, in) != 1) return 1;
    for (int i = 0; i < 64; ++i) m[c][i] = qc_recip((uint32_t)q[c][i] << 3);
  }
  std::vector<uint8_t> px((size_t)W * H * n);
  if (fread(px.data(), 1, px.size(), in) != px.size()) { fprintf(stderr, "compress_host: short pixels\n"); return 1; }
  fclose(in);
  const int hs = n == 1 ? 1 : samp[0][0], vs = n == 1 ? 1 : samp[0][1];
  // the component planes, each over its blocks: conversion, then box downsampling under the edge rules
  FILE* out = fopen(dst, "wb");
  if (!out) return 1;
  fwrite(hdr, sizeof hdr, 1, out);
  int wib[3], hib[3];
  for (int c = 0; c < n; ++c) {
    const int h_c = c ? 1 : hs, v_c = c ? 1 : vs;
    wib[c] = qc_blocks(W, h_c, hs);
    hib[c] = qc_blocks(H, v_c, vs);
    int32_t g[5] = {wib[c], hib[c], n == 1 ? samp[0][0] : h_c, n == 1 ? samp[0][1] : v_c, 1};
    fwrite(g, sizeof g, 1, out);
    fwrite(q[c], sizeof q[c], 1, out);
  }
  for (int c = 0; c < n; ++c) {
    const int hx = c ? hs : 1, vy = c ? vs : 1;            // the box one sample of this component covers
    const int pw = wib[c] * 8, ph = hib[c] * 8;
    std::vector<uint8_t> plane((size_t)pw * ph);
    for (int r = 0; r < ph; ++r)
      for (int x = 0; x < pw; ++x) {
        int sum = 0;
        for (int dy = 0; dy < vy; ++dy)
          for (int dx = 0; dx < hx; ++dx) {
            const int sy = qc_src_row(r, dy, H, vs, c ? 1 : vs), sx = qc_src_col(x * hx + dx, W);
            const uint8_t* p = &px[((size_t)sy * W + sx) * n];
            uint8_t ycc[3];
            if (n == 3 && cs == 3) {
              qc_rgb_ycc(p[0], p[1], p[2], ycc);
              sum += ycc[c];
            } else {
              sum += p[c];
            }
          }
        plane[(size_t)r * pw + x] = (uint8_t)(hx * vy == 1 ? sum : qc_downsample(sum, hx, vy, x));
      }
    for (int by = 0; by < hib[c]; ++by)
      for (int bx = 0; bx < wib[c]; ++bx) {
        int32_t w[64];
        int16_t coef[64];
        fdct_block(&plane[((size_t)by * 8) * pw + bx * 8], pw, w);
        for (int i = 0; i < 64; ++i) coef[i] = qc_quant(w[i], q[c][i], m[c][i]);
        fwrite(coef, sizeof coef, 1, out);
      }
  }
  return fclose(out) != 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "info")) return do_info();
  if (argc == 2 && !strcmp(argv[1], "quantcheck")) return do_quantcheck();
  if (argc == 4 && !strcmp(argv[1], "block")) return do_block(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "image")) return do_image(argv[2], argv[3]);
  fprintf(stderr, "usage: compress_host info | quantcheck | block in.bin out.bin | image in.bin out.bin\n");
  return 2;
}
