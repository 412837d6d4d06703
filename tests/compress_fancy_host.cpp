/*
 * compress_fancy_host.cpp -- the device compress's arithmetic (csrc/qs_compress.h) with both chroma downsampling modes,
 * compiled for the host, for tests/test_compress_fancy_host.py: the block functions the lanes of a block run together
 * (16-point passes included), the plain-clamp edge rule of the DCT-scaled mode and the quantiser, fed from files.  A
 * stand-alone program: it is also built with -fsanitize=address,undefined and run as a program.
 *
 *   compress_fancy_host image box|dct in.bin out.bin   a whole image; in.bin as `libjpeg9_compress image` takes it;
 *                                                      out.bin in the format of `libjpeg9_decode read`
 *   compress_fancy_host block WxH in.bin out.bin       the block function of WxH = 16x16 | 16x8 | 8x16 samples (W wide):
 *                                                      int32 n, n x H x W samples -> n x 64 int32
 *   compress_fancy_host norms                          key=value lines: the integer matrices of the 8- and 16-point
 *                                                      passes taken with unit vectors, their rows' L1 norms, and the
 *                                                      bounds on every pass's sums for 8-bit samples
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "qs_compress.h"

#define MAGIC 0x51534a43

// one block of dw x dh samples -> 64 outputs scaled by 8, as the eight lanes of a block run it
static void fdct_block(const uint8_t* s, int stride, int dw, int dh, int32_t* w) {
  int32_t d[16 * 8], col[16], o[8];
  for (int r = 0; r < dh; ++r) {
    if (dw == 16) qc_fdct16_row(s + (size_t)r * stride, d + r * 8);
    else qc_fdct_row(s + (size_t)r * stride, d + r * 8);
  }
  for (int c = 0; c < 8; ++c) {
    for (int r = 0; r < dh; ++r) col[r] = d[r * 8 + c];
    if (dh == 16) qc_fdct16_col(col, dw == 16 ? 2 : 1, o);
    else if (dw == 16) qc_fdct_col_half(col, o);
    else qc_fdct_col(col, o);
    for (int r = 0; r < 8; ++r) w[r * 8 + c] = o[r];
  }
}

static int shape_of(const char* s, int* dw, int* dh) {
  if (!strcmp(s, "16x16")) { *dw = 16; *dh = 16; return 0; }
  if (!strcmp(s, "16x8")) { *dw = 16; *dh = 8; return 0; }
  if (!strcmp(s, "8x16")) { *dw = 8; *dh = 16; return 0; }
  if (!strcmp(s, "8x8")) { *dw = 8; *dh = 8; return 0; }
  fprintf(stderr, "compress_fancy_host: block shape %s\n", s);
  return 2;
}

static int do_block(const char* shape, const char* src, const char* dst) {
  int dw, dh;
  if (int r = shape_of(shape, &dw, &dh)) return r;
  FILE *in = fopen(src, "rb"), *out = fopen(dst, "wb");
  int32_t n;
  if (!in || !out || fread(&n, sizeof n, 1, in) != 1 || n < 0) { fprintf(stderr, "compress_fancy_host: bad input\n"); return 1; }
  for (int b = 0; b < n; ++b) {
    uint8_t s[256];
    int32_t w[64];
    if (fread(s, (size_t)dw * dh, 1, in) != 1) { fprintf(stderr, "compress_fancy_host: short input\n"); return 1; }
    fdct_block(s, dw, dw, dh, w);
    fwrite(w, sizeof w, 1, out);
  }
  fclose(in);
  return fclose(out) != 0;
}

// ---- the bounds: each pass is an integer matrix and one rounding shift -------------------------------------------------
static int do_norms() {
  int64_t m16[8][16], m8[8][8];
  for (int k = 0; k < 16; ++k) {                           // unit vectors: column k of the matrix
    int64_t in[16] = {0}, o[8];
    in[k] = 1;
    qc_fdct16<int64_t>(in, o);
    for (int i = 0; i < 8; ++i) m16[i][k] = o[i];
  }
  for (int k = 0; k < 8; ++k) {
    uint32_t in[8] = {0}, o[8];
    in[k] = 1;
    qc_fdct8(in, 0, 0, o);
    for (int i = 0; i < 8; ++i) m8[i][k] = (int32_t)o[i];  // (entries below 2^15: the residue is the entry)
  }
  int64_t l16[8], l8[8], s16[8], s8[8], l16max = 0, l8max = 0;
  for (int i = 0; i < 8; ++i) {
    l16[i] = l8[i] = s16[i] = s8[i] = 0;
    for (int k = 0; k < 16; ++k) { l16[i] += llabs(m16[i][k]); s16[i] += m16[i][k]; }
    for (int k = 0; k < 8; ++k) { l8[i] += llabs(m8[i][k]); s8[i] += m8[i][k]; }
    printf("l1_16_%d=%lld\nl1_8_%d=%lld\nrowsum_16_%d=%lld\nrowsum_8_%d=%lld\n", i, (long long)l16[i], i, (long long)l8[i],
           i, (long long)s16[i], i, (long long)s8[i]);
    if (i) { l16max = std::max(l16max, l16[i]); l8max = std::max(l8max, l8[i]); }
  }
  // pass 1 on samples: rows 1..7 sum to zero, so x may be taken as x - 128 in [-128, 127]; row 0 is the plain sum
  const int64_t p1_16 = l16max * 128 + (1 << 10), p1_8 = l8max * 128 + (1 << 10);
  const int64_t d16 = std::max<int64_t>(p1_16 >> 11, 16 * 128 * 4), d8 = std::max<int64_t>(p1_8 >> 11, 8 * 128 * 4);
  // pass 2: a column of |d| <= dmax through either matrix; row 0 (L1 16 or 8) is far below the scaled rows
  const int64_t p2_16x16 = l16max * d16 + (1 << 16), p2_8x16 = l16max * d8 + (1 << 15), p2_16x8 = l8max * d16 + (1 << 15);
  printf("l1max_16=%lld\nl1max_8=%lld\npass1_16=%lld\npass1_8=%lld\ndmax_16=%lld\ndmax_8=%lld\n", (long long)l16max,
         (long long)l8max, (long long)p1_16, (long long)p1_8, (long long)d16, (long long)d8);
  printf("pass2_16x16=%lld\npass2_8x16=%lld\npass2_16x8=%lld\n", (long long)p2_16x16, (long long)p2_8x16, (long long)p2_16x8);
  printf("wmax_16x16=%lld\nwmax_8x16=%lld\nwmax_16x8=%lld\n", (long long)(p2_16x16 >> 17), (long long)(p2_8x16 >> 16),
         (long long)(p2_16x8 >> 16));
  const int64_t lim = (int64_t)1 << 31;
  printf("needs64=%d\n", p1_16 >= lim || p1_8 >= lim || p2_16x16 >= lim || p2_8x16 >= lim || p2_16x8 >= lim);
  return 0;
}

static int do_image(const char* modename, const char* src, const char* dst) {
  int mode;
  if (!strcmp(modename, "box")) mode = QS_CMP_DS_BOX;
  else if (!strcmp(modename, "dct")) mode = QS_CMP_DS_DCT;
  else { fprintf(stderr, "compress_fancy_host: mode %s\n", modename); return 2; }
  FILE* in = fopen(src, "rb");
  int32_t hdr[5];
  if (!in || fread(hdr, sizeof hdr, 1, in) != 1 || hdr[0] != MAGIC) { fprintf(stderr, "compress_fancy_host: bad header\n"); return 1; }
  const int n = hdr[1], W = hdr[2], H = hdr[3], cs = hdr[4];
  if ((n != 1 && n != 3) || W < 1 || H < 1) { fprintf(stderr, "compress_fancy_host: bad geometry\n"); return 1; }
  int32_t samp[3][2];
  uint16_t q[3][64];
  uint32_t m[3][64];
  for (int c = 0; c < n; ++c) {
    if (fread(samp[c], sizeof samp[c], 1, in) != 1 || fread(q[c], sizeof q[c], 1, in) != 1) return 1;
    for (int i = 0; i < 64; ++i) m[c][i] = qc_recip((uint32_t)q[c][i] << 3);
  }
  std::vector<uint8_t> px((size_t)W * H * n);
  if (fread(px.data(), 1, px.size(), in) != px.size()) { fprintf(stderr, "compress_fancy_host: short pixels\n"); return 1; }
  fclose(in);
  const int hs = n == 1 ? 1 : samp[0][0], vs = n == 1 ? 1 : samp[0][1];
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
    QsCmpShape sh = {1, 1, 8, 8};                          // luma: no box, the 8x8 DCT
    if (c) sh = qc_chroma_shape(mode, hs, vs);
    const int pw = wib[c] * sh.dw, ph = hib[c] * sh.dh;    // the plane the DCTs read
    std::vector<uint8_t> plane((size_t)pw * ph);
    for (int r = 0; r < ph; ++r)
      for (int x = 0; x < pw; ++x) {
        int sum = 0;
        for (int dy = 0; dy < sh.bv; ++dy)
          for (int dx = 0; dx < sh.bh; ++dx) {
            const int sy = mode == QS_CMP_DS_DCT ? (r < H - 1 ? r : H - 1) : qc_src_row(r, dy, H, vs, c ? 1 : vs);
            const int sx = qc_src_col(x * sh.bh + dx, W);
            const uint8_t* p = &px[((size_t)sy * W + sx) * n];
            uint8_t ycc[3];
            if (n == 3 && cs == 3) {
              qc_rgb_ycc(p[0], p[1], p[2], ycc);
              sum += ycc[c];
            } else {
              sum += p[c];
            }
          }
        plane[(size_t)r * pw + x] = (uint8_t)(sh.bh * sh.bv == 1 ? sum : qc_downsample(sum, sh.bh, sh.bv, x));
      }
    for (int by = 0; by < hib[c]; ++by)
      for (int bx = 0; bx < wib[c]; ++bx) {
        int32_t w[64];
        int16_t coef[64];
        fdct_block(&plane[((size_t)by * sh.dh) * pw + bx * sh.dw], pw, sh.dw, sh.dh, w);
        for (int i = 0; i < 64; ++i) coef[i] = qc_quant(w[i], q[c][i], m[c][i]);
        fwrite(coef, sizeof coef, 1, out);
      }
  }
  return fclose(out) != 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "norms")) return do_norms();
  if (argc == 5 && !strcmp(argv[1], "block")) return do_block(argv[2], argv[3], argv[4]);
  if (argc == 5 && !strcmp(argv[1], "image")) return do_image(argv[2], argv[3], argv[4]);
  fprintf(stderr, "usage: compress_fancy_host norms | block 16x16|16x8|8x16 in.bin out.bin | image box|dct in.bin out.bin\n");
  return 2;
}
