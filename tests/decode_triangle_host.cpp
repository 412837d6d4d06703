/*
 * decode_triangle_host.cpp -- the device decode's triangle mode (csrc/qs_decode.h: qd_idct_block, qd_tri_column,
 * qd_tri_block_needed, qd_ycc_rgb_turbo) compiled for the host, for tests/test_decode_triangle_host.py: whole images decoded
 * tile by tile the way the kernel's workgroups do it -- the same tile size, the same planes of chroma blocks with one
 * block of context, the same per-column filter call -- built plain and with -fsanitize=address,undefined.  Each plane is
 * its own heap block of exactly the kernel's size and is filled with 0xA5 before every tile, so a read outside a plane
 * is a sanitizer report and a read of a block the tile did not compute is a wrong sample.
 *
 *   decode_triangle_host run in.bin out.bin
 *
 * in.bin: int32 number of cases, then per case
 *   int32 flags (1: no colour conversion -- the upsampled components interleaved, whatever the colour space),
 *   int32 magic, ncomp, width, height, colorspace; per component int32 wblk (row stride in blocks), hblk, hsamp, vsamp,
 *   has_table and uint16 table[64]; then each component's int16 coefficients (hblk * wblk * 64).
 * out.bin: per case height * width * (1 or 3) samples.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "qs_decode.h"

#define MAGIC 0x51534A43

struct Comp {
  int32_t wblk, hblk, hs, vs, hasq;
  uint16_t q[64];
  std::vector<int16_t> coef;
};

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

static void idct_into(const Comp& c, int bx, int by, uint8_t* dst, int stride) {
  int32_t dq[64];
  qd_dequant(c.coef.data() + ((size_t)by * c.wblk + bx) * 64, c.q, dq);
  qd_idct_block<false, false>(dq, dst, stride);
}

static int decode_case(FILE* in, FILE* out) {
  int32_t flags, head[5];
  if (!rd(in, &flags, 4) || !rd(in, head, sizeof head) || head[0] != MAGIC) return 1;
  const int n = head[1], W = head[2], H = head[3], cs = head[4];
  if ((n != 1 && n != 3) || W < 1 || H < 1) return 1;
  std::vector<Comp> comp((size_t)n);
  for (Comp& c : comp)
    if (!rd(in, &c.wblk, 20) || !rd(in, c.q, sizeof c.q) || c.wblk < 1 || c.hblk < 1) return 1;
  for (Comp& c : comp) {
    c.coef.resize((size_t)c.wblk * c.hblk * 64);
    if (!rd(in, c.coef.data(), c.coef.size() * 2)) return 1;
  }
  const int hs = n == 1 ? 1 : comp[0].hs, vs = n == 1 ? 1 : comp[0].vs;
  if (n == 3 && (comp[1].hs != 1 || comp[1].vs != 1 || comp[2].hs != 1 || comp[2].vs != 1)) return 1;
  if (!((hs == 1 || hs == 2 || hs == 4) && (vs == 1 || vs == 2) && hs * vs <= 4)) return 1;
  const int nout = n == 1 ? 1 : 3;
  const bool convert = n == 3 && cs == 3 && !(flags & 1);
  const bool tri = n == 3 && hs * vs > 1;
  const int cw = 8 * hs, ch = 8 * vs;
  const int hx = tri ? qd_tri_halo_x(hs) : 0, hy = tri ? qd_tri_halo_y(vs) : 0;
  const int Wc = (W + hs - 1) / hs, Hc = (H + vs - 1) / vs;
  const int ncx = QS_DEC_TW / cw + 2 * hx, ncy = QS_DEC_TH / ch + 2 * hy;
  if (ncx * 8 > QS_DEC_TRI_W || ncy * 8 > QS_DEC_TRI_H) return 1;
  std::vector<uint8_t> img((size_t)W * H * nout);
  std::vector<uint8_t> px[3], cpx[2];
  for (int t = 0, tx = (W + QS_DEC_TW - 1) / QS_DEC_TW; t < tx * ((H + QS_DEC_TH - 1) / QS_DEC_TH); ++t) {
    const int X0 = (t % tx) * QS_DEC_TW, Y0 = (t / tx) * QS_DEC_TH;
    for (auto& p : px) p.assign((size_t)QS_DEC_TH * QS_DEC_TW, 0xA5);
    for (auto& p : cpx) p.assign((size_t)QS_DEC_TRI_H * QS_DEC_TRI_W, 0xA5);
    for (int lane = 0; lane < 16; ++lane) {                // luma: the kernel's lanes 0 .. 15
      const int bx = (X0 >> 3) + (lane & 7), by = (Y0 >> 3) + (lane >> 3);
      const int x0 = (lane & 7) * 8, y0 = (lane >> 3) * 8;
      if (X0 + x0 < W && Y0 + y0 < H && bx < comp[0].wblk && by < comp[0].hblk)
        idct_into(comp[0], bx, by, &px[0][(size_t)y0 * QS_DEC_TW + x0], QS_DEC_TW);
    }
    for (int ci = 1; ci < n; ++ci)
      for (int k = 0; k < ncx * ncy; ++k) {
        const int kx = k % ncx, ky = k / ncx;
        const int bx = X0 / cw + kx - hx, by = Y0 / ch + ky - hy;
        const int x0 = (kx - hx) * cw, y0 = (ky - hy) * ch;
        const bool needed = tri ? qd_tri_block_needed(bx, by, Wc, Hc) : X0 + x0 < W && Y0 + y0 < H;
        if (!needed || bx >= comp[ci].wblk || by >= comp[ci].hblk) continue;
        if (tri) idct_into(comp[ci], bx, by, &cpx[ci - 1][(size_t)ky * 8 * QS_DEC_TRI_W + kx * 8], QS_DEC_TRI_W);
        else idct_into(comp[ci], bx, by, &px[ci][(size_t)y0 * QS_DEC_TW + x0], QS_DEC_TW);
      }
    const int w = W - X0 < QS_DEC_TW ? W - X0 : QS_DEC_TW, h = H - Y0 < QS_DEC_TH ? H - Y0 : QS_DEC_TH;
    for (int lane = 0; lane < w; ++lane) {
      if (tri)
        for (int ci = 1; ci < 3; ++ci)
          qd_tri_column_any(hs, vs, cpx[ci - 1].data(), QS_DEC_TRI_W, X0 / hs - 8 * hx, Y0 / vs - 8 * hy, Wc, Hc,
                            X0 + lane, Y0, &px[ci][lane], QS_DEC_TW);
      for (int r = 0; r < h; ++r) {
        uint8_t* o = &img[((size_t)(Y0 + r) * W + X0 + lane) * nout];
        const size_t at = (size_t)r * QS_DEC_TW + lane;
        if (convert) qd_ycc_rgb_turbo(px[0][at], px[1][at], px[2][at], o);
        else for (int ci = 0; ci < nout; ++ci) o[ci] = px[ci][at];
      }
    }
  }
  return fwrite(img.data(), 1, img.size(), out) != img.size();
}

int main(int argc, char** argv) {
  if (argc != 4 || strcmp(argv[1], "run")) {
    fprintf(stderr, "usage: decode_triangle_host run in.bin out.bin\n");
    return 2;
  }
  FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
  int32_t n;
  if (!in || !out || !rd(in, &n, 4) || n < 0) { fprintf(stderr, "decode_triangle_host: bad input\n"); return 1; }
  for (int i = 0; i < n; ++i)
    if (decode_case(in, out)) { fprintf(stderr, "decode_triangle_host: case %d: bad input\n", i); return 1; }
  fclose(in);
  return fclose(out) != 0;
}
