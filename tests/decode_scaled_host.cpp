/*
 * decode_scaled_host.cpp -- the device decode's reduced sizes (csrc/qs_decode.h) compiled for
 * the host, for tests/test_decode_scaled_host.py: the same qd_scaled_item and qd_scaled_convert a lane of
 * qs_decode_scaled_kernel runs, fed from files.  Also built with -fsanitize=address,undefined: the output, the tile's
 * planes and rows and every coefficient array are heap blocks of exactly the kernel's sizes.
 *
 *   decode_scaled_host info                      key=value lines: the 4-point pass-1 bound, its matrix's L1 norm, the
 *                                                tile, the sizes of a job's workspace and kernel-argument records
 *   decode_scaled_host block KIND in.bin out.bin qd_scaled_block on blocks; KIND 4x4, 2x2, 1x1, 8x4, 4x2, 2x1, 4x8, 2x4,
 *                                                1x2 (width x height); files as `libjpeg9_decode_scaled block` takes them
 *   decode_scaled_host decode in.bin out.raw DENOM   a whole image tile by tile, work item by work item; files as
 *                                                `libjpeg9_decode_scaled decode` takes and writes them
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "qs_decode.h"

#define MAGIC 0x51534a43

// the largest row L1 norm of the 4-point pass-1 odd part: unit vectors through the 64-bit form give its columns
static long long l1_norm4() {
  long long m[2][2];
  for (int k = 0; k < 2; ++k) {
    int64_t o[2];
    qd_idct4_odd<int64_t>(k == 0, k == 1, 0, o);
    m[0][k] = (long long)o[0]; m[1][k] = (long long)o[1];
  }
  long long best = 0;
  for (int i = 0; i < 2; ++i) {
    const long long s = llabs(m[i][0]) + llabs(m[i][1]);
    if (s > best) best = s;
  }
  return best;
}

static int do_info() {
  printf("fast_bound4=%lld\nfast_bound=%lld\nl1_4=%lld\n", (long long)QS_DEC_FAST_BOUND4, (long long)QS_DEC_FAST_BOUND, l1_norm4());
  printf("chunk=%d\ntile_w=%d\ntile_h=%d\n", QS_DEC_CHUNK, QS_DEC_TW, QS_DEC_TH);
  printf("job_size=%zu\nptrs_size=%zu\n", sizeof(QsDecJob), sizeof(QsDecPtrs));
  return 0;
}

static int do_block(const char* kind, const char* src, const char* dst) {
  static const char* kinds[9] = {"4x4", "2x2", "1x1", "8x4", "4x2", "2x1", "4x8", "2x4", "1x2"};
  int which = -1;
  for (int i = 0; i < 9; ++i)
    if (!strcmp(kind, kinds[i])) which = i;
  if (which < 0) { fprintf(stderr, "decode_scaled_host: unknown kind %s\n", kind); return 1; }
  const int cols = kind[0] - '0', rows = kind[2] - '0';
  FILE *in = fopen(src, "rb"), *out = fopen(dst, "wb");
  int32_t n;
  if (!in || !out || fread(&n, sizeof n, 1, in) != 1 || n < 0) { fprintf(stderr, "decode_scaled_host: bad input\n"); return 1; }
  std::vector<uint8_t> px((size_t)rows * cols);
  for (int b = 0; b < n; ++b) {
    alignas(16) int16_t coef[64];
    uint16_t q[64];
    if (fread(coef, sizeof coef, 1, in) != 1 || fread(q, sizeof q, 1, in) != 1) {
      fprintf(stderr, "decode_scaled_host: short input\n");
      return 1;
    }
    switch (which) {
      case 0: qd_scaled_block<4, 4>(coef, q, px.data(), cols); break;
      case 1: qd_scaled_block<2, 2>(coef, q, px.data(), cols); break;
      case 2: qd_scaled_block<1, 1>(coef, q, px.data(), cols); break;
      case 3: qd_scaled_block<8, 4>(coef, q, px.data(), cols); break;
      case 4: qd_scaled_block<4, 2>(coef, q, px.data(), cols); break;
      case 5: qd_scaled_block<2, 1>(coef, q, px.data(), cols); break;
      case 6: qd_scaled_block<4, 8>(coef, q, px.data(), cols); break;
      case 7: qd_scaled_block<2, 4>(coef, q, px.data(), cols); break;
      default: qd_scaled_block<1, 2>(coef, q, px.data(), cols); break;
    }
    fwrite(px.data(), 1, px.size(), out);
  }
  fclose(in);
  return fclose(out) != 0;
}

static int do_decode(const char* src, const char* dst, int denom) {
  FILE* in = fopen(src, "rb");
  int32_t hdr[5], g[3][5];
  if (!in || fread(hdr, sizeof hdr, 1, in) != 1 || hdr[0] != MAGIC || (hdr[1] != 1 && hdr[1] != 3)) {
    fprintf(stderr, "decode_scaled_host: bad header\n");
    return 1;
  }
  if (denom != 2 && denom != 4 && denom != 8) { fprintf(stderr, "decode_scaled_host: DENOM 2, 4 or 8\n"); return 1; }
  const int n = hdr[1], W = hdr[2], H = hdr[3];
  QsDecJob job;
  QsDecPtrs P;
  memset(&job, 0, sizeof job);
  memset(&P, 0, sizeof P);
  for (int c = 0; c < n; ++c) {
    if (fread(g[c], sizeof g[c], 1, in) != 1 || fread(job.q[c], sizeof job.q[c], 1, in) != 1) return 1;
    job.g[0].wblk[c] = g[c][0]; job.g[0].hblk[c] = g[c][1];
  }
  job.layout = n == 1 ? QS_DEC_GRAY : hdr[4] == 3 ? QS_DEC_YCC : QS_DEC_RGB;
  job.g[0].hs = n == 1 ? 1 : g[0][2]; job.g[0].vs = n == 1 ? 1 : g[0][3];
  job.upsampling = (int16_t)(QS_DEC_UP_DCT + 256 * denom);
  const int m = qd_job_m(job);
  job.nout = n == 1 ? 1 : 3;
  job.width = (W * m + 7) / 8; job.height = (H * m + 7) / 8;
  int16_t* arr[3] = {nullptr, nullptr, nullptr};
  for (int c = 0; c < n; ++c) {                            // each array a heap block of exactly its size
    const size_t bytes = (size_t)g[c][0] * g[c][1] * 128;
    if (posix_memalign((void**)&arr[c], 16, bytes ? bytes : 16) || fread(arr[c], 1, bytes, in) != bytes) {
      fprintf(stderr, "decode_scaled_host: short input\n");
      return 1;
    }
    P.coef[c] = arr[c];
    P.nblk[c] = g[c][0] * g[c][1];
  }
  fclose(in);
  const int nout = job.nout, OW = job.width, OH = job.height;
  uint8_t* out = (uint8_t*)malloc((size_t)OW * OH * nout);
  P.out = out; P.pitch = (int64_t)OW * nout; P.width = OW; P.height = OH;
  const int items = qd_scaled_items(job, job.g[0], m);
  for (int Y0 = 0; Y0 < OH; Y0 += QS_DEC_TH)
    for (int X0 = 0; X0 < OW; X0 += QS_DEC_TW) {
      uint8_t* px = (uint8_t*)malloc(3 * QS_DEC_TH * QS_DEC_TW);       // the kernel's two LDS arrays
      uint8_t* rows = (uint8_t*)malloc(QS_DEC_TH * QS_DEC_TW * 3);
      memset(px, 0xAA, 3 * QS_DEC_TH * QS_DEC_TW);
      for (int it = 0; it < items; ++it) qd_scaled_item(job, P, job.g[0], 0, m, OW, OH, X0, Y0, it, px);
      const int w = OW - X0 < QS_DEC_TW ? OW - X0 : QS_DEC_TW, h = OH - Y0 < QS_DEC_TH ? OH - Y0 : QS_DEC_TH;
      for (int x = 0; x < w; ++x)
        for (int r = 0; r < h; ++r) qd_scaled_convert(job, px, r, x, rows);
      for (int r = 0; r < h; ++r)
        memcpy(out + (size_t)(Y0 + r) * P.pitch + (size_t)X0 * nout, rows + (size_t)r * QS_DEC_TW * 3, (size_t)w * nout);
      free(px);
      free(rows);
    }
  FILE* o = fopen(dst, "wb");
  if (!o) return 1;
  const int32_t shape[3] = {OW, OH, nout};
  fwrite(shape, sizeof shape, 1, o);
  fwrite(out, 1, (size_t)OW * OH * nout, o);
  free(out);
  for (int c = 0; c < n; ++c) free(arr[c]);
  return fclose(o) != 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "info")) return do_info();
  if (argc == 5 && !strcmp(argv[1], "block")) return do_block(argv[2], argv[3], argv[4]);
  if (argc == 5 && !strcmp(argv[1], "decode")) return do_decode(argv[2], argv[3], atoi(argv[4]));
  fprintf(stderr, "usage: decode_scaled_host info | block KIND in.bin out.bin | decode in.bin out.raw DENOM\n");
  return 2;
}
