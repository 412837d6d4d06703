// qs_kernels_compress.hip -- the kernel of the device compress (csrc/qs_compress_job.cpp,
// qs_hip_compress_device_batch): colour conversion, edge replication, box-filter chroma downsampling, forward DCT and
// quantisation exactly as libjpeg 9 does them with JDCT_ISLOW and do_fancy_downsampling = FALSE (the fancy mode, its
// default, is out of scope: see qs_compress.h), for every job of a batch in ONE launch.
//
// The decode's shape, reversed.  A workgroup (one wave) owns an input tile of QS_CMP_TW x QS_CMP_TH = 64 x 16 pixels of
// one job, a whole number of MCUs in every supported layout.
//   phase 1  the tile's 16 pixel rows into LDS, consecutive lanes on consecutive bytes (dwords where a row's first byte
//            is 4-byte aligned and the tile lies inside the image: 48 lanes per RGB row, 16 per gray row); rows and
//            columns beyond the image are replicated here, by address: a source column is min(x, W - 1), a source
//            row min(y, H - 1).
//   phase 2  one lane per column converts colour into three LDS planes (jccolor.c);
//   phase 3  subsampled chroma: box sums of the converted planes under libjpeg's two-step vertical edge rule
//            (qc_src_row: the last DOWNSAMPLED row is repeated, not the last pixel row);
//   phase 4  the forward DCT, eight blocks at a time and EIGHT LANES PER BLOCK: lane k of a block runs row k's pass 1
//            from the plane, the rows meet in an LDS transpose (row stride 9 dwords: by construction, not by
//            measurement, each half-wave's 32 accesses fall into 32 different banks, writing and reading), lane k
//            runs column k's pass 2 and quantises its eight outputs, and a second LDS transpose hands lane k the
//            block's row k as 16 bytes.  Eight consecutive blocks of a block row are 1024 consecutive bytes of the
//            array: each store instruction writes them with consecutive lanes on consecutive 16 bytes.
// Blocks outside libjpeg's width_in_blocks x height_in_blocks are not written.
//
// Geometry and tables live in the caller's workspace (written by the prepare call); the pixels, the arrays and their
// extents travel in the kernel arguments (QsCmpArgs), one chunk of up to QS_CMP_CHUNK jobs per launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qs_compress.h"

#define QS_CMP_LANES 64
#define QS_CMP_RAW (QS_CMP_TW * 3)       // bytes of one raw pixel row of the tile
#define QS_CMP_WS 72                     // dwords of one block in the transpose buffer: 8 rows of 9
#define QS_CMP_SCRATCH (8 * QS_CMP_WS * 4 + 8 * 128)       // the two transpose buffers: 3328 bytes

__global__ void __launch_bounds__(QS_CMP_LANES)
qs_compress_kernel(const QsCmpArgs a) {
  // raw rows (phases 1-2), then the two transpose buffers of phase 4 in the same bytes
  __shared__ __attribute__((aligned(16))) uint8_t scratch[QS_CMP_SCRATCH];
  __shared__ __attribute__((aligned(16))) uint8_t px[3][QS_CMP_TH][QS_CMP_TW];     // converted samples, full resolution
  __shared__ __attribute__((aligned(16))) uint8_t ds[2][QS_CMP_TH][QS_CMP_TW];     // downsampled chroma
  static_assert(QS_CMP_TH * QS_CMP_RAW <= QS_CMP_SCRATCH, "the raw rows fit the bytes of the transpose buffers");
  int32_t* const ws = reinterpret_cast<int32_t*>(scratch);                          // [8][QS_CMP_WS]
  int16_t* const tr = reinterpret_cast<int16_t*>(scratch + 8 * QS_CMP_WS * 4);      // [8][64]

  const QsCmpJob* J = a.jobs;
  const int tile = (int)blockIdx.x;
  int lo = 0, hi = a.n - 1;                                // the job whose tiles hold this workgroup
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (J[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  const QsCmpJob& job = J[lo];
  const int t = tile - job.tile0;
  if (t < 0 || t >= job.tiles) return;
  const QsCmpPtrs& P = a.p[lo];
  const int hs = job.hs, vs = job.vs;
  if ((hs != 1 && hs != 2 && hs != 4) || (vs != 1 && vs != 2) || hs * vs > 4) return;    // (never prepared)
  const int W = min(job.width, P.width), H = min(job.height, P.height);
  const int X0 = (t % job.tiles_x) * QS_CMP_TW, Y0 = (t / job.tiles_x) * QS_CMP_TH;
  if (W < 1 || H < 1 || X0 >= W || Y0 >= H) return;
  const int nin = job.layout == QS_CMP_GRAY ? 1 : 3;
  const int lane = (int)threadIdx.x;

  // phase 1: the raw rows
  const int nb = QS_CMP_TW * nin;
  const bool inside = X0 + QS_CMP_TW <= W;
  for (int r = 0; r < QS_CMP_TH; ++r) {
    const int y = min(Y0 + r, H - 1);
    const uint8_t* row = P.pix + (size_t)y * (size_t)P.pitch;
    uint8_t* dst = scratch + r * QS_CMP_RAW;
    if (inside && ((reinterpret_cast<uintptr_t>(row) + (size_t)X0 * nin) & 3) == 0) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(row + (size_t)X0 * nin);
      if (lane < nb / 4) reinterpret_cast<uint32_t*>(dst)[lane] = src[lane];
    } else {
      for (int b = lane; b < nb; b += QS_CMP_LANES) {
        const int xp = b / nin, ch = b - xp * nin;
        dst[b] = row[(size_t)min(X0 + xp, W - 1) * nin + ch];
      }
    }
  }
  __syncthreads();

  // phase 2: colour conversion, one lane per column (jccolor.c: rgb_ycc_convert, rgb_convert, grayscale_convert)
  for (int r = 0; r < QS_CMP_TH; ++r) {
    const uint8_t* s = scratch + r * QS_CMP_RAW + lane * nin;
    if (job.layout == QS_CMP_YCC) {
      uint8_t ycc[3];
      qc_rgb_ycc(s[0], s[1], s[2], ycc);
      px[0][r][lane] = ycc[0]; px[1][r][lane] = ycc[1]; px[2][r][lane] = ycc[2];
    } else if (job.layout == QS_CMP_RGB) {
      px[0][r][lane] = s[0]; px[1][r][lane] = s[1]; px[2][r][lane] = s[2];
    } else {
      px[0][r][lane] = s[0];
    }
  }
  __syncthreads();

  // phase 3: box downsampling of the two chroma planes (jcsample.c without fancy downsampling)
  const bool sub = nin == 3 && hs * vs > 1;
  const int cw = QS_CMP_TW / hs, chh = QS_CMP_TH / vs;     // chroma samples of the tile
  if (sub) {
    const int per = cw * chh;
    for (int i = lane; i < 2 * per; i += QS_CMP_LANES) {
      const int c = i / per, k = i - c * per, j = k / cw, x = k - j * cw;
      int sum = 0;
      for (int dy = 0; dy < vs; ++dy) {
        // the source row in the image, then in the tile: it lies in [Y0, Y0 + 16) (Y0 < H and Y0 is a multiple of vs)
        const int sy = min(max(qc_src_row(Y0 / vs + j, dy, H, vs, 1) - Y0, 0), QS_CMP_TH - 1);
        for (int dx = 0; dx < hs; ++dx) sum += px[1 + c][sy][x * hs + dx];
      }
      ds[c][j][x] = (uint8_t)qc_downsample(sum, hs, vs, x);     // (X0 / hs is even: the tile's x has the image's parity)
    }
  }
  __syncthreads();

  // phase 4: the blocks, eight at a time.  The list: 16 luma blocks (8 x 2), then per chroma component ncx x ncy.
  // Its length is a multiple of 8 in every supported layout -- 16 (gray), 24 (2x2, 4x1), 32 (2x1, 1x2), 48 (1x1) -- so
  // every lane has a block in every round and the barriers below are uniform.
  const int ncomp = nin;
  const int ncx = sub ? cw / 8 : 8, ncy = sub ? chh / 8 : 2, nc = ncx * ncy;
  const int nblocks = 16 + (ncomp - 1) * nc;
  const int slot = lane >> 3, k = lane & 7;
  for (int g0 = 0; g0 < nblocks; g0 += 8) {
    const int b = g0 + slot;
    int ci = 0, lbx, lby;                                  // component, block position inside the tile
    if (b < 16) { lbx = b & 7; lby = b >> 3; }
    else { const int kk = (b - 16) % nc; ci = 1 + (b - 16) / nc; lbx = kk % ncx; lby = kk / ncx; }
    {                                                      // pass 1: row k of the block
      const uint8_t* s = (ci && sub) ? &ds[ci - 1][lby * 8 + k][lbx * 8] : &px[ci][lby * 8 + k][lbx * 8];
      const uint2 v = *reinterpret_cast<const uint2*>(s);
      uint8_t smp[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) { smp[i] = (uint8_t)(v.x >> (8 * i)); smp[4 + i] = (uint8_t)(v.y >> (8 * i)); }
      int32_t d[8];
      qc_fdct_row(smp, d);
#pragma unroll
      for (int i = 0; i < 8; ++i) ws[slot * QS_CMP_WS + k * 9 + i] = d[i];
    }
    __syncthreads();
    {                                                      // pass 2: column k, quantised
      int32_t d[8], w[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) d[i] = ws[slot * QS_CMP_WS + i * 9 + k];
      qc_fdct_col(d, w);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        tr[slot * 64 + i * 8 + k] = qc_quant(w[i], job.q[ci][i * 8 + k], job.recip[ci][i * 8 + k]);
    }
    __syncthreads();
    {                                                      // row k of the block out: 16 bytes
      const int cwp = ci ? 8 * hs : 8, chp = ci ? 8 * vs : 8;        // pixels one block of this component covers
      const int bx = X0 / cwp + lbx, by = Y0 / chp + lby;
      const long long idx = (long long)by * job.stride[ci] + bx;
      if (bx < job.wib[ci] && by < job.hib[ci] && job.wib[ci] <= job.stride[ci] && idx < P.nblk[ci]) {
        const uint4 v = *reinterpret_cast<const uint4*>(&tr[slot * 64 + k * 8]);
        reinterpret_cast<uint4*>(P.coef[ci] + (size_t)idx * 64)[k] = v;
      }
    }
    __syncthreads();                                       // (the buffers are written again by the next eight)
  }
}

void qs_launch_compress(const QsCmpArgs& a, int tiles, hipStream_t s) {
  if (tiles > 0) hipLaunchKernelGGL(qs_compress_kernel, dim3(tiles), dim3(QS_CMP_LANES), 0, s, a);
}
