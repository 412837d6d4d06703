// qs_kernels_decode.hip -- the kernel of the device decode to pixels (csrc/qs_decode_job.cpp,
// qs_hip_decode_device_batch): dequantise, inverse DCT, chroma upsampling and colour conversion exactly as libjpeg 9
// does them with JDCT_ISLOW and its default settings -- or, job by job, as libjpeg-turbo does them (the triangle mode,
// below) -- for every job of a batch in ONE launch.
//
// A workgroup (one wave) owns an output tile of QS_DEC_TW x QS_DEC_TH = 64 x 16 pixels of one job, a whole number of
// MCUs in every supported layout.  Phase 1: one lane per 8x8 block the tile needs -- 16 luma blocks, and per chroma
// component the blocks whose scaled IDCT (libjpeg 9 upsamples 2x chroma by DCT scaling: jpeg_idct_16x16, _16x8, _8x16;
// 4:1:1 = 16x8 then 2x horizontal replication) covers the tile -- reads its 128 bytes, runs the IDCT in registers and
// writes the samples into LDS planes.  Phase 2: the lanes convert colour (jdcolor.c's integer tables, SCALEBITS 16)
// into an LDS copy of the tile's output rows.  Phase 3: the rows go out as consecutive bytes per lane (coalesced).
// Rows and columns beyond the image are neither computed into the output nor stored.
//
// Triangle mode (QS_DEC_UP_TRIANGLE): subsampled chroma goes through the 8x8 islow at its own
// resolution into the cpx planes -- the blocks under the tile plus one block of context on each side the filter reaches
// across, computed by lanes that idle in the dct mode -- and each lane then interpolates its pixel column with
// jdsample.c's triangle filters (qd_tri_column); the colour conversion takes turbo's green constant.  The two modes are
// two instantiations of one tile function behind a workgroup-uniform branch, so the dct mode's instructions are those
// it had before the triangle mode existed.
//
// Geometry and tables live in the caller's workspace (written by the prepare call); the arrays, the outputs and the
// output extent travel in the kernel arguments (QsDecArgs), one chunk of up to QS_DEC_CHUNK jobs per launch.
//
// Jobs at libjpeg 9's reduced sizes (scale_denom 2, 4, 8) have no tiles in this kernel's launch: they are decoded by
// qs_decode_scaled_kernel at the end of this file.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qs_decode.h"

#define QS_DEC_LANES 64

typedef uint8_t QsDecPlane[QS_DEC_TH][QS_DEC_TW];
typedef uint8_t QsDecRows[QS_DEC_TW * 3];
typedef uint8_t QsDecTriPlane[QS_DEC_TRI_H][QS_DEC_TRI_W];

template <bool TURBO>
__device__ __forceinline__ void qs_decode_tile(const QsDecJob& job, const QsDecPtrs& P, const QsDecGeom& g, int variant,
                                               int X0, int Y0, QsDecPlane* px, QsDecRows* rows, QsDecTriPlane* cpx) {
  const int width = min(job.width, P.width), height = min(job.height, P.height);
  const int lane = (int)threadIdx.x;

  // phase 1: 16 luma blocks, then nc blocks per chroma component.  Triangle mode on subsampled chroma: the blocks at
  // chroma resolution under the tile plus hx / hy blocks of context on each side, 8x8 islow into the cpx planes.
  const int ncomp = job.layout == QS_DEC_GRAY ? 1 : 3;
  const int cw = 8 * g.hs, ch = 8 * g.vs;                  // pixels one chroma block covers
  const bool tri = TURBO && ncomp == 3 && g.hs * g.vs > 1;
  const int hx = tri ? qd_tri_halo_x(g.hs) : 0, hy = tri ? qd_tri_halo_y(g.vs) : 0;
  const int shx = g.hs >> 1, shy = g.vs >> 1;              // log2 of the sampling factors (1, 2, 4: checked by the caller)
  const int Wc = (job.width + g.hs - 1) >> shx, Hc = (job.height + g.vs - 1) >> shy;   // chroma's downsampled size
  const int ncx = QS_DEC_TW / cw + 2 * hx, nc = ncx * (QS_DEC_TH / ch + 2 * hy);
  if (lane < 16 + (ncomp - 1) * nc) {
    int ci = 0, bx, by, x0, y0, kx = 0, ky = 0;
    if (lane < 16) {
      bx = (X0 >> 3) + (lane & 7); by = (Y0 >> 3) + (lane >> 3);
      x0 = (lane & 7) * 8; y0 = (lane >> 3) * 8;
    } else {
      const int k = (lane - 16) % nc;
      ci = 1 + (lane - 16) / nc;
      kx = k % ncx; ky = k / ncx;                          // the block in the plane; hx, hy: the tile's first own block
      bx = X0 / cw + kx - hx; by = Y0 / ch + ky - hy;
      x0 = (kx - hx) * cw; y0 = (ky - hy) * ch;
    }
    const bool tric = tri && ci;
    const int pw = ci && !TURBO ? cw : 8, ph = ci && !TURBO ? ch : 8;   // (TURBO: every block through the 8x8 islow)
    const int k = variant && ci ? 2 + ci : ci;
    const int16_t* base = P.coef[k];
    const bool needed = tric ? qd_tri_block_needed(bx, by, Wc, Hc) : X0 + x0 < width && Y0 + y0 < height;
    if (needed && bx < g.wblk[ci] && by < g.hblk[ci] && (long long)by * g.wblk[ci] + bx < P.nblk[k]) {
      const int16_t* src = base + ((size_t)by * g.wblk[ci] + bx) * 64;
      const uint4* s4 = reinterpret_cast<const uint4*>(src);
      const uint16_t* q = job.q[ci];
      int32_t dq[64];
#pragma unroll
      for (int v = 0; v < 8; ++v) {                        // the block's 128 bytes, 16 per load
        const uint4 w = s4[v];
        const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          dq[v * 8 + 2 * k] = (int32_t)(int16_t)(d[k] & 0xffff) * (int32_t)q[v * 8 + 2 * k];
          dq[v * 8 + 2 * k + 1] = ((int32_t)d[k] >> 16) * (int32_t)q[v * 8 + 2 * k + 1];
        }
      }
      uint8_t* dst = tric ? &cpx[ci - 1][ky * 8][kx * 8] : &px[ci][y0][x0];
      static_assert(QS_DEC_TRI_W == QS_DEC_TW, "one row stride for the IDCT's destination");
      if (pw == 8 && ph == 8) qd_idct_block<false, false>(dq, dst, QS_DEC_TW);
      else if (pw == 16 && ph == 16) qd_idct_block<true, true>(dq, dst, QS_DEC_TW);
      else if (pw == 16 && ph == 8) qd_idct_block<true, false>(dq, dst, QS_DEC_TW);
      else if (pw == 8 && ph == 16) qd_idct_block<false, true>(dq, dst, QS_DEC_TW);
      else qd_idct_block<true, false, 2>(dq, dst, QS_DEC_TW);     // 32 x 8: 4:1:1
    }
  }
  __syncthreads();

  const int w = min(QS_DEC_TW, width - X0), h = min(QS_DEC_TH, height - Y0);
  // triangle mode: each lane interpolates its pixel column of both chroma components out of the cpx planes into px
  // (read back below by the same lane only)
  if (tri && lane < w) {
#pragma unroll
    for (int ci = 1; ci < 3; ++ci)
      qd_tri_column_any(g.hs, g.vs, &cpx[ci - 1][0][0], QS_DEC_TRI_W, (X0 >> shx) - 8 * hx, (Y0 >> shy) - 8 * hy, Wc, Hc,
                        X0 + lane, Y0, &px[ci][0][lane], QS_DEC_TW);
  }

  // phase 2: colour conversion into the output rows (jdcolor.c: ycc_rgb_convert, rgb_convert, grayscale_convert)
  for (int r = 0; r < h; ++r) {
    if (lane >= w) break;
    if (job.layout == QS_DEC_YCC) {
      if (TURBO) qd_ycc_rgb_turbo(px[0][r][lane], px[1][r][lane], px[2][r][lane], &rows[r][lane * 3]);
      else qd_ycc_rgb(px[0][r][lane], px[1][r][lane], px[2][r][lane], &rows[r][lane * 3]);
    } else if (job.layout == QS_DEC_RGB) {
      rows[r][lane * 3] = px[0][r][lane];
      rows[r][lane * 3 + 1] = px[1][r][lane];
      rows[r][lane * 3 + 2] = px[2][r][lane];
    } else {
      rows[r][lane] = px[0][r][lane];
    }
  }
  __syncthreads();

  // phase 3: the rows out, consecutive lanes on consecutive bytes
  const int nb = w * job.nout;
  for (int r = 0; r < h; ++r) {
    uint8_t* out = P.out + (size_t)(Y0 + r) * P.pitch + (size_t)X0 * job.nout;
    for (int b = lane; b < nb; b += QS_DEC_LANES) out[b] = rows[r][b];
  }
}

// three waves per SIMD, as before the triangle mode: at most 168 VGPRs (the build's --no-scratch check catches a spill)
__global__ void __launch_bounds__(QS_DEC_LANES) __attribute__((amdgpu_waves_per_eu(3)))
qs_decode_kernel(const QsDecArgs a) {
  __shared__ uint8_t px[3][QS_DEC_TH][QS_DEC_TW];          // component samples of the tile
  __shared__ uint8_t rows[QS_DEC_TH][QS_DEC_TW * 3];        // the tile's output rows
  __shared__ uint8_t cpx[2][QS_DEC_TRI_H][QS_DEC_TRI_W];    // triangle mode: chroma at its own resolution, with context
  const QsDecJob* J = a.jobs;
  const int tile = (int)blockIdx.x;
  int lo = 0, hi = a.n - 1;                                // the job whose tiles hold this workgroup
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (J[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  const QsDecJob& job = J[lo];
  const int t = tile - job.tile0;
  if (t < 0 || t >= job.tiles) return;
  const int X0 = (t % job.tiles_x) * QS_DEC_TW, Y0 = (t / job.tiles_x) * QS_DEC_TH;
  const QsDecPtrs& P = a.p[lo];
  const int variant = job.two && a.d_stop && a.d_stop[a.job0 + lo] != 0 ? 1 : 0;
  const QsDecGeom& g = job.g[variant];
  if ((g.hs != 1 && g.hs != 2 && g.hs != 4) || (g.vs != 1 && g.vs != 2) || g.hs * g.vs > 4) return;   // (never prepared)
  if (job.upsampling == QS_DEC_UP_TRIANGLE) qs_decode_tile<true>(job, P, g, variant, X0, Y0, px, rows, cpx);
  else qs_decode_tile<false>(job, P, g, variant, X0, Y0, px, rows, cpx);
}

void qs_launch_decode(const QsDecArgs& a, int tiles, hipStream_t s) {
  if (tiles > 0) hipLaunchKernelGGL(qs_decode_kernel, dim3(tiles), dim3(QS_DEC_LANES), 0, s, a);
}

// The reduced sizes (scale_denom 2, 4, 8): a kernel of its own, so the full-size one keeps its
// instructions.  A workgroup (one wave) owns QS_DEC_TW x QS_DEC_TH OUTPUT samples of one job with m < 8, i.e. 64 / m x
// 16 / m luma blocks and the chroma blocks over them; libjpeg 9 sizes each component's IDCT so that none is upsampled
// (qs_decode.h).  Phase 1: the lanes walk the tile's blocks (qd_scaled_item), consecutive lanes on consecutive blocks
// of a block row; each reads the top-left PW x PH coefficients of its block and nothing else.  Phases 2 and 3 as above.
__global__ void __launch_bounds__(QS_DEC_LANES) __attribute__((amdgpu_waves_per_eu(3)))
qs_decode_scaled_kernel(const QsDecArgs a) {
  __shared__ uint8_t px[3 * QS_DEC_TH * QS_DEC_TW];        // component samples of the tile
  __shared__ uint8_t rows[QS_DEC_TH * QS_DEC_TW * 3];       // the tile's output rows
  const QsDecJob* J = a.jobs;
  const int tile = (int)blockIdx.x;
  int lo = 0, hi = a.n - 1;                                // the job whose tiles hold this workgroup
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.p[mid].stile0 <= tile) lo = mid; else hi = mid - 1;
  }
  const QsDecJob& job = J[lo];
  const QsDecPtrs& P = a.p[lo];
  const int m = qd_job_m(job);
  if (m != 1 && m != 2 && m != 4) return;                  // a full-size job (the other kernel's), or never prepared
  if (job.width < 1 || job.height < 1 || job.width > 65500 || job.height > 65500) return;
  const int stiles_x = (job.width + QS_DEC_TW - 1) / QS_DEC_TW, stiles = stiles_x * ((job.height + QS_DEC_TH - 1) / QS_DEC_TH);
  const int t = tile - P.stile0;
  if (t < 0 || t >= stiles) return;
  const int X0 = (t % stiles_x) * QS_DEC_TW, Y0 = (t / stiles_x) * QS_DEC_TH;
  const int variant = job.two && a.d_stop && a.d_stop[a.job0 + lo] != 0 ? 1 : 0;
  const QsDecGeom& g = job.g[variant];
  if ((g.hs != 1 && g.hs != 2 && g.hs != 4) || (g.vs != 1 && g.vs != 2) || g.hs * g.vs > 4) return;
  const int width = min(job.width, P.width), height = min(job.height, P.height);
  if ((job.nout != 1 && job.nout != 3) || P.pitch < (int64_t)width * job.nout) return;   // (a run that does not match the prepare)
  const int lane = (int)threadIdx.x;

  const int items = qd_scaled_items(job, g, m);
  for (int it = lane; it < items; it += QS_DEC_LANES) qd_scaled_item(job, P, g, variant, m, width, height, X0, Y0, it, px);
  __syncthreads();

  const int w = min(QS_DEC_TW, width - X0), h = min(QS_DEC_TH, height - Y0);
  if (lane < w)
    for (int r = 0; r < h; ++r) qd_scaled_convert(job, px, r, lane, rows);
  __syncthreads();

  const int nb = w * job.nout;
  for (int r = 0; r < h; ++r) {
    uint8_t* out = P.out + (size_t)(Y0 + r) * P.pitch + (size_t)X0 * job.nout;
    for (int b = lane; b < nb; b += QS_DEC_LANES) out[b] = rows[r * QS_DEC_TW * 3 + b];
  }
}

void qs_launch_decode_scaled(const QsDecArgs& a, int tiles, hipStream_t s) {
  if (tiles > 0) hipLaunchKernelGGL(qs_decode_scaled_kernel, dim3(tiles), dim3(QS_DEC_LANES), 0, s, a);
}
