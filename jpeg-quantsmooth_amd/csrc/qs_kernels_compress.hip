// qs_kernels_compress.hip -- the kernel of the device compress (csrc/qs_compress_job.cpp,
// qs_hip_compress_device_batch): colour conversion, edge replication, chroma downsampling, forward DCT and quantisation
// exactly as libjpeg 9 does them with JDCT_ISLOW, for every job of a batch in ONE launch.  The chroma downsampling is
// the job's (QsCmpJob::mode, qc_chroma_shape): the box filter of do_fancy_downsampling = FALSE and the 8x8 DCT, or
// libjpeg 9's default, 2x chroma through jpeg_fdct_16x16 / _16x8 / _8x16 of the full-resolution samples.
//
// The decode's shape, reversed.  A workgroup (one wave) owns an input tile of QS_CMP_TW x QS_CMP_TH = 64 x 16 pixels of
// one job, a whole number of MCUs in every supported layout.
//   phase 1  the tile's 16 pixel rows into LDS, consecutive lanes on consecutive bytes (dwords where a row's first byte
//            is 4-byte aligned and the tile lies inside the image: 48 lanes per RGB row, 16 per gray row); rows and
//            columns beyond the image are replicated here, by address: a source column is min(x, W - 1), a source
//            row min(y, H - 1).
//   phase 2  one lane per column converts colour into three LDS planes (jccolor.c);
//   phase 3  subsampled chroma: box sums of the converted planes under libjpeg's two-step vertical edge rule
//            (qc_src_row: the last DOWNSAMPLED row is repeated, not the last pixel row).  In the DCT-scaled mode only
//            4x1 has a box left (h2v1, then the 16x8 DCT); every other layout skips the phase;
//   phase 4  the forward DCT, eight blocks at a time and EIGHT LANES PER BLOCK: lane k of a block runs row k's pass 1
//            from the plane, the rows meet in an LDS transpose (row stride 9 dwords: by construction, not by
//            measurement, each half-wave's 32 accesses fall into 32 different banks, writing and reading), lane k
//            runs column k's pass 2 and quantises its eight outputs, and a second LDS transpose hands lane k the
//            block's row k as 16 bytes.  Eight consecutive blocks of a block row are 1024 consecutive bytes of the
//            array: each store instruction writes them with consecutive lanes on consecutive 16 bytes.
//            A DCT-scaled chroma block reads 16x16, 16x8 or 8x16 samples: lane k runs rows k and k + 8 of pass 1 where
//            the block has 16 rows (a 16-point row pass where it has 16 columns), and column k of pass 2 over 8 or 16
//            rows.  The transpose keeps its row stride of 9; a block of 16 rows takes 168 dwords (16 x 9 = 144, padded
//            to 8 modulo 32 like the 72 of 8 rows, so that the half-wave's four blocks still start 8 banks apart).
//            Eight of those fill the raw-row bytes and the downsampled planes' bytes, which such a job does not use
//            (2x2 and 1x2 have no box), so the kernel's LDS does not grow: 8 448 bytes per wave in either mode.  The
//            second transpose then lies in the first one's bytes, behind one more barrier.
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
#define QS_CMP_WS16 168                  // ... of a job whose chroma blocks have 16 rows: 16 rows of 9, padded
#define QS_CMP_SCRATCH (8 * QS_CMP_WS * 4 + 8 * 128)       // the two transpose buffers: 3328 bytes

// the workgroup's LDS.  A struct: a job with 16-row blocks runs its transposes over scratch AND ds.
struct QsCmpLds {
  uint8_t scratch[QS_CMP_SCRATCH];       // raw rows (phases 1-2), then the two transpose buffers of phase 4
  uint8_t ds[2][QS_CMP_TH][QS_CMP_TW];   // downsampled chroma
  uint8_t px[3][QS_CMP_TH][QS_CMP_TW];   // converted samples, full resolution
};
static_assert(QS_CMP_TH * QS_CMP_RAW <= QS_CMP_SCRATCH, "the raw rows fit the bytes of the transpose buffers");
static_assert(8 * QS_CMP_WS16 * 4 <= QS_CMP_SCRATCH + 2 * QS_CMP_TH * QS_CMP_TW && 8 * 128 <= 8 * QS_CMP_WS16 * 4,
              "eight 16-row transposes fit scratch + ds, the second transpose fits the first");
static_assert(QS_CMP_SCRATCH % 16 == 0 && QS_CMP_WS16 % 32 == 8 && QS_CMP_WS % 32 == 8, "alignment, bank spread");

// a row of 8 / 16 samples from LDS (8- / 16-byte aligned)
__device__ inline void qs_cmp_row8(const uint8_t* s, uint8_t* smp) {
  const uint2 v = *reinterpret_cast<const uint2*>(s);
#pragma unroll
  for (int i = 0; i < 4; ++i) { smp[i] = (uint8_t)(v.x >> (8 * i)); smp[4 + i] = (uint8_t)(v.y >> (8 * i)); }
}
__device__ inline void qs_cmp_row16(const uint8_t* s, uint8_t* smp) {
  const uint4 v = *reinterpret_cast<const uint4*>(s);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    smp[i] = (uint8_t)(v.x >> (8 * i)); smp[4 + i] = (uint8_t)(v.y >> (8 * i));
    smp[8 + i] = (uint8_t)(v.z >> (8 * i)); smp[12 + i] = (uint8_t)(v.w >> (8 * i));
  }
}

// phase 4: the blocks, eight at a time.  The list: 16 luma blocks (8 x 2), then per chroma component ncx x ncy.
// Its length is a multiple of 8 in every supported layout and in both modes -- 16 (gray), 24 (2x2, 4x1), 32 (2x1,
// 1x2), 48 (1x1) -- so every lane has a block in every round and the barriers below are uniform; the 16 luma blocks
// are two whole rounds, so a round is all luma or all chroma.  SCALED: the job's chroma blocks take 16 samples one
// way or both (sh.dw, sh.dh); without it every block is 8x8 and the code is the box mode's alone.
template <bool SCALED>
__device__ __forceinline__ void qs_cmp_blocks(QsCmpLds& L, const QsCmpJob& job, const QsCmpPtrs& P, const QsCmpShape sh,
                                              const bool sub, const int cw, const int chh, const int X0, const int Y0,
                                              const int lane) {
  int32_t* const ws = reinterpret_cast<int32_t*>(L.scratch);                        // [8][wss]
  const int hs = job.hs, vs = job.vs;
  const int ncomp = job.layout == QS_CMP_GRAY ? 1 : 3;
  const int ncx = cw / sh.dw, ncy = chh / sh.dh, nc = ncx * ncy;
  const bool tall = SCALED && sh.dh == 16;                 // the job has blocks of 16 rows: the wide transposes
  const int wss = tall ? QS_CMP_WS16 : QS_CMP_WS;
  int16_t* const tr = reinterpret_cast<int16_t*>(tall ? L.scratch : L.scratch + 8 * QS_CMP_WS * 4);      // [8][64]
  const int nblocks = 16 + (ncomp - 1) * nc;
  const int slot = lane >> 3, k = lane & 7;
  for (int g0 = 0; g0 < nblocks; g0 += 8) {
    const int b = g0 + slot;
    int ci = 0, lbx, lby;                                  // component, block position inside the tile
    if (b < 16) { lbx = b & 7; lby = b >> 3; }
    else { const int kk = (b - 16) % nc; ci = 1 + (b - 16) / nc; lbx = kk % ncx; lby = kk / ncx; }
    // this round's blocks: 16 samples per row / 16 rows
    const bool wide = SCALED && ci && sh.dw == 16, high = SCALED && ci && sh.dh == 16;
    const uint8_t* plane = (ci && sub) ? &L.ds[ci - 1][0][0] : &L.px[ci][0][0];
    if (!wide && !high) {                                  // pass 1: row k of the block
      uint8_t smp[8];
      qs_cmp_row8(plane + (lby * 8 + k) * QS_CMP_TW + lbx * 8, smp);
      int32_t d[8];
      qc_fdct_row(smp, d);
#pragma unroll
      for (int i = 0; i < 8; ++i) ws[slot * wss + k * 9 + i] = d[i];
    } else {                                               // ... rows k and k + 8 of a block of 16 rows
      for (int row = k; row < (high ? 16 : 8); row += 8) {
        const uint8_t* s = plane + (lby * (high ? 16 : 8) + row) * QS_CMP_TW + lbx * (wide ? 16 : 8);
        int32_t d[8];
        if (wide) {
          uint8_t smp[16];
          qs_cmp_row16(s, smp);
          qc_fdct16_row(smp, d);
        } else {
          uint8_t smp[8];
          qs_cmp_row8(s, smp);
          qc_fdct_row(smp, d);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) ws[slot * wss + row * 9 + i] = d[i];
      }
    }
    __syncthreads();
    int32_t w[8];                                          // pass 2: column k
    if (high) {
      int32_t d[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) d[i] = ws[slot * wss + i * 9 + k];
      qc_fdct16_col(d, wide ? 2 : 1, w);
    } else {
      int32_t d[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) d[i] = ws[slot * wss + i * 9 + k];
      if (wide) qc_fdct_col_half(d, w); else qc_fdct_col(d, w);
    }
    if (tall) __syncthreads();                             // (uniform: tr lies in the bytes the columns were read from)
#pragma unroll
    for (int i = 0; i < 8; ++i)                            // ... quantised
      tr[slot * 64 + i * 8 + k] = qc_quant(w[i], job.q[ci][i * 8 + k], job.recip[ci][i * 8 + k]);
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

__global__ void __launch_bounds__(QS_CMP_LANES)
qs_compress_kernel(const QsCmpArgs a) {
  __shared__ __attribute__((aligned(16))) QsCmpLds L;
  uint8_t* const scratch = L.scratch;
  uint8_t (&px)[3][QS_CMP_TH][QS_CMP_TW] = L.px;
  uint8_t (&ds)[2][QS_CMP_TH][QS_CMP_TW] = L.ds;

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

  // phase 3: box downsampling of the two chroma planes (jcsample.c): the whole hs x vs in the box mode; in the
  // DCT-scaled mode what the scaled DCT leaves, the h2v1 box of 4x1 (bv = 1: its rows are the tile's, clamped in phase 1)
  QsCmpShape sh = {1, 1, 8, 8};
  if (nin == 3) sh = qc_chroma_shape(job.mode == QS_CMP_DS_DCT ? QS_CMP_DS_DCT : QS_CMP_DS_BOX, hs, vs);
  const int bh = sh.bh, bv = sh.bv;
  const bool sub = bh * bv > 1;
  const int cw = QS_CMP_TW / bh, chh = QS_CMP_TH / bv;     // chroma samples of the tile in front of the DCT
  if (sub) {
    const int per = cw * chh;
    for (int i = lane; i < 2 * per; i += QS_CMP_LANES) {
      const int c = i / per, k = i - c * per, j = k / cw, x = k - j * cw;
      int sum = 0;
      for (int dy = 0; dy < bv; ++dy) {
        // the source row in the image, then in the tile: it lies in [Y0, Y0 + 16) (Y0 < H and Y0 is a multiple of bv)
        const int sy = min(max(qc_src_row(Y0 / bv + j, dy, H, bv, 1) - Y0, 0), QS_CMP_TH - 1);
        for (int dx = 0; dx < bh; ++dx) sum += px[1 + c][sy][x * bh + dx];
      }
      ds[c][j][x] = (uint8_t)qc_downsample(sum, bh, bv, x);     // (X0 / bh is even: the tile's x has the image's parity)
    }
  }
  __syncthreads();

  // phase 4 (qs_cmp_blocks above).  A job whose chroma DCTs are all 8x8 -- the box mode, and the DCT-scaled mode of gray
  // and 1x1 -- runs the instantiation that has no 16-point code in it; the branch is the workgroup's
  if (sh.dw == 16 || sh.dh == 16) qs_cmp_blocks<true>(L, job, P, sh, sub, cw, chh, X0, Y0, lane);
  else qs_cmp_blocks<false>(L, job, P, sh, sub, cw, chh, X0, Y0, lane);
}

void qs_launch_compress(const QsCmpArgs& a, int tiles, hipStream_t s) {
  if (tiles > 0) hipLaunchKernelGGL(qs_compress_kernel, dim3(tiles), dim3(QS_CMP_LANES), 0, s, a);
}
