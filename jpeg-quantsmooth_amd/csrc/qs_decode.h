// qs_decode.h -- the device decode to pixels (qs_hip_decode_device_batch, csrc/qs_kernels_decode.hip): libjpeg 9's
// JDCT_ISLOW inverse DCTs (jidctint.c: jpeg_idct_islow, jpeg_idct_16x16, jpeg_idct_16x8, jpeg_idct_8x16), its range
// limit and its YCbCr -> RGB tables (jdcolor.c), as functions the kernel and a host build can both compile, and the
// per-job descriptor the host driver writes into the caller's workspace.
//
// Numerical contract: libjpeg 9's INT32 is `long` (64 bits) and its workspace between the two
// passes is `int`.  Both passes are linear in their inputs up to their one final right shift, so
//   pass 1: ws = (int32)((sum + 2^10) >> 11)  needs bits 11..42 of the sum: 64-bit arithmetic (an int32 product
//           coef * q times a 14-bit constant exceeds 32 bits);
//   pass 2: sample = limit[((sum + bias) >> 18) & 1023] needs bits 18..27 of the sum only, i.e. the sum modulo 2^28:
//           wrapping 32-bit arithmetic gives exactly those bits, whatever the size of the true sum.
// Pass 1 runs in wrapping 32 bits where the block's dequantised values are bounded so that its final sums fit int32
// (QS_DEC_FAST_BOUND), in 64 bits otherwise.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define QS_DEC_HD __host__ __device__ inline
#define QS_DEC_HDF __host__ __device__ __forceinline__   // (the scaled kernel's functions: no calls, no stack)
#define QD_UNROLL _Pragma("unroll")
#else
#define QS_DEC_HD static inline
#define QS_DEC_HDF static inline
#define QD_UNROLL
#endif

enum {                           // the supported layouts (qs_hip_decode_device_batch_info)
  QS_DEC_GRAY = 0,               // one component, any sampling: 8x8 islow
  QS_DEC_YCC = 1,                // YCbCr -> RGB, chroma 1x1, luma (h, v) in {(1,1), (2,1), (1,2), (2,2), (4,1)}
  QS_DEC_RGB = 2                 // RGB without a colour transform, same sampling set, no conversion
};

enum {                           // chroma upsampling (qs_hip_decode_opts: QS_HIP_UPSAMPLE_*)
  QS_DEC_UP_DCT = 0,             // libjpeg 7..9: the scaled IDCTs below
  QS_DEC_UP_TRIANGLE = 1         // libjpeg-turbo / 6b: 8x8 islow at chroma resolution, then jdsample.c's triangle filters
};

// One job as the kernel sees it (workspace, written by the prepare call): geometry and tables, no addresses.  Two
// geometries when the job carries UPSAMPLE_UV's replacement chroma: variant 0 = the replacement chroma at luma
// resolution (taken when d_stop[job] reads 0), variant 1 = the original chroma and sampling (reference :2835).
struct QsDecGeom {
  int32_t wblk[3], hblk[3];      // each component's block array (wblk = row stride in blocks)
  int32_t hs, vs;                // component 0's sampling factors (chroma is 1x1); 1x1 for gray
};

struct QsDecJob {
  QsDecGeom g[2];
  int32_t width, height;         // output crop
  int32_t layout, nout;          // QS_DEC_*, output samples per pixel (1 or 3)
  int16_t two;                   // 1: the variant follows d_stop[job] (else variant 0)
  int16_t upsampling;            // QS_DEC_UP_*: how subsampled chroma reaches luma resolution (the record keeps its size)
  int32_t tiles_x;               // output tiles of QS_DEC_TW x QS_DEC_TH pixels per tile row
  int32_t tile0, tiles;          // first workgroup of this job in its chunk's launch, and how many it has
  uint16_t q[3][64];             // the components' tables (natural order)
};
// The reduced sizes (section 12.2) keep the record's size: a job at scale_denom 2, 4 or 8 carries the denominator in the
// high byte of `upsampling` (QS_DEC_UP_DCT + 256 * scale_denom), width x height are its scaled output, and tiles == 0 --
// the full-size kernel, which reads `upsampling` only for a job with tiles, steps over it.  The scaled kernel derives the
// job's tiles from width x height and takes the job's first workgroup from the kernel arguments (QsDecPtrs::stile0).

// What addresses caller memory travels in the kernel arguments of the run call, one chunk of jobs per launch, so the
// kernel bounds every access by them (a workspace that does not match the run gives wrong pixels, never a stray
// address: the output extent comes from here too).
#define QS_DEC_CHUNK 44            // jobs per launch (about 3.8 KiB of kernel arguments)
struct QsDecPtrs {
  const int16_t* coef[5];        // 0..2 variant 0's arrays; 3..4 variant 1's chroma (luma is coef[0] in both)
  uint8_t* out;
  int64_t pitch;
  int32_t width, height;         // the output extent the caller gave
  int32_t nblk[5];               // blocks in each array
  int32_t stile0;                // first workgroup of this job in the chunk's scaled launch (the full-size kernel ignores it)
};
struct QsDecArgs {
  const QsDecJob* jobs;          // the chunk's descriptors (workspace)
  const int32_t* d_stop;         // the caller's int32[njobs] or null, indexed by job0 + i
  int32_t job0, n;
  QsDecPtrs p[QS_DEC_CHUNK];
};

#define QS_DEC_TW 64             // output tile: 64 x 16 pixels = every MCU shape of the supported layouts
#define QS_DEC_TH 16

// 14-bit fixed-point constants of jidctint.c (CONST_BITS 13): FIX(x) = (INT32)(x * 8192 + 0.5)
#define QD_FIX(x) ((int32_t)((x) * 8192 + 0.5))

// One 8-point column / row of jpeg_idct_islow.  in[k] = input k (already dequantised for pass 1); dc_bias is added
// to in[0] << 13.  out[i] = the sum before the final shift.  T: int64_t (pass 1) or uint32_t (wrapping; pass 2 and
// the bounded pass 1).
template <class T>
QS_DEC_HD void qd_idct8(const T* in, T dc_bias, T* out) {
  T z2 = in[0], z3 = in[4];
  z2 = (T)(z2 << 13) + dc_bias;
  z3 = (T)(z3 << 13);
  T tmp0 = z2 + z3, tmp1 = z2 - z3;
  z2 = in[2]; z3 = in[6];
  T z1 = (z2 + z3) * (T)QD_FIX(0.541196100);
  T tmp2 = z1 + z2 * (T)QD_FIX(0.765366865);
  T tmp3 = z1 - z3 * (T)QD_FIX(1.847759065);
  const T tmp10 = tmp0 + tmp2, tmp13 = tmp0 - tmp2, tmp11 = tmp1 + tmp3, tmp12 = tmp1 - tmp3;
  tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
  z2 = tmp0 + tmp2;
  z3 = tmp1 + tmp3;
  z1 = (z2 + z3) * (T)QD_FIX(1.175875602);
  z2 = z2 * (T)(-QD_FIX(1.961570560));
  z3 = z3 * (T)(-QD_FIX(0.390180644));
  z2 += z1;
  z3 += z1;
  z1 = (tmp0 + tmp3) * (T)(-QD_FIX(0.899976223));
  tmp0 = tmp0 * (T)QD_FIX(0.298631336);
  tmp3 = tmp3 * (T)QD_FIX(1.501321110);
  tmp0 += z1 + z2;
  tmp3 += z1 + z3;
  z1 = (tmp1 + tmp2) * (T)(-QD_FIX(2.562915447));
  tmp1 = tmp1 * (T)QD_FIX(2.053119869);
  tmp2 = tmp2 * (T)QD_FIX(3.072711026);
  tmp1 += z1 + z3;
  tmp2 += z1 + z2;
  out[0] = tmp10 + tmp3; out[7] = tmp10 - tmp3;
  out[1] = tmp11 + tmp2; out[6] = tmp11 - tmp2;
  out[2] = tmp12 + tmp1; out[5] = tmp12 - tmp1;
  out[3] = tmp13 + tmp0; out[4] = tmp13 - tmp0;
}

// One 16-point column / row of jpeg_idct_16x16 (8 inputs, 16 outputs), same conventions.
template <class T>
QS_DEC_HD void qd_idct16(const T* in, T dc_bias, T* out) {
  T tmp0 = (T)(in[0] << 13) + dc_bias;
  T z1 = in[4];
  T tmp1 = z1 * (T)QD_FIX(1.306562965);
  T tmp2 = z1 * (T)QD_FIX(0.541196100);
  T tmp10 = tmp0 + tmp1, tmp11 = tmp0 - tmp1, tmp12 = tmp0 + tmp2, tmp13 = tmp0 - tmp2;
  z1 = in[2];
  T z2 = in[6];
  T z3 = z1 - z2;
  T z4 = z3 * (T)QD_FIX(0.275899379);
  z3 = z3 * (T)QD_FIX(1.387039845);
  tmp0 = z3 + z2 * (T)QD_FIX(2.562915447);
  tmp1 = z4 + z1 * (T)QD_FIX(0.899976223);
  tmp2 = z3 - z1 * (T)QD_FIX(0.601344887);
  T tmp3 = z4 - z2 * (T)QD_FIX(0.509795579);
  const T tmp20 = tmp10 + tmp0, tmp27 = tmp10 - tmp0, tmp21 = tmp12 + tmp1, tmp26 = tmp12 - tmp1;
  const T tmp22 = tmp13 + tmp2, tmp25 = tmp13 - tmp2, tmp23 = tmp11 + tmp3, tmp24 = tmp11 - tmp3;
  z1 = in[1]; z2 = in[3]; z3 = in[5]; z4 = in[7];
  tmp11 = z1 + z3;
  tmp1 = (z1 + z2) * (T)QD_FIX(1.353318001);
  tmp2 = tmp11 * (T)QD_FIX(1.247225013);
  tmp3 = (z1 + z4) * (T)QD_FIX(1.093201867);
  tmp10 = (z1 - z4) * (T)QD_FIX(0.897167586);
  tmp11 = tmp11 * (T)QD_FIX(0.666655658);
  tmp12 = (z1 - z2) * (T)QD_FIX(0.410524528);
  tmp0 = tmp1 + tmp2 + tmp3 - z1 * (T)QD_FIX(2.286341144);
  tmp13 = tmp10 + tmp11 + tmp12 - z1 * (T)QD_FIX(1.835730603);
  z1 = (z2 + z3) * (T)QD_FIX(0.138617169);
  tmp1 += z1 + z2 * (T)QD_FIX(0.071888074);
  tmp2 += z1 - z3 * (T)QD_FIX(1.125726048);
  z1 = (z3 - z2) * (T)QD_FIX(1.407403738);
  tmp11 += z1 - z3 * (T)QD_FIX(0.766367282);
  tmp12 += z1 + z2 * (T)QD_FIX(1.971951411);
  z2 += z4;
  z1 = z2 * (T)(-QD_FIX(0.666655658));
  tmp1 += z1;
  tmp3 += z1 + z4 * (T)QD_FIX(1.065388962);
  z2 = z2 * (T)(-QD_FIX(1.247225013));
  tmp10 += z2 + z4 * (T)QD_FIX(3.141271809);
  tmp12 += z2;
  z2 = (z3 + z4) * (T)(-QD_FIX(1.353318001));
  tmp2 += z2;
  tmp3 += z2;
  z2 = (z4 - z3) * (T)QD_FIX(0.410524528);
  tmp10 += z2;
  tmp11 += z2;
  out[0] = tmp20 + tmp0;  out[15] = tmp20 - tmp0;
  out[1] = tmp21 + tmp1;  out[14] = tmp21 - tmp1;
  out[2] = tmp22 + tmp2;  out[13] = tmp22 - tmp2;
  out[3] = tmp23 + tmp3;  out[12] = tmp23 - tmp3;
  out[4] = tmp24 + tmp10; out[11] = tmp24 - tmp10;
  out[5] = tmp25 + tmp11; out[10] = tmp25 - tmp11;
  out[6] = tmp26 + tmp12; out[9] = tmp26 - tmp12;
  out[7] = tmp27 + tmp13; out[8] = tmp27 - tmp13;
}

// libjpeg 9's IDCT range limit (jdct.h: RANGE_CENTER 512, RANGE_SUBSET 384, RANGE_MASK 1023; jdmaster.c:
// prepare_range_limit_table): index x = (v + 512) & 1023 of the descaled value v; limit[x] = clamp(x - 384, 0, 255).
// The +512 is folded into pass 2's bias, so x arrives here already masked.
QS_DEC_HD uint8_t qd_limit(uint32_t x) {
  const int v = (int)(x & 1023) - 384;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// pass-2 bias, added to in[0] << 13: (RANGE_CENTER << (PASS1_BITS + 3)) + (1 << (PASS1_BITS + 2)), then << 13
#define QD_PASS2_BIAS ((uint32_t)((512u << 5) + (1u << 4)) << 13)

// Pass 1 in wrapping 32-bit arithmetic is exact whenever its final sums fit int32: additions and products modulo 2^32
// agree with the true ones modulo 2^32, and a sum in [-2^31, 2^31) is its own residue.  Each final sum is
// sum_k M[i][k] * dq[k] + 2^10 with integer weights |M[i][k]| <= 2^13 * sqrt(2) * 1.0004 < 11590 (the composed FIX()
// constants of the 8- and 16-point kernels), so |sum| <= 8 * 11590 * max|dq| + 2^10 < 2^31 for max|dq| <= 23000.
// QS_DEC_FAST_BOUND takes 2^14; blocks above it take the 64-bit pass 1.
#define QS_DEC_FAST_BOUND 16384

// DEQUANTIZE of jidctint.c: an int product (|coef * q| <= 32768 * 65535 < 2^31, never overflows)
QS_DEC_HD void qd_dequant(const int16_t* coef, const uint16_t* q, int32_t* dq) {
  for (int i = 0; i < 64; ++i) dq[i] = (int32_t)coef[i] * (int32_t)q[i];
}

// One block of dequantised values dq: IDCT to rows x cols samples into dst (row stride `stride`).
// W16: 16-point row pass (16 columns out), H16: 16-point column pass (16 rows out); XREP: each output column written
// XREP times (2: libjpeg's h2v1 replication after a 16x8 IDCT, 4:1:1 chroma).
template <bool W16, bool H16, int XREP = 1>
QS_DEC_HD void qd_idct_block(const int32_t* dq, uint8_t* dst, int stride) {
  constexpr int R = H16 ? 16 : 8, Cn = W16 ? 16 : 8;
  int32_t ws[R * 8];                       // libjpeg's `int workspace[8 * R]`, here [row][col]
  int32_t mx = 0;
  QD_UNROLL
  for (int i = 0; i < 64; ++i) {
    const int32_t a = dq[i] < 0 ? -dq[i] : dq[i];        // (-32768 * 65535 > INT32_MIN: no overflow in the negation)
    mx = a > mx ? a : mx;
  }
  const bool fast = mx <= QS_DEC_FAST_BOUND;
  QD_UNROLL
  for (int c = 0; c < 8; ++c) {                          // pass 1: columns
    if (fast) {
      uint32_t in[8], o[16];
      QD_UNROLL
  for (int k = 0; k < 8; ++k) in[k] = (uint32_t)dq[k * 8 + c];
      if (H16) qd_idct16<uint32_t>(in, 1u << 10, o); else qd_idct8<uint32_t>(in, 1u << 10, o);
      QD_UNROLL
  for (int r = 0; r < R; ++r) ws[r * 8 + c] = (int32_t)o[r] >> 11;
    } else {
      int64_t in[8], o[16];
      QD_UNROLL
  for (int k = 0; k < 8; ++k) in[k] = dq[k * 8 + c];
      if (H16) qd_idct16<int64_t>(in, (int64_t)1 << 10, o); else qd_idct8<int64_t>(in, (int64_t)1 << 10, o);
      QD_UNROLL
  for (int r = 0; r < R; ++r) ws[r * 8 + c] = (int32_t)(o[r] >> 11);   // (int) of libjpeg's INT32: wraps
    }
  }
  QD_UNROLL
  for (int r = 0; r < R; ++r) {                          // pass 2: rows, modulo 2^32
    uint32_t in[8], o[16];
    QD_UNROLL
  for (int k = 0; k < 8; ++k) in[k] = (uint32_t)ws[r * 8 + k];
    if (W16) qd_idct16<uint32_t>(in, QD_PASS2_BIAS, o); else qd_idct8<uint32_t>(in, QD_PASS2_BIAS, o);
    QD_UNROLL
  for (int c = 0; c < Cn; ++c) {
      const uint8_t v = qd_limit(o[c] >> 18);
      QD_UNROLL
  for (int k = 0; k < XREP; ++k) dst[r * stride + c * XREP + k] = v;
    }
  }
}

// jdcolor.c (libjpeg 9, JCS_YCbCr): SCALEBITS 16, tables over the 256 chroma values
#define QD_ONE_HALF (1 << 15)
QS_DEC_HD int32_t qd_fix16(double x) { return (int32_t)(x * 65536.0 + 0.5); }
// cb_g: the constant of the Cb -> G table, the one entry in which the libraries differ (below)
QS_DEC_HD void qd_ycc_rgb_g(int y, int cb, int cr, int32_t cb_g, uint8_t* out) {
  const int xb = cb - 128, xr = cr - 128;
  // (INT32 arithmetic: the products stay far below 2^31)
  const int crr = (int)((qd_fix16(1.402) * xr + QD_ONE_HALF) >> 16);
  const int cbb = (int)((qd_fix16(1.772) * xb + QD_ONE_HALF) >> 16);
  const int g = (int)((-qd_fix16(0.714136286) * xr + (-cb_g * xb + QD_ONE_HALF)) >> 16);
  auto lim = [](int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); };   // sample_range_limit
  out[0] = lim(y + crr);
  out[1] = lim(y + g);
  out[2] = lim(y + cbb);
}
// libjpeg 9 builds its tables from nine-digit constants, libjpeg-turbo and 6b from five-digit ones: FIX(1.40200),
// FIX(1.77200) and FIX(0.71414) = FIX(0.714136286) = 46802 come out the same, FIX(0.34414) = 22554 does not
// (FIX(0.344136286) = 22553), so turbo's green is one lower on a few (Cb, Cr) pairs.
#define QD_CB_G_V9 22553
#define QD_CB_G_TURBO 22554
QS_DEC_HD void qd_ycc_rgb(int y, int cb, int cr, uint8_t* out) { qd_ycc_rgb_g(y, cb, cr, QD_CB_G_V9, out); }
QS_DEC_HD void qd_ycc_rgb_turbo(int y, int cb, int cr, uint8_t* out) { qd_ycc_rgb_g(y, cb, cr, QD_CB_G_TURBO, out); }

// ---- triangle-filter chroma upsampling (libjpeg-turbo / libjpeg 6b, jdsample.c) ---------------
// A 2x-subsampled chroma component goes through the 8x8 islow at its own resolution and is then interpolated:
//   2x1 (h2v1_fancy_upsample)  out[y][x] = (3 c[y][x>>1] + c[y][x even ? (x>>1)-1 : (x>>1)+1] + (x even ? 1 : 2)) >> 2
//   1x2 (h1v2_fancy_upsample)  out[y][x] = (3 c[y>>1][x] + c[y even ? (y>>1)-1 : (y>>1)+1][x] + (y even ? 1 : 2)) >> 2
//   2x2 (h2v2_fancy_upsample)  s[y][i] = 3 c[y>>1][i] + c[y even ? (y>>1)-1 : (y>>1)+1][i],
//                              out[y][x] = (3 s[y][x>>1] + s[y][x even ? (x>>1)-1 : (x>>1)+1] + (x even ? 8 : 7)) >> 4
// with every index clamped to the component's downsampled size Wc x Hc = ceil(width / hs) x ceil(height / vs) -- not to
// the block grid: the IDCT's own samples beyond Wc / Hc never reach a pixel.  The horizontal filters are taken only
// when Wc > 2 (jdsample.c: downsampled_width > 2); a narrower plane is replicated 2x horizontally, and for 2x2 also
// vertically (h2v2_upsample).  4x1 has no filter: each sample four times (int_upsample).
//
// A tile holds each chroma component as a plane of blocks at chroma resolution: the blocks under its own
// QS_DEC_TW x QS_DEC_TH pixels plus one block of context on each side the filter reaches across (left and right for
// hs == 2, above and below for vs == 2).
QS_DEC_HD int qd_tri_halo_x(int hs) { return hs == 2 ? 1 : 0; }      // context blocks on each side
QS_DEC_HD int qd_tri_halo_y(int vs) { return vs == 2 ? 1 : 0; }
#define QS_DEC_TRI_W 64          // the plane: at most 8 x 3 blocks (1x2), 6 x 3 (2x2), 6 x 2 (2x1), 2 x 2 (4x1)
#define QS_DEC_TRI_H 24

QS_DEC_HD int qd_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// One output column of a tile: the QS_DEC_TH samples of pixel column x, rows y0 .. y0 + QS_DEC_TH - 1 (y0 a multiple of
// QS_DEC_TH), into out[r * ostride].  c: the component's plane, row stride `stride`, whose sample (0, 0) is sample
// (ox, oy) of the component (negative at the image's left / top tiles); it must hold every sample (cx, cy) with
// cx in {x / HS - 1, x / HS, x / HS + 1} and cy in y0 / VS - 1 .. (y0 + QS_DEC_TH) / VS after the clamp to
// [0, Wc - 1] x [0, Hc - 1] -- nothing else is read.  Requires x / HS < Wc and y0 / VS < Hc.  Rows beyond the image
// come out as the clamp gives them; the caller drops them.
template <int HS, int VS>
QS_DEC_HD void qd_tri_column(const uint8_t* c, int stride, int ox, int oy, int Wc, int Hc, int x, int y0, uint8_t* out,
                             int ostride) {
  constexpr int NR = QS_DEC_TH / VS;                       // chroma rows under the tile's rows
  const bool fh = HS == 2 && Wc > 2;                       // the horizontal triangle filter
  const int odd = x & 1;
  const int cx = x / HS;
  const int cxn = fh ? qd_clampi(odd ? cx + 1 : cx - 1, 0, Wc - 1) : cx;
  const int cy0 = y0 / VS;
  int t[NR + 2];                                           // rows cy0 - 1 .. cy0 + NR: 3 c[cx] + c[cxn] (fh), else c[cx]
  QD_UNROLL
  for (int j = (VS == 2 ? 0 : 1); j < (VS == 2 ? NR + 2 : NR + 1); ++j) {
    const uint8_t* row = c + (qd_clampi(cy0 - 1 + j, 0, Hc - 1) - oy) * stride - ox;
    t[j] = fh ? 3 * (int)row[cx] + (int)row[cxn] : (int)row[cx];
  }
  QD_UNROLL
  for (int r = 0; r < QS_DEC_TH; ++r) {
    int v;
    if (VS == 2) {
      const int j = 1 + (r >> 1), jn = (r & 1) ? j + 1 : j - 1;
      if (HS == 1) v = (3 * t[j] + t[jn] + ((r & 1) ? 2 : 1)) >> 2;
      else if (fh) v = (3 * t[j] + t[jn] + (odd ? 7 : 8)) >> 4;
      else v = t[j];
    } else {
      v = fh ? (t[1 + r] + (odd ? 2 : 1)) >> 2 : t[1 + r];
    }
    out[r * ostride] = (uint8_t)v;
  }
}

// qd_tri_column for a job's sampling (hs, vs) in {(2, 1), (1, 2), (2, 2), (4, 1)}
QS_DEC_HD void qd_tri_column_any(int hs, int vs, const uint8_t* c, int stride, int ox, int oy, int Wc, int Hc, int x,
                                 int y0, uint8_t* out, int ostride) {
  if (hs == 2 && vs == 2) qd_tri_column<2, 2>(c, stride, ox, oy, Wc, Hc, x, y0, out, ostride);
  else if (hs == 2) qd_tri_column<2, 1>(c, stride, ox, oy, Wc, Hc, x, y0, out, ostride);
  else if (vs == 2) qd_tri_column<1, 2>(c, stride, ox, oy, Wc, Hc, x, y0, out, ostride);
  else qd_tri_column<4, 1>(c, stride, ox, oy, Wc, Hc, x, y0, out, ostride);
}

// Whether block (bx, by) of a chroma component is one a tile's plane must hold: it lies in the component and carries at
// least one sample inside the downsampled size (every clamped index falls into such a block).
QS_DEC_HD bool qd_tri_block_needed(int bx, int by, int Wc, int Hc) {
  return bx >= 0 && by >= 0 && bx * 8 < Wc && by * 8 < Hc;
}

// ---- libjpeg 9's reduced sizes: scale_denom 2, 4, 8 ------------------------------------------
// With scale 1/N a luma block gives M x M samples (M = 8 / N) and libjpeg 9 picks each component's IDCT so that no
// upsampling is left (jdmaster.c: DCT_h_scaled_size x DCT_v_scaled_size; 4x1 keeps its 2x replication):
//   luma / gray / 1x1 chroma  M x M          jpeg_idct_4x4, _2x2, _1x1
//   2x2 chroma                2M x 2M        jpeg_idct_islow (8x8), _4x4, _2x2
//   2x1 chroma                2M x M         jpeg_idct_8x4, _4x2, _2x1      (names are width x height)
//   1x2 chroma                M x 2M         jpeg_idct_4x8, _2x4, _1x2
//   4x1 chroma                2M x M, each column twice
// A PW x PH IDCT reads the block's top-left PW columns x PH rows and nothing else.
//
// Numerical contract, function by function (INT32 is long, DEQUANTIZE an int product):
//   4x4, 8x4  pass 1 (4-point columns): ws = (int)(((a +- b) << 2) + ((odd + 2^10) >> 11)), odd the c2 / c6 rotation of
//             rows 1 and 3.  The even term is linear, so its low 32 bits are those of the wrapping form; the odd term
//             needs bits 11..42 of its sum: wrapping 32 bits when the sum fits int32, else 64 bits.  Its matrix rows
//             are (10703, 4433) and (4433, -10704) [FIX(0.541196100) + FIX(0.765366865), FIX(0.541196100),
//             FIX(0.541196100) - FIX(1.847759065)]: L1 norm 15137, and 15137 * x + 2^10 <= 2^31 - 1 holds up to
//             x = 141869 = QS_DEC_FAST_BOUND4 on |dq| of rows 1 and 3 (tests/decode_scaled_host.cpp prints the norm).
//             pass 2 (4-point or 8-point rows, >> 18, & 1023): the sum modulo 2^28, wrapping 32 bits always.
//   4x8       pass 1 is jpeg_idct_islow's 8-point column: QS_DEC_FAST_BOUND as at full size; pass 2 as above.
//   4x2, 2x4  the workspace is INT32 and nothing is shifted before the end: ((...) >> 16) & 1023 takes the sum modulo
//             2^26, wrapping 32 bits in both passes.
//   2x2, 2x1, 1x2, 1x1  sums of dequantised values plus (RANGE_CENTER << 3) + 4, then (>> 3) & 1023: modulo 2^13.
#define QS_DEC_FAST_BOUND4 141869

// the 4-point kernels' odd part: z1 = (z2 + z3) * c6 + bias; o[0] = z1 + z2 * (c2 - c6), o[1] = z1 - z3 * (c2 + c6)
template <class T>
QS_DEC_HDF void qd_idct4_odd(T z2, T z3, T bias, T* o) {
  const T z1 = (z2 + z3) * (T)QD_FIX(0.541196100) + bias;
  o[0] = z1 + z2 * (T)QD_FIX(0.765366865);
  o[1] = z1 - z3 * (T)QD_FIX(1.847759065);
}

// One 4-point row / column whose even part is shifted by CONST_BITS (pass 2 of 4x4, 4x8, 4x2; pass 1 of 2x4).  dc_bias
// is added to in[0] before the shift.  Wrapping arithmetic.
QS_DEC_HDF void qd_idct4(const uint32_t* in, uint32_t dc_bias, uint32_t* out) {
  const uint32_t t0 = in[0] + dc_bias, t2 = in[2];
  const uint32_t t10 = (t0 + t2) << 13, t12 = (t0 - t2) << 13;
  uint32_t o[2];
  qd_idct4_odd<uint32_t>(in[1], in[3], 0u, o);
  out[0] = t10 + o[0]; out[3] = t10 - o[0];
  out[1] = t12 + o[1]; out[2] = t12 - o[1];
}

// One 4-point column of pass 1 of jpeg_idct_4x4 / _8x4: the even part << PASS1_BITS, the odd part descaled on its own.
QS_DEC_HDF void qd_idct4_pass1(const int32_t* in, bool fast, int32_t* ws) {
  const uint32_t e0 = ((uint32_t)in[0] + (uint32_t)in[2]) << 2, e1 = ((uint32_t)in[0] - (uint32_t)in[2]) << 2;
  uint32_t o0, o1;
  if (fast) {
    uint32_t o[2];
    qd_idct4_odd<uint32_t>((uint32_t)in[1], (uint32_t)in[3], 1u << 10, o);
    o0 = (uint32_t)((int32_t)o[0] >> 11); o1 = (uint32_t)((int32_t)o[1] >> 11);
  } else {
    int64_t o[2];
    qd_idct4_odd<int64_t>(in[1], in[3], (int64_t)1 << 10, o);
    o0 = (uint32_t)(o[0] >> 11); o1 = (uint32_t)(o[1] >> 11);      // (int) of libjpeg's INT32 sum: its low 32 bits
  }
  ws[0] = (int32_t)(e0 + o0); ws[3] = (int32_t)(e0 - o0);
  ws[1] = (int32_t)(e1 + o1); ws[2] = (int32_t)(e1 - o1);
}

// pass-2 bias of the kernels whose pass 1 scales by PASS1_BITS, added to in[0] before the shift (qd_idct4)
#define QD_PASS2_BIAS4 ((512u << 5) + (1u << 4))
// (RANGE_CENTER << 3) + (1 << 2): the 2- and 1-point forms and 4x2, whose pass 1 does not scale
#define QD_BIAS3 ((512u << 3) + (1u << 2))

// The block's top-left PW columns x PH rows, dequantised: dq[r * PW + c].  One load of PW * 2 bytes per row (src is a
// block of a 16-byte aligned array: row r lies 16 * r bytes in).
template <int PW, int PH>
QS_DEC_HDF void qd_load_sub(const int16_t* src, const uint16_t* q, int32_t* dq) {
  QD_UNROLL
  for (int r = 0; r < PH; ++r) {
    struct alignas(PW * 2) Row { int16_t v[PW]; };
    const Row row = *reinterpret_cast<const Row*>(src + r * 8);
    QD_UNROLL
    for (int c = 0; c < PW; ++c) dq[r * PW + c] = (int32_t)row.v[c] * (int32_t)q[r * 8 + c];
  }
}

// jpeg_idct_<PW>x<PH> on qd_load_sub's values: PH rows of PW samples into dst (row stride `stride`), each column
// written XREP times.  (8x8 is qd_idct_block<false, false>.)
template <int PW, int PH, int XREP = 1>
QS_DEC_HDF void qd_idct_scaled(const int32_t* dq, uint8_t* dst, int stride) {
  auto put = [&](int r, int c, uint8_t s) {
    QD_UNROLL
    for (int k = 0; k < XREP; ++k) dst[r * stride + c * XREP + k] = s;
  };
  if constexpr (PW <= 2 && PH <= 2) {
    const uint32_t a = (uint32_t)dq[0] + QD_BIAS3;
    if constexpr (PW == 1 && PH == 1) {
      put(0, 0, qd_limit(a >> 3));
    } else if constexpr (PW * PH == 2) {                   // 2x1: dq[1] is column 1; 1x2: dq[1] is row 1
      put(0, 0, qd_limit((a + (uint32_t)dq[1]) >> 3));
      put(PW == 2 ? 0 : 1, PW == 2 ? 1 : 0, qd_limit((a - (uint32_t)dq[1]) >> 3));
    } else {
      const uint32_t t0 = a + (uint32_t)dq[2], t2 = a - (uint32_t)dq[2];
      const uint32_t t1 = (uint32_t)dq[1] + (uint32_t)dq[3], t3 = (uint32_t)dq[1] - (uint32_t)dq[3];
      put(0, 0, qd_limit((t0 + t1) >> 3)); put(0, 1, qd_limit((t0 - t1) >> 3));
      put(1, 0, qd_limit((t2 + t3) >> 3)); put(1, 1, qd_limit((t2 - t3) >> 3));
    }
  } else if constexpr (PW == 4 && PH == 2) {
    QD_UNROLL
    for (int r = 0; r < 2; ++r) {
      uint32_t in[4], o[4];
      QD_UNROLL
      for (int c = 0; c < 4; ++c) in[c] = r ? (uint32_t)dq[c] - (uint32_t)dq[4 + c] : (uint32_t)dq[c] + (uint32_t)dq[4 + c];
      qd_idct4(in, QD_BIAS3, o);
      QD_UNROLL
      for (int c = 0; c < 4; ++c) put(r, c, qd_limit(o[c] >> 16));
    }
  } else if constexpr (PW == 2 && PH == 4) {
    uint32_t ws[4][2];
    QD_UNROLL
    for (int c = 0; c < 2; ++c) {
      uint32_t in[4], o[4];
      QD_UNROLL
      for (int k = 0; k < 4; ++k) in[k] = (uint32_t)dq[k * 2 + c];
      qd_idct4(in, 0u, o);
      QD_UNROLL
      for (int r = 0; r < 4; ++r) ws[r][c] = o[r];
    }
    QD_UNROLL
    for (int r = 0; r < 4; ++r) {
      const uint32_t t = ws[r][0] + ((512u << 16) + (1u << 15));
      put(r, 0, qd_limit((t + ws[r][1]) >> 16));
      put(r, 1, qd_limit((t - ws[r][1]) >> 16));
    }
  } else {
    static_assert((PH == 4 && (PW == 4 || PW == 8)) || (PH == 8 && PW == 4), "4x4, 8x4, 4x8");
    int32_t ws[PH][PW];
    int32_t mx = 0;
    QD_UNROLL
    for (int i = 0; i < PW * PH; ++i) {
      if (PH == 4 && !((i / PW) & 1)) continue;            // (4-point pass 1: rows 1 and 3 alone bear on the choice)
      const int32_t a = dq[i] < 0 ? -dq[i] : dq[i];
      mx = a > mx ? a : mx;
    }
    const bool fast = mx <= (PH == 4 ? QS_DEC_FAST_BOUND4 : QS_DEC_FAST_BOUND);
    QD_UNROLL
    for (int c = 0; c < PW; ++c) {                         // pass 1: columns
      if constexpr (PH == 4) {
        int32_t in[4], o[4];
        QD_UNROLL
        for (int k = 0; k < 4; ++k) in[k] = dq[k * PW + c];
        qd_idct4_pass1(in, fast, o);
        QD_UNROLL
        for (int r = 0; r < 4; ++r) ws[r][c] = o[r];
      } else if (fast) {
        uint32_t in[8], o[8];
        QD_UNROLL
        for (int k = 0; k < 8; ++k) in[k] = (uint32_t)dq[k * PW + c];
        qd_idct8<uint32_t>(in, 1u << 10, o);
        QD_UNROLL
        for (int r = 0; r < 8; ++r) ws[r][c] = (int32_t)o[r] >> 11;
      } else {
        int64_t in[8], o[8];
        QD_UNROLL
        for (int k = 0; k < 8; ++k) in[k] = dq[k * PW + c];
        qd_idct8<int64_t>(in, (int64_t)1 << 10, o);
        QD_UNROLL
        for (int r = 0; r < 8; ++r) ws[r][c] = (int32_t)(o[r] >> 11);
      }
    }
    QD_UNROLL
    for (int r = 0; r < PH; ++r) {                         // pass 2: rows, modulo 2^32
      uint32_t in[PW], o[PW];
      QD_UNROLL
      for (int k = 0; k < PW; ++k) in[k] = (uint32_t)ws[r][k];
      if constexpr (PW == 8) qd_idct8<uint32_t>(in, QD_PASS2_BIAS, o); else qd_idct4(in, QD_PASS2_BIAS4, o);
      QD_UNROLL
      for (int c = 0; c < PW; ++c) put(r, c, qd_limit(o[c] >> 18));
    }
  }
}

template <int PW, int PH, int XREP = 1>
QS_DEC_HDF void qd_scaled_block(const int16_t* src, const uint16_t* q, uint8_t* dst, int stride) {
  int32_t dq[PW * PH];
  qd_load_sub<PW, PH>(src, q, dq);
  if constexpr (PW == 8 && PH == 8) qd_idct_block<false, false>(dq, dst, stride);
  else qd_idct_scaled<PW, PH, XREP>(dq, dst, stride);
}

// The scaled kernel's tile: QS_DEC_TW x QS_DEC_TH output samples, a whole number of MCUs at every scale and layout.
// Component ci's blocks cover bw x bh output samples each (luma m x m, chroma m * hs x m * vs); the tile's work items
// are its luma blocks, then chroma 1's, then chroma 2's, in raster order: 64 / 256 / 1,024 luma blocks at m = 4 / 2 / 1.
// output samples per luma block edge of a job: 8 / scale_denom; 0 for a record that is not one of prepare's
QS_DEC_HDF int qd_job_m(const QsDecJob& job) {
  const int d = job.upsampling >> 8;
  return d == 0 ? 8 : d == 2 ? 4 : d == 4 ? 2 : d == 8 ? 1 : 0;
}

QS_DEC_HDF int qd_scaled_items(const QsDecJob& job, const QsDecGeom& g, int m) {
  const int nl = (QS_DEC_TW / m) * (QS_DEC_TH / m);
  return job.layout == QS_DEC_GRAY ? nl : nl + 2 * (QS_DEC_TW / (m * g.hs)) * (QS_DEC_TH / (m * g.vs));
}

// Work item `it` of the tile at (X0, Y0): one block of one component into its plane px[ci] (QS_DEC_TH rows of QS_DEC_TW).
// width x height: the output crop (never more than the caller's extent).  A block outside the crop, the component's
// grid or the caller's array is not read and leaves its samples unwritten (no pixel of the crop takes them).
QS_DEC_HDF void qd_scaled_item(const QsDecJob& job, const QsDecPtrs& P, const QsDecGeom& g, int variant, int m, int width,
                              int height, int X0, int Y0, int it, uint8_t* px) {
  const int nl = (QS_DEC_TW / m) * (QS_DEC_TH / m);
  const int ci = it < nl ? 0 : 1 + (it - nl) / ((QS_DEC_TW / (m * g.hs)) * (QS_DEC_TH / (m * g.vs)));
  const int hs = ci ? g.hs : 1, vs = ci ? g.vs : 1;
  const int bw = m * hs, bh = m * vs, nbx = QS_DEC_TW / bw;
  const int k = ci ? (it - nl) % (nbx * (QS_DEC_TH / bh)) : it;
  const int kx = k % nbx, ky = k / nbx;
  const int bx = X0 / bw + kx, by = Y0 / bh + ky, x0 = kx * bw, y0 = ky * bh;
  const int slot = variant && ci ? 2 + ci : ci;
  if (!(X0 + x0 < width && Y0 + y0 < height && bx < g.wblk[ci] && by < g.hblk[ci] &&
        (long long)by * g.wblk[ci] + bx < P.nblk[slot])) return;
  const int16_t* src = P.coef[slot] + ((size_t)by * g.wblk[ci] + bx) * 64;
  const uint16_t* q = job.q[ci];
  uint8_t* dst = px + ((size_t)ci * QS_DEC_TH + y0) * QS_DEC_TW + x0;
  const int pw = hs == 4 ? bw / 2 : bw;                    // 4x1: a 2m x m IDCT, each column twice
  switch (pw * 16 + bh) {
    case 8 * 16 + 8: qd_scaled_block<8, 8>(src, q, dst, QS_DEC_TW); break;
    case 4 * 16 + 4: qd_scaled_block<4, 4>(src, q, dst, QS_DEC_TW); break;
    case 2 * 16 + 2: qd_scaled_block<2, 2>(src, q, dst, QS_DEC_TW); break;
    case 1 * 16 + 1: qd_scaled_block<1, 1>(src, q, dst, QS_DEC_TW); break;
    case 8 * 16 + 4:
      if (hs == 4) qd_scaled_block<8, 4, 2>(src, q, dst, QS_DEC_TW); else qd_scaled_block<8, 4>(src, q, dst, QS_DEC_TW);
      break;
    case 4 * 16 + 2:
      if (hs == 4) qd_scaled_block<4, 2, 2>(src, q, dst, QS_DEC_TW); else qd_scaled_block<4, 2>(src, q, dst, QS_DEC_TW);
      break;
    case 2 * 16 + 1:
      if (hs == 4) qd_scaled_block<2, 1, 2>(src, q, dst, QS_DEC_TW); else qd_scaled_block<2, 1>(src, q, dst, QS_DEC_TW);
      break;
    case 4 * 16 + 8: qd_scaled_block<4, 8>(src, q, dst, QS_DEC_TW); break;
    case 2 * 16 + 4: qd_scaled_block<2, 4>(src, q, dst, QS_DEC_TW); break;
    case 1 * 16 + 2: qd_scaled_block<1, 2>(src, q, dst, QS_DEC_TW); break;
    default: break;                                        // (never prepared)
  }
}

// Pixel (x, r) of the tile: its component samples -> its output samples in rows (QS_DEC_TH rows of QS_DEC_TW * 3).
QS_DEC_HDF void qd_scaled_convert(const QsDecJob& job, const uint8_t* px, int r, int x, uint8_t* rows) {
  const uint8_t* p = px + (size_t)r * QS_DEC_TW + x;
  uint8_t* o = rows + (size_t)r * QS_DEC_TW * 3;
  if (job.layout == QS_DEC_YCC) {
    qd_ycc_rgb(p[0], p[QS_DEC_TH * QS_DEC_TW], p[2 * QS_DEC_TH * QS_DEC_TW], o + x * 3);
  } else if (job.layout == QS_DEC_RGB) {
    o[x * 3] = p[0];
    o[x * 3 + 1] = p[QS_DEC_TH * QS_DEC_TW];
    o[x * 3 + 2] = p[2 * QS_DEC_TH * QS_DEC_TW];
  } else {
    o[x] = p[0];
  }
}
