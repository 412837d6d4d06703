// qs_compress.h -- the device compress of pixels to quantised coefficient arrays (qs_hip_compress_device_batch,
// csrc/qs_kernels_compress.hip): libjpeg 9's RGB -> YCbCr conversion (jccolor.c), its edge replication and both of its
// chroma downsamplings -- the box filter of do_fancy_downsampling = FALSE (jcprepct.c, jcsample.c) with jpeg_fdct_islow,
// and its default, 2x chroma through the scaled forward DCTs jpeg_fdct_16x16 / _16x8 / _8x16 (jfdctint.c) -- and the
// quantiser of jcdctmgr.c, as functions the kernel and the host builds (tests/compress_host.cpp,
// tests/compress_fancy_host.cpp) can both compile, and the per-job descriptor the host driver writes into the caller's
// workspace.
//
// Covered: JDCT_ISLOW with either downsampling, per job (QsCmpJob::mode).  OUT OF SCOPE: smoothing_factor != 0 and the
// other DCT methods (JDCT_IFAST, JDCT_FLOAT).  For 1x1 chroma and grayscale the two modes coincide.
//
// Numerical contract: everything fits wrapping 32-bit arithmetic for 8-bit samples.
//   colour:  |FIX(c) * s| <= 65536 * 255 per term, three terms plus (128 << 16) + 32767 < 2^26.
// Each DCT pass is an integer matrix M (the composed FIX() constants) and one rounding shift.  The matrices are taken
// with unit vectors from a host build (tests/compress_fancy_host.cpp norms; asserted in
// tests/test_compress_fancy_host.py): row 0 is the plain sum (L1 norm 8 or 16); every other row sums to zero, so x may be
// taken as x - 128, |x - 128| <= 128; the largest row L1 norm is 60 548 for the 8-point pass (row 4 of it is a
// butterfly of norm 8, scaled << 2) and 121 088 for the 16-point pass -- not the crude 8 or 16 times 11 590.
//   pass 1:  8-point  |sum| <=  60 548 * 128 + 2^10 < 2^23, stored >> 11: |d| <= 3 784; DC (sum - 1024) << 2: |d| <= 4 096.
//            16-point |sum| <= 121 088 * 128 + 2^10 < 2^24, stored >> 11: |d| <= 7 568; DC (sum - 2048) << 2: |d| <= 8 192.
//   pass 2:  a column of |d| <= dmax through either matrix, plus the rounding term:
//            8x8    60 548 * 4 096 + 2^14 < 2^27.9        16x8  60 548 * 8 192 + 2^15 < 2^28.9
//            8x16  121 088 * 4 096 + 2^15 < 2^28.9        16x16 121 088 * 8 192 + 2^16 = 992 018 432 < 2^29.9
// The crude bound 16 * 11 590 * 11 590 passes 2^31 for the second pass of _16x16 (libjpeg's INT32 is a 64-bit long
// there); the measured norms leave a factor 2.16 of room, so NO pass needs 64-bit arithmetic.
// Every final sum fits int32, so sums and products taken modulo 2^32 (uint32_t here) agree with the true ones: a value
// in [-2^31, 2^31) is its own residue, whatever the intermediates did.  After pass 2's shifts |w| <= 8 192 (the DC of an
// all-0 block; 7 569 elsewhere) < 2^17, the domain over which the quantiser's reciprocal is proven below.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define QS_CMP_HD __host__ __device__ inline
#else
#define QS_CMP_HD static inline
#endif

enum {                           // the supported layouts (qs_hip_compress_device_batch_info): those of the decode
  QS_CMP_GRAY = 0,               // one component, taken as 1x1
  QS_CMP_YCC = 1,                // RGB -> YCbCr, chroma 1x1, luma (h, v) in {(1,1), (2,1), (1,2), (2,2), (4,1)}
  QS_CMP_RGB = 2                 // RGB without a colour transform, same sampling set
};

#define QS_CMP_TW 64             // input tile: 64 x 16 pixels = a whole number of MCUs in every supported layout
#define QS_CMP_TH 16
#define QS_CMP_CHUNK 44          // jobs per launch (about 2.8 KiB of kernel arguments)

// One job as the kernel sees it (workspace, written by the prepare call): geometry and tables, no addresses.
struct QsCmpJob {
  int32_t width, height;         // the image
  int32_t layout, nin;           // QS_CMP_*, input samples per pixel (1 or 3)
  int32_t hs, vs;                // component 0's sampling factors (chroma is 1x1); 1x1 for gray
  int32_t wib[3], hib[3];        // libjpeg's width_in_blocks / height_in_blocks: the blocks that are written
  int32_t stride[3];             // the caller's row stride in blocks (its wblk >= wib)
  int32_t tiles_x;               // tiles per tile row
  int32_t tile0, tiles;          // first workgroup of this job in its chunk's launch, and how many it has
  int32_t mode, pad;             // QS_CMP_DS_*: what chroma goes through (qc_chroma_shape)
  uint16_t q[3][64];             // the components' tables (natural order)
  uint32_t recip[3][64];         // qc_recip(q << 3)
};

// What addresses caller memory travels in the kernel arguments of the run call, so the kernel bounds every access by
// them: reads by width x height x pitch, stores by nblk.
struct QsCmpPtrs {
  const uint8_t* pix;
  int64_t pitch;
  int16_t* coef[3];
  int32_t nblk[3];               // blocks in each array
  int32_t width, height;         // the input extent the caller gave
  int32_t pad;
};
struct QsCmpArgs {
  const QsCmpJob* jobs;          // the chunk's descriptors (workspace)
  int32_t n, pad;
  QsCmpPtrs p[QS_CMP_CHUNK];
};

// ---- jccolor.c (libjpeg 9, rgb_ycc_convert): SCALEBITS 16, FIX(x) = (INT32)(x * 65536 + 0.5), arithmetic shift ------
#define QC_FIX16(x) ((int32_t)((x) * 65536.0 + 0.5))
QS_CMP_HD void qc_rgb_ycc(int r, int g, int b, uint8_t* out) {
  const int32_t half = 1 << 15, cboff = (128 << 16) + half - 1;      // CBCR_OFFSET + ONE_HALF - 1
  out[0] = (uint8_t)((QC_FIX16(0.299) * r + QC_FIX16(0.587) * g + QC_FIX16(0.114) * b + half) >> 16);
  out[1] = (uint8_t)((-QC_FIX16(0.168735892) * r - QC_FIX16(0.331264108) * g + QC_FIX16(0.5) * b + cboff) >> 16);
  out[2] = (uint8_t)((QC_FIX16(0.5) * r - QC_FIX16(0.418687589) * g - QC_FIX16(0.081312411) * b + cboff) >> 16);
}

// ---- edges (jcprepct.c, jcsample.c) -----------------------------------------------------------------------------------
// Horizontally the input's right edge is replicated BEFORE downsampling: a source column is min(x, W - 1).
// Vertically libjpeg first pads the input to a multiple of max_v_samp rows with row H - 1, downsamples, and then
// repeats the last DOWNSAMPLED row of each component.  Component row r of a component with v_samp_c of max_v:
//   r' = min(r, ceil(H / max_v) * v_samp_c - 1), source rows min(r' * (max_v / v_samp_c) + dy, H - 1).
// For the component with v_samp_c = max_v (luma) that is the plain clamp min(r, H - 1).
QS_CMP_HD int qc_src_col(int x, int W) { return x < W - 1 ? x : W - 1; }
QS_CMP_HD int qc_src_row(int r, int dy, int H, int max_v, int v_samp) {
  const int last = (H + max_v - 1) / max_v * v_samp - 1;
  const int rr = r < last ? r : last;
  const int y = rr * (max_v / v_samp) + dy;
  return y < H - 1 ? y : H - 1;
}

// ---- jcsample.c without fancy downsampling: a box of hx x vy samples summed to `sum`, x = the output column ----------
// h2v1: bias 0, 1, 0, 1, ...; h2v2: bias 1, 2, 1, 2, ...; every other ratio (int_downsample): (sum + n / 2) / n
QS_CMP_HD int qc_downsample(int sum, int hx, int vy, int x) {
  if (hx == 2 && vy == 1) return (sum + (x & 1)) >> 1;
  if (hx == 2 && vy == 2) return (sum + 1 + (x & 1)) >> 2;
  const int n = hx * vy;
  return (sum + (n >> 1)) / n;
}

// ---- jfdctint.c: jpeg_fdct_islow (CONST_BITS 13, PASS1_BITS 2), one 8-point pass in wrapping 32 bits -----------------
#define QC_FIX(x) ((uint32_t)(int32_t)((x) * 8192 + 0.5))
// The 8-point kernel both passes share.  in[k]: the samples / pass-1 values (as residues modulo 2^32); even0 is added
// to the sum behind outputs 0 and 4 (pass 2's fudge 1 << (PASS1_BITS - 1); pass 1 has none); fudge is the rounding
// term of the six rotated outputs.  The outputs are the sums before their shifts: the caller shifts.
QS_CMP_HD void qc_fdct8(const uint32_t* in, uint32_t even0, uint32_t fudge, uint32_t* o) {
  uint32_t tmp0 = in[0] + in[7], tmp1 = in[1] + in[6], tmp2 = in[2] + in[5], tmp3 = in[3] + in[4];
  const uint32_t tmp10 = tmp0 + tmp3 + even0, tmp11 = tmp1 + tmp2;
  uint32_t tmp12 = tmp0 - tmp3, tmp13 = tmp1 - tmp2;
  tmp0 = in[0] - in[7]; tmp1 = in[1] - in[6]; tmp2 = in[2] - in[5]; tmp3 = in[3] - in[4];
  o[0] = tmp10 + tmp11;
  o[4] = tmp10 - tmp11;
  uint32_t z1 = (tmp12 + tmp13) * QC_FIX(0.541196100) + fudge;
  o[2] = z1 + tmp12 * QC_FIX(0.765366865);
  o[6] = z1 - tmp13 * QC_FIX(1.847759065);
  tmp12 = tmp0 + tmp2;
  tmp13 = tmp1 + tmp3;
  z1 = (tmp12 + tmp13) * QC_FIX(1.175875602) + fudge;
  tmp12 = z1 - tmp12 * QC_FIX(0.390180644);
  tmp13 = z1 - tmp13 * QC_FIX(1.961570560);
  z1 = (uint32_t)0 - (tmp0 + tmp3) * QC_FIX(0.899976223);
  tmp0 = tmp0 * QC_FIX(1.501321110) + z1 + tmp12;
  tmp3 = tmp3 * QC_FIX(0.298631336) + z1 + tmp13;
  z1 = (uint32_t)0 - (tmp1 + tmp2) * QC_FIX(2.562915447);
  tmp1 = tmp1 * QC_FIX(3.072711026) + z1 + tmp13;
  tmp2 = tmp2 * QC_FIX(2.053119869) + z1 + tmp12;
  o[1] = tmp0; o[3] = tmp1; o[5] = tmp2; o[7] = tmp3;
}

// pass 1: one row of 8 samples -> 8 values scaled by 2^PASS1_BITS (jpeg_fdct_islow subtracts CENTERJSAMPLE itself)
QS_CMP_HD void qc_fdct_row(const uint8_t* s, int32_t* d) {
  uint32_t in[8], o[8];
  for (int k = 0; k < 8; ++k) in[k] = s[k];
  qc_fdct8(in, 0, 1u << 10, o);
  o[0] -= 8u * 128u;                                     // 8 * CENTERJSAMPLE: the unsigned -> signed conversion
  for (int k = 0; k < 8; ++k) d[k] = (k & 3) ? (int32_t)o[k] >> 11 : (int32_t)(o[k] << 2);
}

// pass 2: one column of pass-1 values -> 8 outputs, left scaled by 8
QS_CMP_HD void qc_fdct_col(const int32_t* d, int32_t* w) {
  uint32_t in[8], o[8];
  for (int k = 0; k < 8; ++k) in[k] = (uint32_t)d[k];
  qc_fdct8(in, 1u << 1, 1u << 14, o);
  for (int k = 0; k < 8; ++k) w[k] = (int32_t)o[k] >> ((k & 3) ? 15 : 2);
}

// ---- jfdctint.c: the 16-point pass of jpeg_fdct_16x16 / _16x8 / _8x16 (cK = sqrt(2) * cos(K * pi / 32)) --------------
// 16 inputs -> the 8 low-frequency sums BEFORE rounding and shift: o[0] is the plain sum of the inputs, o[1..7] carry
// 2^CONST_BITS.  T is uint32_t (wrapping; exact whenever the final sums fit int32, see the contract above) or int64_t.
template <class T>
QS_CMP_HD void qc_fdct16(const T* in, T* o) {
#define QC_F(x) ((T)(int32_t)((x) * 8192 + 0.5))
  T tmp0 = in[0] + in[15], tmp1 = in[1] + in[14], tmp2 = in[2] + in[13], tmp3 = in[3] + in[12];
  T tmp4 = in[4] + in[11], tmp5 = in[5] + in[10], tmp6 = in[6] + in[9], tmp7 = in[7] + in[8];
  T tmp10 = tmp0 + tmp7, tmp14 = tmp0 - tmp7, tmp11 = tmp1 + tmp6, tmp15 = tmp1 - tmp6;
  T tmp12 = tmp2 + tmp5, tmp16 = tmp2 - tmp5, tmp13 = tmp3 + tmp4, tmp17 = tmp3 - tmp4;
  tmp0 = in[0] - in[15]; tmp1 = in[1] - in[14]; tmp2 = in[2] - in[13]; tmp3 = in[3] - in[12];
  tmp4 = in[4] - in[11]; tmp5 = in[5] - in[10]; tmp6 = in[6] - in[9]; tmp7 = in[7] - in[8];
  o[0] = tmp10 + tmp11 + tmp12 + tmp13;
  o[4] = (tmp10 - tmp13) * QC_F(1.306562965) + (tmp11 - tmp12) * QC_F(0.541196100);       // c4, c12
  tmp10 = (tmp17 - tmp15) * QC_F(0.275899379) + (tmp14 - tmp16) * QC_F(1.387039845);      // c14, c2
  o[2] = tmp10 + tmp15 * QC_F(1.451774982) + tmp16 * QC_F(2.172734804);                   // c6+c14, c2+c10
  o[6] = tmp10 - tmp14 * QC_F(0.211164243) - tmp17 * QC_F(1.061594338);                   // c2-c6, c10+c14
  tmp11 = (tmp0 + tmp1) * QC_F(1.353318001) + (tmp6 - tmp7) * QC_F(0.410524528);          // c3, c13
  tmp12 = (tmp0 + tmp2) * QC_F(1.247225013) + (tmp5 + tmp7) * QC_F(0.666655658);          // c5, c11
  tmp13 = (tmp0 + tmp3) * QC_F(1.093201867) + (tmp4 - tmp7) * QC_F(0.897167586);          // c7, c9
  tmp14 = (tmp1 + tmp2) * QC_F(0.138617169) + (tmp6 - tmp5) * QC_F(1.407403738);          // c15, c1
  tmp15 = (T)0 - (tmp1 + tmp3) * QC_F(0.666655658) - (tmp4 + tmp6) * QC_F(1.247225013);   // -c11, -c5
  tmp16 = (T)0 - (tmp2 + tmp3) * QC_F(1.353318001) + (tmp5 - tmp4) * QC_F(0.410524528);   // -c3, c13
  o[1] = tmp11 + tmp12 + tmp13 - tmp0 * QC_F(2.286341144) + tmp7 * QC_F(0.779653625);
  o[3] = tmp11 + tmp14 + tmp15 + tmp1 * QC_F(0.071888074) - tmp6 * QC_F(1.663905119);
  o[5] = tmp12 + tmp14 + tmp16 - tmp2 * QC_F(1.125726048) + tmp5 * QC_F(1.227391138);
  o[7] = tmp13 + tmp15 + tmp16 + tmp3 * QC_F(1.065388962) + tmp4 * QC_F(2.167985692);
#undef QC_F
}

// pass 1 of _16x16 and _16x8: one row of 16 samples -> 8 values scaled by 2^PASS1_BITS (16 * CENTERJSAMPLE leaves the
// sum; the other rows of the matrix sum to zero).  Wrapping 32 bits: |sum| < 2^24 (contract above).
QS_CMP_HD void qc_fdct16_row(const uint8_t* s, int32_t* d) {
  uint32_t in[16], o[8];
  for (int k = 0; k < 16; ++k) in[k] = s[k];
  qc_fdct16<uint32_t>(in, o);
  d[0] = (int32_t)((o[0] - 16u * 128u) << 2);
  for (int k = 1; k < 8; ++k) d[k] = (int32_t)(o[k] + (1u << 10)) >> 11;
}

// pass 2 of _16x16 (extra = 2: the output scaled by (8/16)^2) and of _8x16 (extra = 1: by 8/16): one column of 16
// pass-1 values -> 8 outputs, left scaled by 8
QS_CMP_HD void qc_fdct16_col(const int32_t* d, int extra, int32_t* w) {
  uint32_t in[16], o[8];
  for (int k = 0; k < 16; ++k) in[k] = (uint32_t)d[k];
  qc_fdct16<uint32_t>(in, o);
  w[0] = (int32_t)(o[0] + (1u << (1 + extra))) >> (2 + extra);
  for (int k = 1; k < 8; ++k) w[k] = (int32_t)(o[k] + (1u << (14 + extra))) >> (15 + extra);
}

// pass 2 of _16x8: the 8-point column pass with one more bit removed (the output scaled by 8/16)
QS_CMP_HD void qc_fdct_col_half(const int32_t* d, int32_t* w) {
  uint32_t in[8], o[8];
  for (int k = 0; k < 8; ++k) in[k] = (uint32_t)d[k];
  qc_fdct8(in, 1u << 2, 1u << 15, o);
  for (int k = 0; k < 8; ++k) w[k] = (int32_t)o[k] >> ((k & 3) ? 16 : 3);
}

// ---- jcdctmgr.c: forward_DCT's quantiser for JDCT_ISLOW, divisor d = quantval << 3 ------------------------------------
// coef = sign(w) * ((|w| + (d >> 1)) / d), exact integer division.  The division is a multiplication by
// m = floor(2^32 / d) and one correction: for 0 <= a < 2^32 and 8 <= d < 2^19, with e = 2^32 / d - m in [0, 1),
//   a / d - a * m / 2^32 = a * e / 2^32 in [0, 1),
// so t = floor(a * m / 2^32) is floor(a / d) or one less, and a - t * d >= d tells which.  (d >= 8 keeps m < 2^32.)
QS_CMP_HD uint32_t qc_recip(uint32_t d) { return (uint32_t)(((uint64_t)1 << 32) / d); }
QS_CMP_HD int16_t qc_quant(int32_t w, uint32_t q, uint32_t m) {
  const uint32_t d = q << 3;
  const uint32_t a = (uint32_t)(w < 0 ? -w : w) + (d >> 1);
  uint32_t t = (uint32_t)(((uint64_t)a * m) >> 32);
  if (a - t * d >= d) ++t;
  return (int16_t)(w < 0 ? -(int32_t)t : (int32_t)t);
}

// ---- what chroma goes through (jcmaster.c, jcsample.c, jcdctmgr.c), per downsampling mode -----------------------------
// With luma hs x vs and chroma 1x1, one chroma block covers 8 hs x 8 vs pixels.  QS_CMP_DS_BOX: a box of hs x vs, then the
// 8x8 DCT.  QS_CMP_DS_DCT (do_fancy_downsampling = TRUE): libjpeg scales the component's DCT up to 2x each way
// (DCT_h_scaled_size 16 where hs >= 2, DCT_v_scaled_size 16 where vs == 2) and downsamples only what is left: the
// h2v1 box for 4x1, nothing otherwise.  Edges are plain clamps there: source column min(x, W - 1), source row
// min(y, H - 1) (the expanded-edge rows of jcprepct.c; no downsampled row is repeated, since none is made).
#define QS_CMP_DS_BOX 0
#define QS_CMP_DS_DCT 1
struct QsCmpShape {
  int bh, bv;                    // the box in front of the DCT
  int dw, dh;                    // samples one block's DCT takes: 8 or 16 each way
};
QS_CMP_HD QsCmpShape qc_chroma_shape(int mode, int hs, int vs) {
  QsCmpShape s;
  if (mode == QS_CMP_DS_DCT) {
    s.bh = hs == 4 ? 2 : 1; s.bv = 1;
    s.dw = hs >= 2 ? 16 : 8; s.dh = vs == 2 ? 16 : 8;
  } else {
    s.bh = hs; s.bv = vs; s.dw = 8; s.dh = 8;
  }
  return s;
}

// libjpeg's geometry of component ci: width_in_blocks / height_in_blocks for a sampling factor `samp` of `max`
QS_CMP_HD int qc_blocks(int pixels, int samp, int max) {
  return (int)(((long long)pixels * samp + 8LL * max - 1) / (8LL * max));
}
