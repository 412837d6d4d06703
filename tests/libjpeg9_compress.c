/*
 * libjpeg9_compress.c -- TEST ORACLE for the device compress (tests/test_compress_host.py, tests/test_gpu_compress.py):
 * libjpeg 9 itself, with no code of this project or of the reference in the loop.
 *
 *   libjpeg9_compress image in.bin out.jpg   compress pixels with jpeg_write_scanlines: JDCT_ISLOW, smoothing_factor 0,
 *                                            do_fancy_downsampling FALSE, one explicitly given table per component
 *                                            (quant_tbl_no = c, quantval set directly)
 *   libjpeg9_compress block in.bin out.bin   the exported jpeg_fdct_islow on blocks of samples
 *
 * image in.bin: int32 magic 0x51534a43, ncomp (1 or 3), image_width, image_height, jpeg colour space (1 gray, 2 RGB,
 *   3 YCbCr); per component int32 hsamp, vsamp; uint16 quant[64] (natural order); then image_height rows of
 *   image_width * ncomp samples (gray, or RGB).  The coefficient arrays are read back from out.jpg with
 *   `libjpeg9_decode read`.
 * block in.bin: int32 n, then n blocks of 64 samples; out.bin: n blocks of 64 int32 (the DCT scaled by 8).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "jpeglib.h"

#define MAGIC 0x51534a43

/* exported by libjpeg 9 (jfdctint.c), declared in its private jdct.h; DCTELEM is int for 8-bit samples */
extern void jpeg_fdct_islow(int *data, JSAMPARRAY sample_data, JDIMENSION start_col);

static int do_image(const char *src, const char *dst) {
	struct jpeg_compress_struct co;
	struct jpeg_error_mgr err;
	FILE *in = fopen(src, "rb"), *out;
	int32_t hdr[5], samp[3][2];
	uint16_t q[3][64];
	unsigned char *px;
	size_t rowbytes;
	int c, i, n;
	if (!in || fread(hdr, sizeof hdr, 1, in) != 1 || hdr[0] != MAGIC) { fprintf(stderr, "libjpeg9_compress: bad header\n"); return 1; }
	n = hdr[1];
	if ((n != 1 && n != 3) || hdr[2] < 1 || hdr[3] < 1) { fprintf(stderr, "libjpeg9_compress: bad geometry\n"); return 1; }
	for (c = 0; c < n; c++)
		if (fread(samp[c], sizeof samp[c], 1, in) != 1 || fread(q[c], sizeof q[c], 1, in) != 1) return 1;
	rowbytes = (size_t)hdr[2] * n;
	px = (unsigned char *)malloc(rowbytes * hdr[3]);
	if (!px || fread(px, 1, rowbytes * hdr[3], in) != rowbytes * hdr[3]) { fprintf(stderr, "libjpeg9_compress: short pixels\n"); return 1; }
	fclose(in);
	if (!(out = fopen(dst, "wb"))) return 1;

	co.err = jpeg_std_error(&err);
	jpeg_create_compress(&co);
	jpeg_stdio_dest(&co, out);
	co.image_width = (JDIMENSION)hdr[2];
	co.image_height = (JDIMENSION)hdr[3];
	co.input_components = n;
	co.in_color_space = n == 1 ? JCS_GRAYSCALE : JCS_RGB;
	jpeg_set_defaults(&co);
	jpeg_set_colorspace(&co, (J_COLOR_SPACE)hdr[4]);
	co.dct_method = JDCT_ISLOW;
	co.smoothing_factor = 0;
	co.do_fancy_downsampling = FALSE;
	co.optimize_coding = FALSE;
	for (c = 0; c < n; c++) {
		JQUANT_TBL *t;
		co.comp_info[c].h_samp_factor = samp[c][0];
		co.comp_info[c].v_samp_factor = samp[c][1];
		co.comp_info[c].quant_tbl_no = c;
		if (!co.quant_tbl_ptrs[c]) co.quant_tbl_ptrs[c] = jpeg_alloc_quant_table((j_common_ptr)&co);
		t = co.quant_tbl_ptrs[c];
		for (i = 0; i < 64; i++) t->quantval[i] = q[c][i];
		t->sent_table = FALSE;
	}
	jpeg_start_compress(&co, TRUE);
	while (co.next_scanline < co.image_height) {
		JSAMPROW row = px + (size_t)co.next_scanline * rowbytes;
		jpeg_write_scanlines(&co, &row, 1);
	}
	jpeg_finish_compress(&co);
	jpeg_destroy_compress(&co);
	free(px);
	return fclose(out) != 0;
}

static int do_block(const char *src, const char *dst) {
	FILE *in = fopen(src, "rb"), *out = fopen(dst, "wb");
	int32_t n, k;
	int i;
	if (!in || !out || fread(&n, sizeof n, 1, in) != 1 || n < 0) return 1;
	for (k = 0; k < n; k++) {
		JSAMPLE s[64];
		JSAMPROW rows[8];
		int data[64];
		int32_t w[64];
		if (fread(s, sizeof s, 1, in) != 1) return 1;
		for (i = 0; i < 8; i++) rows[i] = s + 8 * i;
		jpeg_fdct_islow(data, rows, 0);
		for (i = 0; i < 64; i++) w[i] = data[i];
		fwrite(w, sizeof w, 1, out);
	}
	fclose(in);
	return fclose(out) != 0;
}

int main(int argc, char **argv) {
	if (argc == 4 && !strcmp(argv[1], "image")) return do_image(argv[2], argv[3]);
	if (argc == 4 && !strcmp(argv[1], "block")) return do_block(argv[2], argv[3]);
	fprintf(stderr, "usage: libjpeg9_compress image in.bin out.jpg | block in.bin out.bin\n");
	return 2;
}
