/*
 * libjpeg9_compress_fancy.c -- TEST ORACLE for the device compress with libjpeg 9's default DCT-scaled chroma
 * downsampling (tests/test_compress_fancy_host.py, tests/test_gpu_compress_fancy.py): libjpeg 9 itself, with no code of
 * this project or of the reference in the loop.
 *
 *   libjpeg9_compress_fancy image in.bin out.jpg         compress pixels with jpeg_write_scanlines: JDCT_ISLOW,
 *                                                        smoothing_factor 0, do_fancy_downsampling TRUE, one explicitly
 *                                                        given table per component; in.bin as `libjpeg9_compress image`
 *   libjpeg9_compress_fancy block WxH in.bin out.bin     the exported jpeg_fdct_16x16 / _16x8 / _8x16 (WxH = 16x16,
 *                                                        16x8: 16 wide and 8 high, 8x16) on blocks of samples
 *
 * block in.bin: int32 n, then n blocks of H rows of W samples; out.bin: n blocks of 64 int32 (the DCT scaled by 8).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "jpeglib.h"

#define MAGIC 0x51534a43

/* exported by libjpeg 9 (jfdctint.c), declared in its private jdct.h; DCTELEM is int for 8-bit samples */
extern void jpeg_fdct_16x16(int *data, JSAMPARRAY sample_data, JDIMENSION start_col);
extern void jpeg_fdct_16x8(int *data, JSAMPARRAY sample_data, JDIMENSION start_col);
extern void jpeg_fdct_8x16(int *data, JSAMPARRAY sample_data, JDIMENSION start_col);

static int do_image(const char *src, const char *dst) {
	struct jpeg_compress_struct co;
	struct jpeg_error_mgr err;
	FILE *in = fopen(src, "rb"), *out;
	int32_t hdr[5], samp[3][2];
	uint16_t q[3][64];
	unsigned char *px;
	size_t rowbytes;
	int c, i, n;
	if (!in || fread(hdr, sizeof hdr, 1, in) != 1 || hdr[0] != MAGIC) { fprintf(stderr, "libjpeg9_compress_fancy: bad header\n"); return 1; }
	n = hdr[1];
	if ((n != 1 && n != 3) || hdr[2] < 1 || hdr[3] < 1) { fprintf(stderr, "libjpeg9_compress_fancy: bad geometry\n"); return 1; }
	for (c = 0; c < n; c++)
		if (fread(samp[c], sizeof samp[c], 1, in) != 1 || fread(q[c], sizeof q[c], 1, in) != 1) return 1;
	rowbytes = (size_t)hdr[2] * n;
	px = (unsigned char *)malloc(rowbytes * hdr[3]);
	if (!px || fread(px, 1, rowbytes * hdr[3], in) != rowbytes * hdr[3]) { fprintf(stderr, "libjpeg9_compress_fancy: short pixels\n"); return 1; }
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
	co.do_fancy_downsampling = TRUE;
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

static int do_block(const char *shape, const char *src, const char *dst) {
	FILE *in = fopen(src, "rb"), *out = fopen(dst, "wb");
	void (*fdct)(int *, JSAMPARRAY, JDIMENSION);
	int32_t n, k;
	int i, bw, bh;
	if (!strcmp(shape, "16x16")) { fdct = jpeg_fdct_16x16; bw = 16; bh = 16; }
	else if (!strcmp(shape, "16x8")) { fdct = jpeg_fdct_16x8; bw = 16; bh = 8; }
	else if (!strcmp(shape, "8x16")) { fdct = jpeg_fdct_8x16; bw = 8; bh = 16; }
	else { fprintf(stderr, "libjpeg9_compress_fancy: block shape %s\n", shape); return 2; }
	if (!in || !out || fread(&n, sizeof n, 1, in) != 1 || n < 0) return 1;
	for (k = 0; k < n; k++) {
		JSAMPLE s[256];
		JSAMPROW rows[16];
		int data[64];
		int32_t w[64];
		if (fread(s, (size_t)bw * bh, 1, in) != 1) return 1;
		for (i = 0; i < bh; i++) rows[i] = s + bw * i;
		fdct(data, rows, 0);
		for (i = 0; i < 64; i++) w[i] = data[i];
		fwrite(w, sizeof w, 1, out);
	}
	fclose(in);
	return fclose(out) != 0;
}

int main(int argc, char **argv) {
	if (argc == 4 && !strcmp(argv[1], "image")) return do_image(argv[2], argv[3]);
	if (argc == 5 && !strcmp(argv[1], "block")) return do_block(argv[2], argv[3], argv[4]);
	fprintf(stderr, "usage: libjpeg9_compress_fancy image in.bin out.jpg | block 16x16|16x8|8x16 in.bin out.bin\n");
	return 2;
}
