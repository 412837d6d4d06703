/*
 * libjpeg9_decode_scaled.c -- TEST ORACLE for the device decode at reduced sizes (tests/test_decode_scaled_host.py,
 * tests/test_gpu_decode_scaled.py): libjpeg 9 itself, with no code of this project or of the reference in the loop.
 *
 *   libjpeg9_decode_scaled decode in.bin out.raw DENOM   write in.bin with jpeg_write_coefficients to memory, decode that
 *                                                        with scale_num = 1, scale_denom = DENOM (JDCT_ISLOW, defaults)
 *   libjpeg9_decode_scaled block KIND in.bin out.bin     call jpeg_idct_<KIND> (4x4, 2x2, 1x1, 8x4, 4x2, 2x1, 4x8, 2x4,
 *                                                        1x2: width x height) directly on blocks
 *
 * in.bin of decode: the format of libjpeg9_decode.c (int32 magic, ncomp, image_width, image_height, colorspace; per
 * component int32 wblk, hblk, hsamp, vsamp, has_quant and uint16 quant[64]; then the components' blocks).
 * out.raw: int32 output_width, output_height, output_components, then output_height rows of samples.
 * block in.bin: int32 n, then n records of int16 coef[64] + uint16 table[64]; out.bin: n records of height x width samples.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "jpeglib.h"

#define MAGIC 0x51534a43

static void *xread(FILE *f, size_t n) {
	void *p = malloc(n ? n : 1);
	if (!p || fread(p, 1, n, f) != n) { fprintf(stderr, "libjpeg9_decode_scaled: short input\n"); exit(1); }
	return p;
}

static int do_decode(const char *src, const char *dst, int denom) {
	struct jpeg_compress_struct co;
	struct jpeg_decompress_struct de;
	struct jpeg_error_mgr err1, err2;
	jvirt_barray_ptr arrays[4];
	FILE *in = fopen(src, "rb"), *out;
	int32_t hdr[5], g[4][5], shape[3];
	uint16_t q[4][64];
	int16_t *blk[4];
	unsigned char *mem = NULL;
	unsigned long memsize = 0;
	JSAMPROW row;
	int c, i, n, maxh = 1, maxv = 1;
	if (!in) return 1;
	n = fread(hdr, sizeof hdr, 1, in) == 1 ? hdr[1] : 0;
	if (hdr[0] != MAGIC || n < 1 || n > 4) { fprintf(stderr, "libjpeg9_decode_scaled: bad header\n"); return 1; }
	for (c = 0; c < n; c++) {
		if (fread(g[c], sizeof g[c], 1, in) != 1 || fread(q[c], sizeof q[c], 1, in) != 1) return 1;
		if (g[c][2] > maxh) maxh = g[c][2];
		if (g[c][3] > maxv) maxv = g[c][3];
	}
	for (c = 0; c < n; c++) blk[c] = (int16_t *)xread(in, (size_t)g[c][0] * g[c][1] * 128);
	fclose(in);

	co.err = jpeg_std_error(&err1);
	jpeg_create_compress(&co);
	jpeg_mem_dest(&co, &mem, &memsize);
	co.image_width = (JDIMENSION)hdr[2];
	co.image_height = (JDIMENSION)hdr[3];
	co.input_components = n;
	co.in_color_space = (J_COLOR_SPACE)hdr[4];
	jpeg_set_defaults(&co);
	jpeg_set_colorspace(&co, (J_COLOR_SPACE)hdr[4]);
	/* what jpeg_copy_critical_parameters sets for a transcode */
	co.min_DCT_h_scaled_size = co.min_DCT_v_scaled_size = DCTSIZE;
	co.jpeg_width = co.image_width;
	co.jpeg_height = co.image_height;
	for (c = 0; c < n; c++) {
		JQUANT_TBL *t;
		co.comp_info[c].h_samp_factor = g[c][2];
		co.comp_info[c].v_samp_factor = g[c][3];
		co.comp_info[c].quant_tbl_no = c;
		if (!co.quant_tbl_ptrs[c]) co.quant_tbl_ptrs[c] = jpeg_alloc_quant_table((j_common_ptr)&co);
		t = co.quant_tbl_ptrs[c];
		for (i = 0; i < 64; i++) t->quantval[i] = g[c][4] ? q[c][i] : 1;
		t->sent_table = FALSE;
	}
	for (c = 0; c < n; c++) {       /* the block arrays libjpeg's own geometry asks for; the input may be larger */
		long wb = ((long)hdr[2] * g[c][2] + 8L * maxh - 1) / (8L * maxh);
		long hb = ((long)hdr[3] * g[c][3] + 8L * maxv - 1) / (8L * maxv);
		long rw = (wb + g[c][2] - 1) / g[c][2] * g[c][2], rh = (hb + g[c][3] - 1) / g[c][3] * g[c][3];
		if (wb > g[c][0] || hb > g[c][1]) {
			fprintf(stderr, "libjpeg9_decode_scaled: component %d has %dx%d blocks, the image needs %ldx%ld\n",
					c, g[c][0], g[c][1], wb, hb);
			return 1;
		}
		arrays[c] = (*co.mem->request_virt_barray)((j_common_ptr)&co, JPOOL_IMAGE, TRUE,
				(JDIMENSION)rw, (JDIMENSION)rh, (JDIMENSION)g[c][3]);
	}
	(*co.mem->realize_virt_arrays)((j_common_ptr)&co);
	for (c = 0; c < n; c++) {
		long wb = ((long)hdr[2] * g[c][2] + 8L * maxh - 1) / (8L * maxh);
		long hb = ((long)hdr[3] * g[c][3] + 8L * maxv - 1) / (8L * maxv);
		long rw = (wb + g[c][2] - 1) / g[c][2] * g[c][2], rh = (hb + g[c][3] - 1) / g[c][3] * g[c][3], y;
		for (y = 0; y < rh; y++) {
			JBLOCKARRAY r = (*co.mem->access_virt_barray)((j_common_ptr)&co, arrays[c], (JDIMENSION)y, 1, TRUE);
			memset(r[0], 0, (size_t)rw * sizeof(JBLOCK));
			if (y < hb) memcpy(r[0], blk[c] + (size_t)y * g[c][0] * 64, (size_t)wb * sizeof(JBLOCK));
		}
	}
	jpeg_write_coefficients(&co, arrays);
	jpeg_finish_compress(&co);
	jpeg_destroy_compress(&co);

	de.err = jpeg_std_error(&err2);
	jpeg_create_decompress(&de);
	jpeg_mem_src(&de, mem, memsize);
	jpeg_read_header(&de, TRUE);
	de.dct_method = JDCT_ISLOW;
	de.scale_num = 1;
	de.scale_denom = (unsigned int)denom;
	jpeg_start_decompress(&de);
	if (!(out = fopen(dst, "wb"))) return 1;
	shape[0] = (int32_t)de.output_width; shape[1] = (int32_t)de.output_height; shape[2] = de.output_components;
	fwrite(shape, sizeof shape, 1, out);
	row = (JSAMPROW)malloc((size_t)de.output_width * de.output_components);
	while (de.output_scanline < de.output_height) {
		jpeg_read_scanlines(&de, &row, 1);
		fwrite(row, 1, (size_t)de.output_width * de.output_components, out);
	}
	jpeg_finish_decompress(&de);
	jpeg_destroy_decompress(&de);
	free(row);
	free(mem);
	for (c = 0; c < n; c++) free(blk[c]);
	return fclose(out) != 0;
}

typedef void (*idct_fn)(j_decompress_ptr, jpeg_component_info *, JCOEFPTR, JSAMPARRAY, JDIMENSION);
/* exported by libjpeg 9 (jidctint.c), declared in its private jdct.h */
#define DECL(k) extern void jpeg_idct_##k(j_decompress_ptr, jpeg_component_info *, JCOEFPTR, JSAMPARRAY, JDIMENSION)
DECL(4x4); DECL(2x2); DECL(1x1); DECL(8x4); DECL(4x2); DECL(2x1); DECL(4x8); DECL(2x4); DECL(1x2);

static const struct { const char *kind; idct_fn fn; int w, h; } KINDS[] = {
	{ "4x4", jpeg_idct_4x4, 4, 4 }, { "2x2", jpeg_idct_2x2, 2, 2 }, { "1x1", jpeg_idct_1x1, 1, 1 },
	{ "8x4", jpeg_idct_8x4, 8, 4 }, { "4x2", jpeg_idct_4x2, 4, 2 }, { "2x1", jpeg_idct_2x1, 2, 1 },
	{ "4x8", jpeg_idct_4x8, 4, 8 }, { "2x4", jpeg_idct_2x4, 2, 4 }, { "1x2", jpeg_idct_1x2, 1, 2 },
};

static int do_block(const char *kind, const char *src, const char *dst) {
	/* a real decompressor, started on a tiny in-memory JPEG, so that sample_range_limit is libjpeg's own */
	struct jpeg_compress_struct co;
	struct jpeg_decompress_struct de;
	struct jpeg_error_mgr err1, err2;
	jpeg_component_info comp;
	unsigned char px[64], *mem = NULL;
	unsigned long memsize = 0;
	JSAMPROW r0 = px;
	JSAMPLE samples[8 * 8];
	JSAMPROW rows[8];
	int rcount = 0, ccount = 0, i, k, n;
	idct_fn fn = NULL;
	FILE *in, *out;
	int table[64];

	for (i = 0; i < (int)(sizeof KINDS / sizeof KINDS[0]); i++)
		if (!strcmp(kind, KINDS[i].kind)) { fn = KINDS[i].fn; ccount = KINDS[i].w; rcount = KINDS[i].h; }
	if (!fn) { fprintf(stderr, "libjpeg9_decode_scaled: unknown kind %s\n", kind); return 1; }

	memset(px, 128, sizeof px);
	co.err = jpeg_std_error(&err1);
	jpeg_create_compress(&co);
	jpeg_mem_dest(&co, &mem, &memsize);
	co.image_width = 8; co.image_height = 8; co.input_components = 1; co.in_color_space = JCS_GRAYSCALE;
	jpeg_set_defaults(&co);
	jpeg_start_compress(&co, TRUE);
	for (i = 0; i < 8; i++) jpeg_write_scanlines(&co, &r0, 1);
	jpeg_finish_compress(&co);
	jpeg_destroy_compress(&co);
	de.err = jpeg_std_error(&err2);
	jpeg_create_decompress(&de);
	jpeg_mem_src(&de, mem, memsize);
	jpeg_read_header(&de, TRUE);
	de.dct_method = JDCT_ISLOW;
	jpeg_start_decompress(&de);

	memset(&comp, 0, sizeof comp);
	comp = de.comp_info[0];
	comp.dct_table = table;
	for (i = 0; i < 8; i++) rows[i] = samples + 8 * i;
	if (!(in = fopen(src, "rb")) || !(out = fopen(dst, "wb"))) return 1;
	if (fread(&n, sizeof n, 1, in) != 1) return 1;
	for (k = 0; k < n; k++) {
		JCOEF coef[64];
		uint16_t t[64];
		if (fread(coef, sizeof coef, 1, in) != 1 || fread(t, sizeof t, 1, in) != 1) return 1;
		for (i = 0; i < 64; i++) table[i] = t[i];
		fn(&de, &comp, coef, rows, 0);
		for (i = 0; i < rcount; i++) fwrite(rows[i], 1, (size_t)ccount, out);
	}
	fclose(in);
	jpeg_abort_decompress(&de);
	jpeg_destroy_decompress(&de);
	free(mem);
	return fclose(out) != 0;
}

int main(int argc, char **argv) {
	if (argc == 5 && !strcmp(argv[1], "decode")) return do_decode(argv[2], argv[3], atoi(argv[4]));
	if (argc == 5 && !strcmp(argv[1], "block")) return do_block(argv[2], argv[3], argv[4]);
	fprintf(stderr, "usage: libjpeg9_decode_scaled decode in.bin out.raw DENOM | block KIND in.bin out.bin\n");
	return 2;
}
