/*
 * libjpeg9_decode.c -- TEST ORACLE for the device decode (tests/test_decode_host.py, tests/test_gpu_decode.py):
 * libjpeg 9 itself, with no code of this project or of the reference in the loop.
 *
 *   libjpeg9_decode read   in.jpg  out.bin     coefficient arrays + tables of a JPEG (jpeg_read_coefficients)
 *   libjpeg9_decode decode in.bin  out.raw     write in.bin with jpeg_write_coefficients to memory, decode that
 *                                              (JDCT_ISLOW, default upsampling and output colour space) to samples
 *   libjpeg9_decode block  KIND in.bin out.bin call jpeg_idct_<KIND> (islow, 16x16, 16x8, 8x16) directly on blocks
 *
 * in.bin / out.bin of read and decode (the format of tools/jpeg_coefs):
 *   int32 magic 0x51534a43, ncomp, image_width, image_height, colorspace;
 *   per component int32 wblk, hblk, hsamp, vsamp, has_quant; uint16 quant[64];
 *   then per component hblk * wblk blocks of 64 int16 (natural order, row-major)
 * out.raw: image_height rows of image_width * output_components samples.
 * block in.bin: int32 n, then n records of int16 coef[64] + uint16 table[64]; out.bin: n records of the IDCT's
 * output block (rows x cols samples, rows and cols from KIND).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "jpeglib.h"

#define MAGIC 0x51534a43

static void *xread(FILE *f, size_t n) {
	void *p = malloc(n ? n : 1);
	if (!p || fread(p, 1, n, f) != n) { fprintf(stderr, "libjpeg9_decode: short input\n"); exit(1); }
	return p;
}

static int do_read(const char *src, const char *dst) {
	struct jpeg_decompress_struct ci;
	struct jpeg_error_mgr err;
	FILE *in = fopen(src, "rb"), *out = fopen(dst, "wb");
	jvirt_barray_ptr *coefs;
	int32_t hdr[5];
	int c;
	if (!in || !out) return 1;
	ci.err = jpeg_std_error(&err);
	jpeg_create_decompress(&ci);
	jpeg_stdio_src(&ci, in);
	jpeg_read_header(&ci, TRUE);
	coefs = jpeg_read_coefficients(&ci);
	hdr[0] = MAGIC; hdr[1] = ci.num_components; hdr[2] = (int32_t)ci.image_width;
	hdr[3] = (int32_t)ci.image_height; hdr[4] = (int32_t)ci.jpeg_color_space;
	fwrite(hdr, sizeof hdr, 1, out);
	for (c = 0; c < ci.num_components; c++) {
		jpeg_component_info *comp = ci.comp_info + c;
		int32_t g[5] = { (int32_t)comp->width_in_blocks, (int32_t)comp->height_in_blocks,
				comp->h_samp_factor, comp->v_samp_factor, comp->quant_table != NULL };
		uint16_t q[64];
		int i;
		for (i = 0; i < 64; i++) q[i] = comp->quant_table ? comp->quant_table->quantval[i] : 0;
		fwrite(g, sizeof g, 1, out);
		fwrite(q, sizeof q, 1, out);
	}
	for (c = 0; c < ci.num_components; c++) {
		jpeg_component_info *comp = ci.comp_info + c;
		JDIMENSION y;
		for (y = 0; y < comp->height_in_blocks; y++) {
			JBLOCKARRAY row = (*ci.mem->access_virt_barray)((j_common_ptr)&ci, coefs[c], y, 1, FALSE);
			fwrite(row[0], sizeof(JBLOCK), comp->width_in_blocks, out);
		}
	}
	jpeg_finish_decompress(&ci);
	jpeg_destroy_decompress(&ci);
	fclose(in);
	return fclose(out) != 0;
}

static int do_decode(const char *src, const char *dst) {
	struct jpeg_compress_struct co;
	struct jpeg_decompress_struct de;
	struct jpeg_error_mgr err1, err2;
	jvirt_barray_ptr arrays[4];
	FILE *in = fopen(src, "rb"), *out;
	int32_t hdr[5], g[4][5];
	uint16_t q[4][64];
	int16_t *blk[4];
	unsigned char *mem = NULL;
	unsigned long memsize = 0;
	JSAMPROW row;
	int c, i, n, maxh = 1, maxv = 1;
	if (!in) return 1;
	n = fread(hdr, sizeof hdr, 1, in) == 1 ? hdr[1] : 0;
	if (hdr[0] != MAGIC || n < 1 || n > 4) { fprintf(stderr, "libjpeg9_decode: bad header\n"); return 1; }
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
	for (c = 0; c < n; c++) {       /* the block arrays libjpeg's own geometry asks for */
		long wb = ((long)hdr[2] * g[c][2] + 8L * maxh - 1) / (8L * maxh);
		long hb = ((long)hdr[3] * g[c][3] + 8L * maxv - 1) / (8L * maxv);
		long rw = (wb + g[c][2] - 1) / g[c][2] * g[c][2], rh = (hb + g[c][3] - 1) / g[c][3] * g[c][3];
		if (wb > g[c][0] || hb > g[c][1]) {
			fprintf(stderr, "libjpeg9_decode: component %d has %dx%d blocks, the image needs %ldx%ld\n",
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
	jpeg_start_decompress(&de);
	if (!(out = fopen(dst, "wb"))) return 1;
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
extern void jpeg_idct_islow(j_decompress_ptr, jpeg_component_info *, JCOEFPTR, JSAMPARRAY, JDIMENSION);
extern void jpeg_idct_16x16(j_decompress_ptr, jpeg_component_info *, JCOEFPTR, JSAMPARRAY, JDIMENSION);
extern void jpeg_idct_16x8(j_decompress_ptr, jpeg_component_info *, JCOEFPTR, JSAMPARRAY, JDIMENSION);
extern void jpeg_idct_8x16(j_decompress_ptr, jpeg_component_info *, JCOEFPTR, JSAMPARRAY, JDIMENSION);

static int do_block(const char *kind, const char *src, const char *dst) {
	/* a real decompressor, started on a tiny in-memory JPEG, so that sample_range_limit is libjpeg's own */
	struct jpeg_compress_struct co;
	struct jpeg_decompress_struct de;
	struct jpeg_error_mgr err1, err2;
	jpeg_component_info comp;
	unsigned char px[64], *mem = NULL;
	unsigned long memsize = 0;
	JSAMPROW r0 = px;
	JSAMPLE samples[16 * 16];
	JSAMPROW rows[16];
	int rcount = 8, ccount = 8, i, k, n;
	idct_fn fn;
	FILE *in, *out;
	int table[64];

	if (!strcmp(kind, "islow")) fn = jpeg_idct_islow;
	else if (!strcmp(kind, "16x16")) { fn = jpeg_idct_16x16; rcount = ccount = 16; }
	else if (!strcmp(kind, "16x8")) { fn = jpeg_idct_16x8; ccount = 16; }
	else if (!strcmp(kind, "8x16")) { fn = jpeg_idct_8x16; rcount = 16; }
	else { fprintf(stderr, "libjpeg9_decode: unknown kind %s\n", kind); return 1; }

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
	for (i = 0; i < 16; i++) rows[i] = samples + 16 * i;
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
	if (argc == 4 && !strcmp(argv[1], "read")) return do_read(argv[2], argv[3]);
	if (argc == 4 && !strcmp(argv[1], "decode")) return do_decode(argv[2], argv[3]);
	if (argc == 5 && !strcmp(argv[1], "block")) return do_block(argv[2], argv[3], argv[4]);
	fprintf(stderr, "usage: libjpeg9_decode read in.jpg out.bin | decode in.bin out.raw | block KIND in.bin out.bin\n");
	return 2;
}
