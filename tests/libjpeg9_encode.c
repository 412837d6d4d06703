/*
 * libjpeg9_encode.c -- TEST ORACLE for the device entropy coder, its restart intervals and its progressive files
 * (tests/test_encode_host.py, tests/test_encode_rst_host.py, tests/test_encode_prog_host.py and their GPU twins): libjpeg 9
 * itself, with no code of this project or of the reference in the loop.
 *
 *   libjpeg9_encode write in.bin out.jpg [optimize]
 *   libjpeg9_encode write in.bin out.jpg restart_interval restart_in_rows [optimize | script.txt]
 *
 * writes the coefficient arrays of in.bin (the format of tests/libjpeg9_decode.c) with jpeg_write_coefficients on a
 * fresh compress object: jpeg_set_defaults + jpeg_set_colorspace, the sampling factors and one quant table per
 * component from the file, the standard Huffman tables or, with `optimize`, optimize_coding; cinfo.restart_interval
 * and cinfo.restart_in_rows are the arguments (what jpegtran -restart sets; 0 where there are none), and with a script
 * cinfo.scan_info / num_scans are its lines (one scan each: "ncomp c0 c1 c2 c3 Ss Se Ah Al", what jpegtran -scans sets).
 * Exit status: 0 written; 3 libjpeg stopped with an error (its message on stderr); 2 bad arguments; 1 anything else.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <setjmp.h>
#include "jpeglib.h"

#define MAGIC 0x51534a43

static jmp_buf on_error;

static void error_exit(j_common_ptr cinfo) {
	(*cinfo->err->output_message)(cinfo);
	longjmp(on_error, 1);
}

static void *xread(FILE *f, size_t n) {
	void *p = malloc(n ? n : 1);
	if (!p || fread(p, 1, n, f) != n) { fprintf(stderr, "libjpeg9_encode: short input\n"); exit(1); }
	return p;
}

static jpeg_scan_info script[1024];
static int nscans, have_script;

static int do_write(const char *src, const char *dst, long ri, long rows, int optimize) {
	struct jpeg_compress_struct co;
	struct jpeg_error_mgr err;
	jvirt_barray_ptr arrays[4];
	FILE *in = fopen(src, "rb"), *out;
	int32_t hdr[5], g[4][5];
	uint16_t q[4][64];
	int16_t *blk[4];
	int c, i, n, maxh = 1, maxv = 1;
	if (!in) return 1;
	n = fread(hdr, sizeof hdr, 1, in) == 1 ? hdr[1] : 0;
	if (hdr[0] != MAGIC || n < 1 || n > 4) { fprintf(stderr, "libjpeg9_encode: bad header\n"); return 1; }
	for (c = 0; c < n; c++) {
		if (fread(g[c], sizeof g[c], 1, in) != 1 || fread(q[c], sizeof q[c], 1, in) != 1) return 1;
		if (g[c][2] > maxh) maxh = g[c][2];
		if (g[c][3] > maxv) maxv = g[c][3];
	}
	for (c = 0; c < n; c++) blk[c] = (int16_t *)xread(in, (size_t)g[c][0] * g[c][1] * 128);
	fclose(in);
	if (!(out = fopen(dst, "wb"))) return 1;

	co.err = jpeg_std_error(&err);
	err.error_exit = error_exit;
	if (setjmp(on_error)) {
		jpeg_destroy_compress(&co);
		fclose(out);
		return 3;
	}
	jpeg_create_compress(&co);
	jpeg_stdio_dest(&co, out);
	co.image_width = (JDIMENSION)hdr[2];
	co.image_height = (JDIMENSION)hdr[3];
	co.input_components = n;
	co.in_color_space = (J_COLOR_SPACE)hdr[4];
	jpeg_set_defaults(&co);
	jpeg_set_colorspace(&co, (J_COLOR_SPACE)hdr[4]);
	co.optimize_coding = optimize ? TRUE : FALSE;
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
			fprintf(stderr, "libjpeg9_encode: component %d has %dx%d blocks, the image needs %ldx%ld\n",
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
			/* blocks outside libjpeg's geometry hold a pattern, not zeros: the writer must not look at them */
			memset(r[0], 0x5a, (size_t)rw * sizeof(JBLOCK));
			if (y < hb) memcpy(r[0], blk[c] + (size_t)y * g[c][0] * 64, (size_t)wb * sizeof(JBLOCK));
		}
	}
	co.restart_interval = (unsigned int)ri;
	co.restart_in_rows = (int)rows;
	if (have_script) {
		co.scan_info = script;
		co.num_scans = nscans;
	}
	jpeg_write_coefficients(&co, arrays);
	jpeg_finish_compress(&co);
	jpeg_destroy_compress(&co);
	for (c = 0; c < n; c++) free(blk[c]);
	return fclose(out) != 0;
}

int main(int argc, char **argv) {
	const char *last = argc == 5 || argc == 7 ? argv[argc - 1] : NULL;     /* `optimize` or the script */
	int optimize = last && !strcmp(last, "optimize");
	if (argc >= 4 && argc <= 7 && !strcmp(argv[1], "write") && (argc != 5 || optimize)) {
		long ri = argc >= 6 ? strtol(argv[4], NULL, 10) : 0, rows = argc >= 6 ? strtol(argv[5], NULL, 10) : 0;
		FILE *f = last && !optimize ? fopen(last, "r") : NULL;
		jpeg_scan_info *s = script;
		if (ri < 0 || ri > 65535 || rows < 0 || rows > 65535 || (last && !optimize && !f)) {
			fprintf(stderr, "libjpeg9_encode: bad argument\n");
			return 2;
		}
		while (f && nscans < 1024 && fscanf(f, "%d %d %d %d %d %d %d %d %d", &s->comps_in_scan, &s->component_index[0],
				&s->component_index[1], &s->component_index[2], &s->component_index[3], &s->Ss, &s->Se, &s->Ah, &s->Al) == 9) {
			nscans++;
			s++;
		}
		if (f) {
			have_script = 1;
			fclose(f);
		}
		return do_write(argv[2], argv[3], ri, rows, optimize);
	}
	fprintf(stderr, "usage: libjpeg9_encode write in.bin out.jpg [optimize]\n"
			"       libjpeg9_encode write in.bin out.jpg restart_interval restart_in_rows [optimize | script.txt]\n");
	return 2;
}
