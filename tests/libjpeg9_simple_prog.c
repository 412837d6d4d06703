/*
 * libjpeg9_simple_prog.c -- TEST ORACLE for jpeg_file.simple_progression (tests/test_encode_refine_host.py): libjpeg 9's
 * own jpeg_simple_progression, with no code of this project or of the reference in the loop.
 *
 *   libjpeg9_simple_prog ncomp colorspace
 *
 * sets up a compress object of ncomp components in the J_COLOR_SPACE `colorspace` (jpeg_set_defaults +
 * jpeg_set_colorspace), calls jpeg_simple_progression and prints cinfo.scan_info, one scan per line:
 * "ncomp c0 c1 c2 c3 Ss Se Ah Al" (the format of tests/libjpeg9_encode.c's scripts).
 * Exit status: 0 printed; 3 libjpeg stopped with an error; 1 anything else.
 */
#include <stdio.h>
#include <stdlib.h>
#include <setjmp.h>
#include "jpeglib.h"

static jmp_buf on_error;

static void error_exit(j_common_ptr cinfo) {
	(*cinfo->err->output_message)(cinfo);
	longjmp(on_error, 1);
}

int main(int argc, char **argv) {
	struct jpeg_compress_struct co;
	struct jpeg_error_mgr err;
	int i, c, n, cs;
	if (argc != 3) { fprintf(stderr, "usage: libjpeg9_simple_prog ncomp colorspace\n"); return 1; }
	n = atoi(argv[1]);
	cs = atoi(argv[2]);
	if (n < 1 || n > 4) return 1;
	co.err = jpeg_std_error(&err);
	err.error_exit = error_exit;
	if (setjmp(on_error)) {
		jpeg_destroy_compress(&co);
		return 3;
	}
	jpeg_create_compress(&co);
	co.image_width = co.image_height = 16;
	co.input_components = n;
	co.in_color_space = (J_COLOR_SPACE)cs;
	jpeg_set_defaults(&co);
	jpeg_set_colorspace(&co, (J_COLOR_SPACE)cs);
	if (co.num_components != n) { fprintf(stderr, "libjpeg9_simple_prog: %d components\n", co.num_components); return 1; }
	jpeg_simple_progression(&co);
	for (i = 0; i < co.num_scans; i++) {
		const jpeg_scan_info *s = &co.scan_info[i];
		printf("%d", s->comps_in_scan);
		for (c = 0; c < 4; c++) printf(" %d", c < s->comps_in_scan ? s->component_index[c] : 0);
		printf(" %d %d %d %d\n", s->Ss, s->Se, s->Ah, s->Al);
	}
	jpeg_destroy_compress(&co);
	return 0;
}
