/*
 * jpegqs_hip.h -- flat C ABI of the MI355X (gfx950) implementation of
 * jpeg-quantsmooth's coefficient-recovery path.
 *
 * Two layers, both plain C (pointers + sizes, no libjpeg / torch types):
 *
 *  1. JOB LAYER  qs_hip_do_quantsmooth(): the whole of the reference's
 *     do_quantsmooth() (reference quantsmooth.h:2404-2878) on caller-owned HOST
 *     arrays -- same inputs (JCOEF blocks as jpeg_read_coefficients() returns
 *     them, quant tables, sampling factors, flags/niter/progress), same outputs
 *     (blocks rewritten in place, quant tables set to 1, return value = the
 *     reference's `stop`).  The libjpeg-facing drop-in (include/libjpegqs.h,
 *     csrc/jpegqs_shim.c) gathers JBLOCKROWs into these arrays and calls this.
 *
 *  2. PLANE LAYER  qs_hip_*_plane(): the individual GPU passes on DEVICE
 *     pointers and an explicit HIP stream, for callers that keep data resident
 *     in HBM (bench.py, the multi-GPU band driver, pipelines that decode on the
 *     GPU).  One call = one kernel launch, asynchronous on `stream`.
 *
 *  3. DEVICE JOB  qs_hip_do_quantsmooth_device(): the whole job of layer 1 on
 *     DEVICE arrays, enqueued on one stream without any host synchronisation
 *     (graph-capturable); the range-check stop is decided on the device.
 *     qs_hip_do_quantsmooth_device_batch(): many such jobs sharing launches.
 *
 * All functions return 0 on success and a negative QS_HIP_E* code on failure;
 * qs_hip_last_error() gives the message.  There is no CPU fallback: without a
 * usable HIP device every compute entry point fails with QS_HIP_ENODEV.
 */
#ifndef JPEGQS_HIP_H
#define JPEGQS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QS_HIP_MAXC 4

enum {
	QS_HIP_OK = 0,
	QS_HIP_ENODEV = -1,   /* no HIP device / runtime error */
	QS_HIP_EINVAL = -2,   /* bad argument */
	QS_HIP_ENOMEM = -3,   /* host or device allocation failed */
	QS_HIP_ENOTSUP = -4   /* flags this entry point does not implement (use the one that does) */
};

/* ---- job layer ---------------------------------------------------------- */

/* One image, as do_quantsmooth() sees it (reference quantsmooth.h:2423-2427,
 * 2447-2451, 2488-2493).  Layout is shared with the test oracles. */
typedef struct {
	int32_t ncomp;                     /* cinfo->num_components, 1..4 */
	int32_t colorspace;                /* cinfo->jpeg_color_space (1 gray, 3 YCbCr, ...) */
	int32_t image_width, image_height; /* cinfo->image_width/height */
	int32_t wblk[QS_HIP_MAXC];         /* comp_info[ci].width_in_blocks */
	int32_t hblk[QS_HIP_MAXC];         /* comp_info[ci].height_in_blocks */
	int32_t hsamp[QS_HIP_MAXC];        /* comp_info[ci].h_samp_factor */
	int32_t vsamp[QS_HIP_MAXC];        /* comp_info[ci].v_samp_factor */
	int32_t has_quant[QS_HIP_MAXC];    /* comp_info[ci].quant_table != NULL */
	uint16_t quant[QS_HIP_MAXC][64];   /* quantval[], natural order; set to 1 on return */
	int16_t *coef[QS_HIP_MAXC];        /* hblk*wblk blocks of 64 JCOEF, in/out */
	/* UPSAMPLE_UV only: replacement chroma arrays at luma resolution
	 * (reference :2696-2703, 2836-2849); owned by the caller, release with qs_hip_free()
	 * (NOT free(): large arrays are pinned buffers of the library's pool) */
	int16_t *coef_up[2];
	int32_t up_wblk, up_hblk;          /* 0 when chroma was not replaced */
	int32_t out_hsamp0, out_vsamp0;    /* component 0 sampling factors on return */
} qs_hip_job;

/* opts->progress of reference libjpegqs.h:41-45 */
typedef int (*qs_hip_progress_fn)(void *userdata, int cur, int max);

/* flags: JPEGQS_* algorithm bits (reference libjpegqs.h:16-23); niter, progprec,
 * progress, userdata: the jpegqs_control_t fields of the same names.
 * Returns the reference's `stop` (0 done, 1 cancelled/rejected input) or <0. */
int qs_hip_do_quantsmooth(qs_hip_job *job, int flags, int niter, int progprec,
		qs_hip_progress_fn progress, void *userdata);
/* The same job with every component's blocks given as separate ROWS: rows[ci][y] points at
 * wblk[ci] consecutive blocks of block row y -- what libjpeg's access_virt_barray hands out
 * (reference quantsmooth.h:2557-2560) -- and job->coef[ci] is ignored.  The rows are read and,
 * on success, rewritten in place; the library's helper threads gather them into / scatter them
 * from its pinned staging memory, so a libjpeg-facing caller needs no intermediate copy
 * (csrc/jpegqs_shim.c).  Rows must not overlap. */
int qs_hip_do_quantsmooth_rows(qs_hip_job *job, int16_t *const *const *rows, int flags, int niter,
		int progprec, qs_hip_progress_fn progress, void *userdata);
/* The same for many jobs in one call (one flags/niter setting for all).  Jobs whose
 * components are independent of each other (no JOINT_YUV / UPSAMPLE_UV coupling, no
 * LOW_QUALITY: CLI --quality 3 and 4) are processed TOGETHER: one pass-A and one
 * pass-B launch per iteration over all their planes, so small images fill the 256 CUs
 * as a group; YCbCr jobs coupled by JOINT_YUV / UPSAMPLE_UV (--quality 5 and 6) advance in groups
 * of about 200k blocks (all luma planes as one launch per pass, then all chroma planes), the rest
 * goes through qs_hip_do_quantsmooth -- groups and single jobs up to four at a time from helper
 * threads (their error text is not kept: results[i] carries the code).  results[i] =
 * what qs_hip_do_quantsmooth would have returned for jobs[i].  Returns 0, or < 0 when
 * the batch as a whole could not run (bad arguments, no device).  With several devices
 * configured (qs_hip_set_devices / QS_HIP_DEVICES) the jobs of a batch are spread
 * over them as whole jobs, balanced by block count: independent objects, no exchange.  Not part
 * of the reference API: an addition for callers that serve many images. */
int qs_hip_do_quantsmooth_batch(qs_hip_job *const *jobs, int njobs, int flags, int niter, int *results);

/* ---- several GPUs, one host process (the reference's counterpart is the
 * OpenMP row split INSIDE do_quantsmooth, reference quantsmooth.h:2587-2640) ----
 * A job of at least 512k blocks (QS_HIP_SHARD_MIN_BLOCKS) without a progress callback is cut
 * into one block-row band per device; each band stays on its GPU for the whole job and pulls one
 * pixel row per component from each neighbouring band after every pass A (hipMemcpyPeerAsync over
 * xGMI).  Bit-exact with the one-device result.  Both the independent-component flags (CLI
 * --quality 3/4) and the coupled YCbCr flags (--quality 5/6) are covered; anything else runs on
 * the current device.  OPT-IN: by default everything runs on the caller's current HIP device (a process
 * or thread per GPU is the usual deployment and must not find its jobs on other workers' GPUs).  The device
 * list is given by qs_hip_set_devices(), else by the environment variable QS_HIP_DEVICES ("all", or ordinals
 * such as "0,1,2,3"; read once per process); fewer than two entries = no sharding.  An ordinal may repeat (several bands on one GPU: how the route is
 * tested on a one-GPU box).  n = 0 returns to the default. */
int qs_hip_set_devices(const int *devices, int n);
/* How the bands of an independent-component job (CLI --quality 3/4) keep each other exact:
 *   0 (default)  one pixel row per band edge is exchanged after every pass A (niter small, latency-bound transfers);
 *   1            COMMUNICATION-AVOIDING: every cut side of a band carries `niter` block rows of its neighbour and
 *                all iterations run without any exchange -- the error made by treating the cut as an image edge
 *                moves one block row per iteration and never reaches the rows the band owns.  Costs 2 * niter block
 *                rows of extra work per inner band (+4.7 % at 8192 x 8192 over 8 devices, niter 3; +2.3 % at 16384^2).
 *  -1            back to the default (the environment variable QS_HIP_SHARD_SCHEDULE=deep also selects 1).
 * Both give the one-device result bit for bit.  Coupled YCbCr jobs (--quality 5/6) always use 0.
 * The reference's counterpart: the OpenMP row split of quantsmooth.h:2587-2640, which shares one pixel plane. */
int qs_hip_set_shard_schedule(int schedule);
/* the same job, cut over exactly these devices whatever its size (QS_HIP_ENOTSUP when the
 * flag / table combination has no sharded route; a progress callback is not available here) */
int qs_hip_do_quantsmooth_sharded(qs_hip_job *job, int flags, int niter, const int *devices, int ndev);

/* ---- several GPUs, ONE PROCESS PER GPU: the halo rows travel through RCCL ----
 * `job` is THIS rank's band: for every component the block rows the rank owns (hblk[ci] = rows of the band, cut with
 * qs_hip_band_rows so that the ranks' bands tile the image from top = rank 0 to bottom = rank nranks - 1), quant tables
 * and geometry as for qs_hip_do_quantsmooth.  After pass A and between the iterations the band sends its first / last
 * pixel row per component to rank - 1 / rank + 1 and receives theirs into its apron rows -- one ncclGroupStart /
 * ncclSend / ncclRecv (<= 4 per component) / ncclGroupEnd per iteration on the band's stream, no host synchronisation.
 * nccl_comm: the caller's ncclComm_t (RCCL), ranks numbered in band order; may be NULL when nranks == 1.  The library
 * does not link librccl: it uses the copy already loaded in the caller's process.
 * Independent components only (CLI --quality 3/4; QS_HIP_ENOTSUP otherwise), no progress callback.
 * Returns 0, a negative QS_HIP_E* code, or QS_HIP_BAND_RANGE_CHECK when a coefficient failed the reference's range check
 * on SOME rank (the flag is all-reduced): then no rank has written anything, and the image has to go through
 * qs_hip_do_quantsmooth as a whole, which applies the reference's stop semantics (quantsmooth.h:2599-2610).
 * The reference's counterpart is the OpenMP row split of quantsmooth.h:2587-2640, whose threads share the pixel plane.
 * (The communication-avoiding alternative needs no entry point: hand qs_hip_do_quantsmooth a band extended by niter
 *  block rows per cut side and keep the owned rows -- jpeg-quantsmooth_amd/bands.py: deep_band_rows.) */
#define QS_HIP_BAND_RANGE_CHECK 2
int qs_hip_do_quantsmooth_band(qs_hip_job *job, int flags, int niter, int rank, int nranks, void *nccl_comm);

/* The band arithmetic itself -- ONE definition, used by the in-process route above (csrc/qs_shard.cpp: halo rows
 * pulled with hipMemcpyPeerAsync) and by the one-process-per-GPU driver (bands.py: the same rows sent with RCCL):
 * block rows [*row0, *row1) of band `band` of `nbands` (edges on multiples of `align` block rows);
 * the luma / chroma row ranges of a band of a coupled YCbCr job (cut on chroma block rows, luma = the v_samp
 * times taller range of the same image rows; the last band takes the remaining luma rows);
 * and the byte offsets, inside a band's pixel plane, of the two rows it sends (first / last pixel row) and of
 * the two apron rows it receives into, each *nbytes long (reference quantsmooth.h:1396-1401 is what reads them). */
int qs_hip_band_rows(int hblk, int nbands, int band, int align, int *row0, int *row1);
int qs_hip_colour_band_rows(int hblk_luma, int hblk_chroma, int v_samp, int nbands, int band,
		int *y0, int *y1, int *c0, int *c1);
int qs_hip_band_halo_rows(int wblk, int hblk, size_t *send_top, size_t *send_bot,
		size_t *recv_top, size_t *recv_bot, size_t *nbytes);

/* The progress calls a job will make, as a function of its geometry (no device needed): the reference calls
 * progress(userdata, cur, max) after a pass B whenever its running block-row count crosses a threshold
 * (quantsmooth.h:2474-2482, 2656-2664); the pipelined routes of this library make exactly these calls, in this order,
 * each when at least that share of the work has completed.  Fills cur_out[0 .. min(n, max_calls)) and *max_out (the
 * `max` argument of every call) for a job whose components all run `niter` iterations (ordinary quant tables, no
 * cross-component flags); returns the number of calls n. */
int qs_hip_progress_calls(const qs_hip_job *geometry, int niter, int progprec, int *cur_out, int max_calls, int *max_out);

/* Optional, returns at once: bring the GPU side up IN THE BACKGROUND while the caller is still busy with something
 * else -- typically libjpeg's entropy decoding between jpeg_read_header() and jpeg_read_coefficients().  A fresh
 * process otherwise pays for the HIP runtime, the device context, the code object and the pinned staging buffers
 * inside its first do_quantsmooth (about 0.1 s for a full-HD image, 0.2-0.3 s for 8192 x 8192).  geometry: a job
 * whose ncomp / colorspace / wblk / hblk / hsamp / vsamp / has_quant / quant fields describe the coming call (coef
 * pointers are ignored; quant tables only decide the route), or NULL to start the runtime only.  The first job-layer
 * call waits for a prewarm still in flight.  Not in the reference API. */
int qs_hip_prewarm(const qs_hip_job *geometry, int flags, int niter);

/* ---- device-resident job (whole do_quantsmooth on DEVICE arrays, one stream) ----
 * The job layer above on coefficient arrays that already live in device memory (a GPU JPEG decoder, a PyTorch
 * pipeline): the same semantics bit for bit -- every flag combination, the refresh-only passes, the place of the
 * +-1023 clamp, JOINT_YUV / UPSAMPLE_UV, LOW_QUALITY and the reference's stop rules (quantsmooth.h:2404-2878).
 * Three calls:
 *   info     geometry + quant tables + flags + niter -> what the job needs (host only, no device touched);
 *   prepare  writes the per-component constant blocks and the range-check tables into the caller's device workspace;
 *            may synchronise `stream`, so it is called outside any graph capture, once per geometry + table set +
 *            flags + niter;
 *   run      ENQUEUES the job on `stream` and returns: no allocation, no synchronisation, no event or stream creation
 *            or query, no other stream (a capture of it is a linear graph), no copy from host memory, no buffer pool,
 *            no progress callback.  Graph-capturable.
 * The workspace (device memory, info.workspace_bytes, caller-owned) holds the pixel planes, the constants, the
 * range-check word and tables and a snapshot of the input; one job at a time may use it.  Its layout is a function of the job
 * and flags alone, so a run must see the geometry, tables, flags and niter its prepare saw.  The workspace is 256-byte
 * aligned, the coefficient arrays 16-byte aligned (what hipMalloc and torch's allocator hand out).
 * The range-check stop (reference :2596-2610) is decided on the device: a kernel zeroes the range-check word, a
 * precheck kernel snapshots the input and runs the reference's test before any pass; a fix-up kernel after the last
 * pass rebuilds the reference's result from the snapshot when a component tripped, and writes *d_stop (device int32),
 * the reference's return value, once the stream reaches the end of the job.  These three calls run the batch route
 * below with one job. */
typedef struct {
	size_t workspace_bytes;      /* device workspace the run needs (planes, constants, snapshot, range-check word) */
	int32_t up_wblk, up_hblk;    /* UPSAMPLE_UV: geometry of the two replacement chroma arrays, else 0 */
	int32_t out_hsamp0, out_vsamp0;   /* component 0 sampling factors of the result (1 x 1 when chroma is replaced) */
	int32_t static_stop;         /* 1 when the quant tables alone decide stop (a value >= 0x800, reference :2504) */
} qs_hip_device_info;
/* No device needed.  QS_HIP_EINVAL for a bad job. */
int qs_hip_device_job_info(const qs_hip_job *job, int flags, int niter, qs_hip_device_info *out);
int qs_hip_device_job_prepare(const qs_hip_job *job, int flags, int niter, void *d_workspace, size_t bytes, void *stream);
/* job->coef[ci] are DEVICE arrays of hblk * wblk * 64 JCOEF, rewritten in place.  When info.up_wblk > 0,
 * job->coef_up[0..1] must be caller-allocated DEVICE arrays of up_hblk * up_wblk * 64 JCOEF: they receive the
 * replacement chroma.  On return job->up_wblk / up_hblk / out_hsamp0 / out_vsamp0 are info's values and the quant
 * tables are set to 1 (as qs_hip_do_quantsmooth does); all of that, and coef_up, describes the result only when
 * *d_stop reads 0 -- when it reads 1 the reference drops the replacement chroma (:2835) and component 0 keeps its
 * sampling factors.  Returns 0 when the job was enqueued; QS_HIP_EINVAL for a short workspace, null pointers or
 * missing coef_up arrays; QS_HIP_ENODEV without a device. */
int qs_hip_do_quantsmooth_device(qs_hip_job *job, int flags, int niter, void *d_workspace, size_t bytes,
		int32_t *d_stop, void *stream);

/* ---- device-resident batch (many device-resident jobs, one stream) ----
 * The three calls above for njobs jobs at once, with one flags / niter setting for the whole batch (as
 * qs_hip_do_quantsmooth_batch).  The planes of the jobs share launches -- independent-component jobs (--quality 3/4) as
 * plane sets over all of them, coupled YCbCr jobs (JOINT_YUV / UPSAMPLE_UV) stage by stage -- and the range-check stop
 * is decided per job on the device by one precheck / fix-up pair for the whole batch, each job independent of the
 * others.  Every other job (LOW_QUALITY, tables with entries <= 1, a table-decided stop, niter 0) runs its own
 * component sequence on the same stream.  Results are those of qs_hip_do_quantsmooth_device job by job, bit for bit.
 *   info     per_job[i] = what qs_hip_device_job_info reports for jobs[i]; *workspace_bytes = the batch's workspace;
 *   prepare  the constants and descriptor tables into the workspace; may synchronise `stream`, never inside a capture;
 *   run      enqueues every job on `stream`, with the single-job run call's promises (graph-capturable, a linear graph).
 * The run call checks each job as qs_hip_do_quantsmooth_device does (the message names the job) and reports on each
 * job what it does (quant tables set to 1, up_* and out_*samp0).  d_stop: device int32[njobs]; d_stop[i] receives the
 * reference's return value for jobs[i].  QS_HIP_EINVAL also for njobs < 1, a null job and two jobs whose arrays
 * overlap.  The workspace serves one batch of this geometry, tables, flags and niter at a time. */
int qs_hip_device_batch_info(qs_hip_job *const *jobs, int njobs, int flags, int niter,
		qs_hip_device_info *per_job, size_t *workspace_bytes);
int qs_hip_device_batch_prepare(qs_hip_job *const *jobs, int njobs, int flags, int niter,
		void *d_workspace, size_t bytes, void *stream);
int qs_hip_do_quantsmooth_device_batch(qs_hip_job *const *jobs, int njobs, int flags, int niter,
		void *d_workspace, size_t bytes, int32_t *d_stop, void *stream);

/* ---- device decode to pixels (the coefficient arrays of device-resident jobs -> interleaved uint8 samples) ----
 * What libjpeg 9 hands out of jpeg_read_scanlines() for the same coefficient arrays, quant tables and sampling factors
 * (JDCT_ISLOW, the default do_fancy_upsampling -- libjpeg 9 upsamples 2x chroma by DCT scaling -- and the default
 * output colour space), bit for bit, over the whole int16 coefficient x uint16 quantiser domain.  Jobs are qs_hip_job
 * records over DEVICE arrays, typically those a qs_hip_do_quantsmooth_device[_batch] run has just reported on: their
 * quant tables (all ones after smoothing), coef, and for UPSAMPLE_UV coef_up / up_wblk / up_hblk.  Layouts:
 *   grayscale (1 component, colorspace 1, any sampling)                        -> height x width x 1
 *   YCbCr -> RGB (colorspace 3), chroma 1x1, luma 1x1, 2x1, 1x2, 2x2 or 4x1    -> height x width x 3
 *   RGB without a colour transform (colorspace 2), the same sampling           -> height x width x 3
 * anything else: QS_HIP_ENOTSUP.  image_width x image_height is required and is the output crop; each component
 * needs the blocks libjpeg's geometry gives it (width_in_blocks x height_in_blocks, QS_HIP_EINVAL otherwise).
 * A job with up_wblk > 0 has two geometries: the replacement chroma at luma resolution with 1x1 sampling (the reference's
 * result when its stop is 0) and the original chroma and sampling (stop 1, reference quantsmooth.h:2835).  With d_stop
 * (device int32[njobs], what the smoothing run wrote) the kernel picks one per job from d_stop[i]; with d_stop NULL
 * the replacement chroma is used.  Same three-call pattern as the device-resident job:
 *   info     per_job[i] = output shape and layout of jobs[i]; *workspace_bytes; no device touched;
 *   prepare  writes the per-job descriptors (geometry, tables) into the workspace; may synchronise `stream`, never
 *            inside a capture; once per geometry + table set (the layout does not depend on array addresses);
 *   run      ENQUEUES the decode on `stream`: one kernel launch per QS_HIP_DECODE_CHUNK jobs (the arrays and outputs
 *            travel in its arguments), no allocation, no synchronisation, no copy (graph-capturable).  It must see the
 *            geometry and tables prepare saw.
 * d_out[i]: device buffer of (height - 1) * out_pitch[i] + width * channels bytes, rows out_pitch[i] bytes apart;
 * only the samples of the image are written.  Arrays 16-byte aligned. */
#define QS_HIP_DECODE_CHUNK 44
typedef struct {
	int32_t width, height, channels;   /* output of job i: height rows of width * channels samples */
	int32_t layout;                    /* 0 grayscale, 1 YCbCr -> RGB, 2 RGB */
} qs_hip_decode_info;
int qs_hip_decode_device_batch_info(qs_hip_job *const *jobs, int njobs, qs_hip_decode_info *per_job,
		size_t *workspace_bytes);
int qs_hip_decode_device_batch_prepare(qs_hip_job *const *jobs, int njobs, void *d_workspace, size_t bytes,
		void *stream);
int qs_hip_decode_device_batch(qs_hip_job *const *jobs, int njobs, const int32_t *d_stop, uint8_t *const *d_out,
		const size_t *out_pitch, void *d_workspace, size_t bytes, void *stream);
/* The chroma upsampling, chosen per job through info / prepare with opts[i] for job i:
 *   QS_HIP_UPSAMPLE_DCT       libjpeg 7..9: 2x-subsampled chroma is upsampled by DCT scaling (jpeg_idct_16x16, _16x8,
 *                             _8x16), as described above.  What info / prepare without opts do.
 *   QS_HIP_UPSAMPLE_TRIANGLE  libjpeg-turbo and libjpeg 6b (what Pillow, OpenCV and browsers decode with): the 8x8
 *                             jpeg_idct_islow at chroma resolution, then jdsample.c's "fancy" triangle filters.  With c a
 *                             chroma plane of Wc x Hc = ceil(width / hs) x ceil(height / vs) samples, indices clamped to
 *                             0 .. Wc - 1 and 0 .. Hc - 1 (never to the block grid):
 *       luma 2x1   out[y][x] = (3 c[y][x>>1] + c[y][x even ? (x>>1) - 1 : (x>>1) + 1] + (x even ? 1 : 2)) >> 2
 *       luma 1x2   out[y][x] = (3 c[y>>1][x] + c[y even ? (y>>1) - 1 : (y>>1) + 1][x] + (y even ? 1 : 2)) >> 2
 *       luma 2x2   s[y][i]   = 3 c[y>>1][i] + c[y even ? (y>>1) - 1 : (y>>1) + 1][i]
 *                  out[y][x] = (3 s[y][x>>1] + s[y][x even ? (x>>1) - 1 : (x>>1) + 1] + (x even ? 8 : 7)) >> 4
 *       luma 4x1   each sample four times (turbo has no filter for it)
 *                             When Wc <= 2 the 2x1 and 2x2 filters are not used: each sample is replicated 2x1 / 2x2.
 *                             Luma, grayscale and 1x1 chroma samples are the same in both modes (one jpeg_idct_islow), so
 *                             for a job with replacement chroma (up_wblk > 0) the filters bear on the stop-1 geometry
 *                             alone.  YCbCr -> RGB takes turbo's jdcolor.c tables in this mode, in every layout and both
 *                             geometries: built from five-digit constants, they differ from libjpeg 9's in one entry
 *                             (FIX(0.34414) = 22554 against FIX(0.344136286) = 22553), which makes G one lower on a
 *                             few (Cb, Cr) pairs.
 *                             Bit for bit libjpeg-turbo's pixels wherever its C and SIMD code agree (its 16-bit SIMD
 *                             IDCT departs from jidctint.c on extreme coef * quantiser products; JSIMD_FORCENONE=1
 *                             selects the C code); outside that domain the mode is DEFINED as "the 8x8 islow of this
 *                             library (exact over the whole int16 x uint16 domain), then these filters".
 * opts NULL or opts[i] NULL is QS_HIP_UPSAMPLE_DCT, exactly info / prepare; any other value of `upsampling`:
 * QS_HIP_EINVAL before anything is enqueued.  A batch may mix modes; per_job and *workspace_bytes do not depend on the
 * mode.  The run call is unchanged, with all its promises: it works in the mode the last prepare wrote into the
 * workspace's descriptors. */
#define QS_HIP_UPSAMPLE_DCT      0   /* libjpeg 7..9: DCT-scaled chroma */
#define QS_HIP_UPSAMPLE_TRIANGLE 1   /* libjpeg-turbo / 6b: 8x8 islow + jdsample.c's fancy upsampling */
typedef struct {
	int32_t upsampling;   /* QS_HIP_UPSAMPLE_* */
} qs_hip_decode_opts;
int qs_hip_decode_device_batch_info_opts(qs_hip_job *const *jobs, int njobs, const qs_hip_decode_opts *const *opts,
		qs_hip_decode_info *per_job, size_t *workspace_bytes);
int qs_hip_decode_device_batch_prepare_opts(qs_hip_job *const *jobs, int njobs, const qs_hip_decode_opts *const *opts,
		void *d_workspace, size_t bytes, void *stream);
/* Reduced sizes, chosen per job through info / prepare with a second options record: what libjpeg 9 hands out with
 * scale_num = 1, scale_denom = 2, 4 or 8 (JDCT_ISLOW, defaults), bit for bit.  The output is
 * ceil(image_width * M / 8) x ceil(image_height * M / 8) samples with M = 8 / scale_denom, and libjpeg 9 sizes each
 * component's IDCT so that no chroma upsampling is left (widths x heights, as in jidctint.c's names):
 *   luma, grayscale, 1x1 chroma   M x M     jpeg_idct_4x4, _2x2, _1x1
 *   chroma under 2x2 luma         2M x 2M   jpeg_idct_islow, _4x4, _2x2
 *   chroma under 2x1 luma         2M x M    jpeg_idct_8x4, _4x2, _2x1
 *   chroma under 1x2 luma         M x 2M    jpeg_idct_4x8, _2x4, _1x2
 *   chroma under 4x1 luma         2M x M, then each column twice
 * Only the top-left coefficients those IDCTs take are read.  Layouts, arrays, d_stop and the two geometries of a job
 * with replacement chroma are those of the full-size decode.  per_job[i].width / height report the scaled output, so
 * buffers are sized from info as before.  opts NULL or opts[i] NULL: full size, QS_HIP_UPSAMPLE_DCT.  scale_denom
 * outside {1, 2, 4, 8}: QS_HIP_EINVAL.  QS_HIP_UPSAMPLE_TRIANGLE with scale_denom != 1: QS_HIP_ENOTSUP (a limit: at
 * reduced sizes libjpeg-turbo runs jidctred.c's own kernels before its filters, a contract this library does not
 * carry); libjpeg 9's other denominators (scale_num / scale_denom = k / 8 for k = 3, 5, 6, 7, 9 .. 16) are not offered
 * either.  One batch may mix denominators and, at denominator 1, both upsampling modes.  The run call is unchanged and
 * still makes launches only: at most two per QS_HIP_DECODE_CHUNK jobs (the chunk's full-size jobs, its reduced ones).
 * It takes the scales of the last prepare of d_workspace made through this library instance (the 256 most recently
 * prepared workspaces are remembered; any other runs at full size) and checks out_pitch against the scaled width. */
typedef struct {
	int32_t upsampling;   /* QS_HIP_UPSAMPLE_* */
	int32_t scale_denom;  /* 1, 2, 4 or 8 */
} qs_hip_decode_scale_opts;
int qs_hip_decode_device_batch_info_scaled(qs_hip_job *const *jobs, int njobs,
		const qs_hip_decode_scale_opts *const *opts, qs_hip_decode_info *per_job, size_t *workspace_bytes);
int qs_hip_decode_device_batch_prepare_scaled(qs_hip_job *const *jobs, int njobs,
		const qs_hip_decode_scale_opts *const *opts, void *d_workspace, size_t bytes, void *stream);

/* ---- device entropy coder (the coefficient arrays of device-resident jobs -> the bytes of a baseline JPEG scan) ----
 * What libjpeg 9 writes between the SOS header and EOI when jpeg_write_coefficients gets the same arrays (jchuff.c:
 * sequential Huffman, no scan script, 8-bit precision; restart intervals through the _opts calls below), byte for
 * byte: one interleaved scan over all
 * components (MCUs in raster order; blocks an edge MCU lacks are coded as jctrans.c's dummy blocks), or one
 * non-interleaved scan for a one-component image; the last byte padded with one-bits, 0x00 after every 0xFF.  Jobs are
 * qs_hip_job records over DEVICE arrays as the decode takes them: each array contiguous and 16-byte aligned
 * (QS_HIP_EINVAL otherwise: an offset view of a larger buffer may not be), quant tables not needed; colour spaces 1
 * (grayscale), 2 (RGB), 3 (YCbCr), 4 (CMYK), 5 (YCCK); more than 10 blocks in an MCU: QS_HIP_ENOTSUP.  A job with
 * up_wblk > 0 has the decode's two geometries, chosen per job on the device from d_stop[i] (NULL: replacement chroma).
 * Component ci uses DC and AC table dc_tbl[ci] = ac_tbl[ci]: what jpeg_set_colorspace assigns (table 1 for the chroma of
 * YCbCr and YCCK, table 0 otherwise).  The same three-call pattern:
 *   info       per_job[i] and *workspace_bytes; no device touched.  The workspace holds the unstuffed stream at its
 *              worst-case size (208 bytes per block), so it is larger than the coefficient arrays;
 *   prepare    geometry and Huffman code tables into the workspace; tables: NULL, or per job NULL or a qs_hip_huff_tables --
 *              a table whose has_* byte is 0 is the standard table of JPEG Annex K.3 (libjpeg's default); may synchronise
 *              `stream`, never inside a capture;
 *   run        ENQUEUES seven kernel launches per QS_HIP_ENCODE_CHUNK jobs on `stream`: no allocation, no
 *              synchronisation, no copy (graph-capturable, a linear graph).
 * d_out[i]: device buffer of out_capacity[i] bytes; nothing is written at or beyond the capacity.  d_len[i] (device
 * uint64): the bytes the segment needs.  d_status[i] (device int32): 0 ok; 1 a coefficient libjpeg refuses with
 * JERR_BAD_DCT_COEF (an AC value of more than 10 bits, a DC difference of more than 11); 2 out_capacity[i] < d_len[i]
 * (d_len is exact: retry with that size); 3 a symbol without a code in the tables given.  With 1 or 3 d_len[i] is 0 and
 * the buffer's content unspecified.
 *   histogram  the symbol counts of the same scan: d_counts = device uint32[njobs][4][257], tables in the order DC 0,
 *              DC 1, AC 0, AC 1; entry 256 is libjpeg's reserved pseudo-symbol and reads 1.  d_status[i]: 0 or 1. */
#define QS_HIP_ENCODE_CHUNK 32
typedef struct {
	uint8_t bits[17];      /* bits[l] = codes of length l (1..16), as in a DHT marker */
	uint8_t huffval[256];  /* the symbols in order of increasing code length */
} qs_hip_huff_table;
typedef struct {
	qs_hip_huff_table dc[2], ac[2];
	uint8_t has_dc[2], has_ac[2];   /* 0: the standard table instead */
} qs_hip_huff_tables;
typedef struct {
	int32_t dc_tbl[QS_HIP_MAXC], ac_tbl[QS_HIP_MAXC];   /* table of each component */
	int32_t blocks_in_mcu[2];      /* of the two geometries (equal when the job has one) */
	uint64_t max_segment_bytes;    /* no segment of this job is longer */
} qs_hip_encode_info;
int qs_hip_encode_device_batch_info(qs_hip_job *const *jobs, int njobs, qs_hip_encode_info *per_job,
		size_t *workspace_bytes);
int qs_hip_encode_device_batch_prepare(qs_hip_job *const *jobs, int njobs, const qs_hip_huff_tables *const *tables,
		void *d_workspace, size_t bytes, void *stream);
int qs_hip_encode_device_batch(qs_hip_job *const *jobs, int njobs, const int32_t *d_stop, uint8_t *const *d_out,
		const size_t *out_capacity, uint64_t *d_len, int32_t *d_status, void *d_workspace, size_t bytes, void *stream);
int qs_hip_encode_device_batch_histogram(qs_hip_job *const *jobs, int njobs, const int32_t *d_stop, uint32_t *d_counts,
		int32_t *d_status, void *d_workspace, size_t bytes, void *stream);
/* Restart intervals, as libjpeg 9 writes them for cinfo.restart_interval / cinfo.restart_in_rows (jpegtran -restart
 * N[B]): restart_interval in MCUs, 0 .. 65535, 0 = none; restart_in_rows > 0 wins and means min(restart_in_rows * MCUs per row,
 * 65535), worked out for each of a job's geometries (an MCU of a one-component scan is one block).  Before MCU k * Ri
 * (k >= 1) the pending bits are padded to a byte with one-bits (a padded byte of 0xFF is followed by 0x00 like any
 * other), FF D0+((k-1) & 7) follows unstuffed, and every component's DC prediction starts again at 0 -- in the segment
 * and in the histogram alike.  An interval that covers the scan writes no marker: the segment of a job without one.
 * (The DRI marker of the file is the caller's: libjpeg writes FF DD 00 04 Ri in front of SOS whenever Ri is not 0.)
 *   info_opts / prepare_opts   info / prepare with opts[i] for job i; opts NULL or opts[i] NULL: no restarts, which is
 *              what info / prepare do.  max_segment_bytes and *workspace_bytes cover the options (at most 4 bytes per
 *              interval end; the intervals' offsets live in the workspace), so a workspace sized for other options may
 *              be too small: QS_HIP_EINVAL, as for any short workspace.  A negative value or restart_interval > 65535:
 *              QS_HIP_EINVAL.
 * The run and histogram calls keep their signatures: they work with the intervals the last prepare on d_workspace
 * wrote there.  The library remembers, per workspace address, what prepare saw (the 4096 workspaces prepared last).
 * A workspace the run finds no prepare for -- a copy of a prepared one at another address, say -- runs without
 * restarts, as before; a job of it whose descriptor has a restart interval then ends with d_status 4 and d_len 0
 * (prepare the workspace at the address it runs at).  A run with another number of jobs than that prepare saw:
 * QS_HIP_EINVAL.  A launch chunk without a restart job enqueues exactly the kernels it would without options; one
 * with a restart job enqueues seven as well, in their restart variants. */
typedef struct {
	int32_t restart_interval, restart_in_rows;
} qs_hip_encode_opts;
int qs_hip_encode_device_batch_info_opts(qs_hip_job *const *jobs, int njobs, const qs_hip_encode_opts *const *opts,
		qs_hip_encode_info *per_job, size_t *workspace_bytes);
int qs_hip_encode_device_batch_prepare_opts(qs_hip_job *const *jobs, int njobs, const qs_hip_huff_tables *const *tables,
		const qs_hip_encode_opts *const *opts, void *d_workspace, size_t bytes, void *stream);
/* ---- optimal tables and whole files on the device ----
 * The device twin of qs_hip_huff_optimal (below): d_counts = device uint32[ntables][257] (entry 256 is ignored: the
 * reserved symbol always counts 1), d_tables[ntables] receives bits / huffval as qs_hip_huff_optimal gives them,
 * d_status[t] = 0, or 5 for a code length above 32 (libjpeg's JERR_HUFF_CLEN_OVERFLOW, where the host function returns
 * QS_HIP_EINVAL; bits and huffval are then all 0).  One launch on `stream`, one wave per table, no workspace, no
 * allocation, no synchronisation (graph-capturable). */
int qs_hip_huff_optimal_device(const uint32_t *d_counts, int ntables, qs_hip_huff_table *d_tables,
		int32_t *d_status, void *stream);
/* Whole files: d_out[i] receives head | DHT markers | mid | segment | FF D9 -- the file libjpeg 9 writes -- and d_len[i]
 * its length.  The bytes around the tables and the scan are the caller's (jpeg_file.compose_parts composes them), per
 * job and per geometry variant (variant 1 is used where the coder uses its second geometry: a job with up_wblk > 0 whose
 * d_stop reads non-zero); DEVICE memory, any alignment. */
typedef struct {
	const uint8_t *d_head[2]; uint32_t head_bytes[2];   /* SOI .. SOF (and, without optimize, the DHT markers) */
	const uint8_t *d_mid[2];  uint32_t mid_bytes[2];    /* [DRI] SOS header */
} qs_hip_encode_frame;
/* The DHT markers are written by the run, and only with optimize != 0: one per table the job's components use, in
 * jcmarker.c's order (per component DC then AC, each table once: DC 0, AC 0, DC 1, AC 1 for YCbCr), each FF C4, length,
 * Tc/Th, 16 counts, the symbols; the tables are libjpeg's optimize_coding tables for the scan (qs_hip_huff_optimal on the
 * histogram, both taken on the device), and the segment is coded with them.  optimize == 0: the segment of
 * qs_hip_encode_device_batch, coded with prepare's tables, whose DHT markers the caller puts at the end of the head.
 * frames == NULL: no head, no mid and no EOI -- d_out[i] receives the DHT markers (if any) and the segment.
 * The workspace is the encode workspace, used exactly as qs_hip_encode_device_batch uses it: the same info and prepare
 * calls (restart intervals through the _opts calls), the same size; the run does not write the tables prepare put there,
 * so a plain qs_hip_encode_device_batch on the same workspace afterwards gives the bytes it gave before.  Everything new
 * lives in d_scratch (256-byte aligned, qs_hip_encode_files_scratch_bytes(njobs) bytes): the counts, the derived code
 * words, the tables, each job's prefix length and table status.
 * Per QS_HIP_ENCODE_CHUNK jobs the run ENQUEUES, with optimize: the three launches of the histogram call (counting into
 * the scratch), the table kernel (one wave per table, four per job; a table no component uses is skipped), the seven coder
 * launches (reading their codes from the scratch) and one framing launch; without: the seven coder launches and the
 * framing launch.  No allocation, no synchronisation, no copy from host memory, no other stream; a capture is a linear
 * graph; nothing is stored at or beyond out_capacity[i], framing bytes included.
 * d_len[i]: the length of the whole file.  d_status[i]: as qs_hip_encode_device_batch, plus 5 for a table with a code
 * length above 32; precedence 4, 1, 5, 2 (3 cannot occur with optimize).  With 1, 3, 4 or 5 d_len[i] is 0 and the buffer
 * unspecified; with 2 d_len[i] is exact and the buffer holds the file's first out_capacity[i] bytes.
 * d_tables (device, [njobs], may be NULL): with optimize, the tables of each job; has_* is 0 for a table no component
 * uses.  After status 5 the table whose code lengths pass 32 has has_* 1 and bits and huffval all 0, as
 * qs_hip_huff_optimal_device leaves it, and the job's other tables are the valid ones of their counts.  With
 * status 1 the tables are those of the counts with each refused value clamped to 10 bits (a DC difference to 11) --
 * all 0 again where they pass 32; with status 4 they are unspecified.  Untouched without optimize.
 * QS_HIP_EINVAL before anything is enqueued: a job whose frames[i] lacks a variant it can take (no SOS header bytes, or a
 * null pointer with a non-zero length; variant 1 counts for a job with two geometries when d_stop is given), and a
 * scratch that is null, misaligned or short. */
size_t qs_hip_encode_files_scratch_bytes(int njobs);
int qs_hip_encode_device_batch_files(qs_hip_job *const *jobs, int njobs, const qs_hip_encode_frame *frames,
		int optimize, const int32_t *d_stop, uint8_t *const *d_out, const size_t *out_capacity, uint64_t *d_len,
		int32_t *d_status, qs_hip_huff_tables *d_tables /* device, [njobs], may be NULL */,
		void *d_scratch, size_t scratch_bytes, void *d_workspace, size_t bytes, void *stream);
/* ---- progressive files (spectral selection, and successive approximation behind a flag) on the device ----
 * d_out[i] receives the PROGRESSIVE file libjpeg 9 writes for jpeg_write_coefficients with cinfo.scan_info set to the
 * job's script, and d_len[i] its length: head (SOI .. SOF2, the caller's: jpeg_file.compose_parts(progressive=True)),
 * then per scan the DHT markers of that scan's own optimal tables (progressive mode forces optimize_coding; a DC scan
 * writes the DC tables of its components, an AC scan the AC table of its component, each table once, in component
 * order, directly in front of the scan's SOS), DRI whenever the scan's interval differs from the last one written (0 at
 * the start), the SOS header and the entropy-coded segment, then EOI.
 * A script is what libjpeg's validate_script accepts as progressive with Ah = 0 in every scan: scans in any component
 * order, not necessarily every coefficient, an AC scan (1 <= Ss <= Se <= 63) with one component and behind a DC scan
 * (Ss = Se = 0) of that component, every component with a DC scan, Al within 0 .. 10 (such a script has at most
 * QS_HIP_MAX_SCANS scans).
 * Anything libjpeg refuses: QS_HIP_EINVAL from info and prepare, naming the scan -- a scan that interleaves more than 10
 * blocks per MCU included (the frame as a whole may have more: libjpeg's limit is per scan).  A script libjpeg accepts
 * that has a refinement scan (Ah > 0): QS_HIP_ENOTSUP, naming the scan ("refinement scans are not implemented"), unless
 * the job's opts->flags has QS_HIP_PROG_REFINE (below).
 * A script libjpeg accepts as sequential multi-scan (the first scan is 0 .. 63): QS_HIP_ENOTSUP.
 * flags = QS_HIP_PROG_REFINE: every script libjpeg accepts as progressive is written, refinement scans included, up to
 * QS_HIP_MAX_SCANS scans (a valid longer script: QS_HIP_ENOTSUP; any other flag bit: QS_HIP_EINVAL).  DC refinement (Ss =
 * Se = 0, Ah > 0): one bit per block, (coef[0] >> Al) & 1, a dummy block repeating the bit before it; no symbols, so no
 * DHT marker, and its SOS names table 0 for every component (jcmarker.c emit_sos).  AC refinement (Ss >= 1, Ah > 0):
 * with a = |c| >> Al, a coefficient with a == 1 is newly nonzero -- symbol (run << 4) | 1 and its sign bit, with 0xF0 per
 * 16 zeros in front of it -- one with a > 1 sends the correction bit a & 1 behind the next symbol of the block, or, behind
 * the block's last symbol, with the EOB run: the run's symbol is followed by the buffered correction bits of all its
 * blocks, and it is written in front of the next block with a newly nonzero coefficient, at a restart boundary, at the
 * end, at 0x7FFF blocks or once more than 937 bits are buffered.  No range check: status 1 cannot arise in such a scan.
 * Worst case per block 1 bit and (Se - Ss + 1) * 17 + 14 bits.  A chunk of pairs with a refinement scan adds 7 + R
 * launches, R = ceil(log2(ceil(blocks of the longest restart interval or scan / 15))) rounds of pointer doubling, which
 * follows from the geometry alone.
 * DC scan: the value coded is coef[0] >> Al (arithmetic), the difference goes to the previous block of the component in
 * scan order; several components are interleaved in the coder's MCU order with its dummy blocks, one component runs
 * over width_in_blocks x height_in_blocks.  A category above 11: status 1.  AC scan: blocks in raster order over
 * width_in_blocks x height_in_blocks, per coefficient |c| >> Al with the sign put back, run/size symbols with 0xF0 per
 * 16 zeros, more than 10 bits after the shift: status 1; a block that ends in zeros inside the band adds 1 to the EOB
 * run, which is written (symbol n << 4, n = floor(log2 run), and the low n bits) in front of the next symbol, at every
 * restart boundary, at 0x7FFF and at the end of the scan.  Restart intervals count in the scan's own MCUs (one block in
 * a one-component scan; restart_in_rows in the scan's MCU rows), as libjpeg's per_scan_setup does.
 * component_id: the ids the SOS headers name (they must be the head's); all 0: jpeg_set_colorspace's for the job's colour
 * space.  Huffman table slots are jpeg_set_colorspace's, as everywhere in the coder.
 *   info     per job the number of scans, each scan's MCU count and the interval DRI carries (geometry variant 0), and
 *            max_body_bytes: a bound on the file's length without its head.  *workspace_bytes and *scratch_bytes: what
 *            prepare and the run need (both 256-byte aligned device memory).  The unstuffed stream of a scan is sized by
 *            its own worst case per block: 27 bits in a DC scan, (Se - Ss + 1) * 26 + 30 in an AC scan (csrc/
 *            qs_encode_prog.h).
 *   prepare  writes the scan jobs' descriptors and every scan's DRI / SOS bytes into the workspace (synchronises
 *            `stream`; not inside a capture) and remembers the plan under the workspace's address.
 *   files    ENQUEUES the run on `stream`: no allocation, no synchronisation, no copy from host memory, no other stream;
 *            a capture is a linear graph whose launch count follows from the batch and the scripts alone.  The unit of
 *            work is a (job, scan) pair; all pairs of the batch go through the coder's stages side by side, in chunks
 *            of QS_HIP_ENCODE_CHUNK pairs: 1 launch per chunk of jobs, then per chunk of pairs 11 (state and histogram
 *            reset, block flags, head scan, EOB runs, histogram, the table kernel, sizes, bit scan, emit, the two
 *            stuffing counts), then 1 framing launch per chunk of jobs and 1 stuffing launch per chunk of pairs.
 *            frames[i]: d_head / head_bytes per geometry variant (d_mid is not looked at); variant 1 is used where the
 *            whole-file run uses it (up_wblk > 0 and d_stop[i] != 0; d_stop NULL: variant 0).
 *            d_status[i]: 0; 1 a refused coefficient in any scan; 5 a table whose code lengths pass 32; 2 capacity;
 *            4 a workspace the run finds no prepare for (every job of the batch) -- precedence 4, 1, 5, 2.  With 1, 4
 *            or 5 d_len[i] is 0 and the buffer unspecified; with 2 d_len[i] is exact and the buffer holds the file's
 *            first out_capacity[i] bytes.  Nothing is stored at or beyond out_capacity[i].
 *            A run with another number of jobs than the prepare saw: QS_HIP_EINVAL. */
#define QS_HIP_MAX_SCANS 256
#define QS_HIP_PROG_REFINE 1
typedef struct {
	int32_t ncomp, comp[4];            /* comps_in_scan, component_index[] (frame order) */
	int32_t Ss, Se, Ah, Al;
} qs_hip_encode_scan;                  /* = jpeg_scan_info */
typedef struct {
	const qs_hip_encode_scan *scans;
	int32_t nscans;
	int32_t restart_interval, restart_in_rows;
	int32_t component_id[QS_HIP_MAXC];
	int32_t flags;                     /* 0, or QS_HIP_PROG_REFINE: refinement scans (Ah > 0) are written */
} qs_hip_encode_prog_opts;
typedef struct {
	int32_t nscans;
	int32_t mcus[QS_HIP_MAX_SCANS], interval[QS_HIP_MAX_SCANS];
	uint64_t max_body_bytes;
} qs_hip_encode_prog_info;
int qs_hip_encode_progressive_device_batch_info(qs_hip_job *const *jobs, int njobs,
		const qs_hip_encode_prog_opts *const *opts, qs_hip_encode_prog_info *per_job, size_t *workspace_bytes,
		size_t *scratch_bytes);
int qs_hip_encode_progressive_device_batch_prepare(qs_hip_job *const *jobs, int njobs,
		const qs_hip_encode_prog_opts *const *opts, void *d_workspace, size_t bytes, void *stream);
int qs_hip_encode_progressive_device_batch_files(qs_hip_job *const *jobs, int njobs, const qs_hip_encode_frame *frames,
		const int32_t *d_stop, uint8_t *const *d_out, const size_t *out_capacity, uint64_t *d_len, int32_t *d_status,
		void *d_scratch, size_t scratch_bytes, void *d_workspace, size_t bytes, void *stream);
/* ---- device scan reader (the bytes of a JPEG scan with restart intervals -> device-resident coefficient arrays) ----
 * What libjpeg 9 leaves in its coefficient arrays after jpeg_read_coefficients (jdhuff.c decode_mcu: the DC prediction
 * runs as int and is stored as JCOEF, AC values by HUFF_EXTEND, de-zigzagged), for ONE sequential Huffman scan (SOF0 /
 * SOF1, 8 bits) that carries all components of the frame in frame order.  One lane reads one restart interval: the
 * reader is parallel over the intervals and over nothing else, so a file without DRI is read by a single lane.
 * Jobs are qs_hip_job records over the DEVICE arrays to fill: coef[ci] with wblk as the row stride and wblk x hblk
 * blocks, contiguous and 16-byte aligned; each must hold at least libjpeg's width_in_blocks x height_in_blocks
 * (QS_HIP_EINVAL otherwise).  Quant tables and the colour space are not looked at.  More than 10 blocks in an MCU:
 * QS_HIP_ENOTSUP.  An interval -- restart_interval MCUs, or the whole scan when that is 0 or at least the MCU count --
 * of more than QS_HIP_READ_MAX_INTERVAL_BLOCKS blocks: QS_HIP_ENOTSUP from info, before anything is enqueued (the cap
 * is one MCU row of the widest legal JPEG, 65 500 pixels at 4:4:4 = 24 564 blocks, rounded up; it bounds how long one
 * lane runs).  The same three-call pattern:
 *   info     per_job[i] and *workspace_bytes; no device touched;
 *   prepare  geometry and derived code tables into the workspace; opts[i] is required: tables by DHT id 0..3 (a table
 *            whose has_* byte is 0 is the Annex K.3 table for ids 0 / 1; a component that uses an id 2 / 3 without
 *            one: QS_HIP_EINVAL), Td / Ta of each component, the DRI value; may synchronise `stream`, never inside a
 *            capture;
 *   run      ENQUEUES five kernel launches per QS_HIP_READ_CHUNK jobs on `stream`: no allocation, no synchronisation,
 *            no copy (graph-capturable, a linear graph).  It must see the geometry prepare saw.
 * d_scan[i]: device memory (any alignment) holding the file from the first byte behind the SOS header; scan_bytes[i]:
 * how many bytes may be read there.  The kernels find the end themselves -- the first FF xx with xx not in {00,
 * D0..D7}; EOI and anything behind it are ignored -- and look no further than the longest segment the geometry can have.
 * Every block the scan codes is written if its position lies inside the caller's array: in an interleaved scan the
 * dummy blocks of edge MCUs count as coded, as jdcoefct.c keeps them in libjpeg's own padded virtual arrays (so an
 * array with wblk > width_in_blocks receives them); a one-component scan codes width_in_blocks x height_in_blocks
 * blocks.  Every other block of the array is set to 0: the output is a function of the input alone.
 * d_status[i] (device int32): 0 ok; 1 the number or order of the RSTn markers does not match the restart interval
 * (marker k must be RST((k - 1) & 7)); 2 an interval ran out of bytes before its blocks were done, or had one or more
 * whole bytes left over; 3 a bit pattern without a code, or a zero run that passes coefficient 63.  With a non-zero
 * status the arrays' content is unspecified, every store lies inside them, and other jobs are unaffected.  Matching
 * libjpeg's output on corrupt data (it warns and carries on) is not attempted. */
#define QS_HIP_READ_CHUNK 32
#define QS_HIP_READ_MAX_INTERVAL_BLOCKS 32768
typedef struct {
	qs_hip_huff_table dc[4], ac[4];
	uint8_t has_dc[4], has_ac[4];                        /* 0: the standard table (ids 0 / 1 only) */
	int32_t dc_tbl[QS_HIP_MAXC], ac_tbl[QS_HIP_MAXC];    /* Td / Ta of each component */
	int32_t restart_interval;                            /* MCUs, from DRI; 0: none */
} qs_hip_read_opts;
typedef struct {
	int32_t blocks_in_mcu, mcus, intervals;
	int64_t blocks_per_interval;
} qs_hip_read_info;
int qs_hip_read_device_batch_info(qs_hip_job *const *jobs, int njobs, const qs_hip_read_opts *const *opts,
		qs_hip_read_info *per_job, size_t *workspace_bytes);
int qs_hip_read_device_batch_prepare(qs_hip_job *const *jobs, int njobs, const qs_hip_read_opts *const *opts,
		void *d_workspace, size_t bytes, void *stream);
int qs_hip_read_device_batch(qs_hip_job *const *jobs, int njobs, const uint8_t *const *d_scan, const uint64_t *scan_bytes,
		int32_t *d_status, void *d_workspace, size_t bytes, void *stream);
/* The split route of the scan reader: the same jobs, options, arguments and output as the three calls above, parallel
 * inside an interval as well, so a file without DRI is read by many lanes and there is no interval cap (the other
 * refusals are the same).  Every restart interval -- the whole scan when the file has none -- is cut into segments of
 * QS_HIP_READ_SPLIT_BYTES stuffed bytes and one lane decodes one segment.  The first segment of an interval starts in
 * the known state; every other one starts from a guess and takes, in each of QS_HIP_READ_SPLIT_ROUNDS further launches,
 * the state its left neighbour reached in the launch before (Huffman streams synchronise themselves).  Then every link
 * is checked: only when each segment was decoded from exactly the state its neighbour ended in are the values
 * written, and the DC predictions rebuilt from the differences by a prefix sum (mod 2^16: libjpeg's int prediction
 * stored as JCOEF).  For every input the calls above read with status 0 the arrays and the status are the same.
 * d_status[i]: 0..3 as above (0 and 1 for exactly the inputs that get them there; which of 2 and 3 a damaged interval
 * gets may differ), and 4: the segments did not synchronise in QS_HIP_READ_SPLIT_ROUNDS rounds -- the arrays are
 * unspecified, every store lies inside them, other jobs are unaffected; the three calls above read such a file.  No
 * valid file of the corpus the constant was measured on comes near it.
 * per_job[i].max_segments: the segments the workspace is sized for, those of the longest scan the geometry can have.
 * The run ENQUEUES 4 + 7 + QS_HIP_READ_SPLIT_ROUNDS + 1 kernel launches per QS_HIP_READ_CHUNK jobs on `stream`, a fixed
 * number: no allocation, no synchronisation, no copy (graph-capturable, a linear graph).  The workspace is not the one
 * of the calls above. */
#define QS_HIP_READ_SPLIT_BYTES 256
#define QS_HIP_READ_SPLIT_ROUNDS 17
typedef struct {
	int32_t blocks_in_mcu, mcus, intervals;
	int64_t blocks_per_interval;
	int64_t max_segments;
} qs_hip_read_split_info;
int qs_hip_read_split_device_batch_info(qs_hip_job *const *jobs, int njobs, const qs_hip_read_opts *const *opts,
		qs_hip_read_split_info *per_job, size_t *workspace_bytes);
int qs_hip_read_split_device_batch_prepare(qs_hip_job *const *jobs, int njobs, const qs_hip_read_opts *const *opts,
		void *d_workspace, size_t bytes, void *stream);
int qs_hip_read_split_device_batch(qs_hip_job *const *jobs, int njobs, const uint8_t *const *d_scan,
		const uint64_t *scan_bytes, int32_t *d_status, void *d_workspace, size_t bytes, void *stream);
/* The progressive route of the scan reader: the bytes of a whole PROGRESSIVE Huffman file (SOF2, 8 bits) in device memory
 * -> the coefficient arrays libjpeg 9's jpeg_read_coefficients leaves (jdhuff.c decode_mcu_DC_first / _AC_first /
 * _DC_refine / _AC_refine, jdcoefct.c consume_data).  The jobs are the ones of the calls above; the options carry what a
 * host-side walk over the file's markers found (jpeg_file.parse_progressive): per scan the jpeg_scan_info record, Td / Ta
 * of its components, the DHT tables and the DRI value in effect at its SOS, and the offset of the first byte behind its
 * SOS header.  The unit of work is a (job, scan) pair, and one lane decodes one restart interval of one scan.
 * A scan depends on every earlier scan of the file that shares a component with it and whose band [Ss, Se] overlaps its
 * own; its level is 0 if it depends on nothing, else 1 + the largest level it depends on, and the run makes one decode
 * launch per level (libjpeg's ten-scan YCbCr script: three).  Parallelism comes from restart intervals, independent scans
 * and the batch and from nothing else: a file without DRI is read by one lane per scan.  No self-synchronisation inside
 * an interval (an AC refinement scan cannot have it).
 * Rules: DC first -- the prediction runs as int from 0 in every interval, per scan component, the store is (JCOEF)(pred
 * << Al); AC first -- HUFF_EXTEND << Al at zz[k], EOB runs (r < 15, s = 0: (1 << r) + r more bits; this block and the next
 * run - 1 blocks are done), cleared at every interval start; DC refinement -- one bit per block, coef[0] |= 1 << Al, no
 * table; AC refinement -- decode_mcu_AC_refine: a new coefficient has s = 1 and a sign bit, every already non-zero
 * coefficient passed over takes one correction bit, applied only if (coef & (1 << Al)) == 0 and away from zero.  An
 * interleaved scan keeps the frame's MCU grid and writes the dummy blocks of edge MCUs where the array has room for
 * them; a one-component scan runs raster over width_in_blocks x height_in_blocks.  Every block no scan codes is 0.
 * Refusals, from info, before anything is enqueued: a script libjpeg's validate_script refuses QS_HIP_EINVAL naming the
 * scan; one it takes as sequential multi-scan, more than QS_HIP_MAX_SCANS scans, more than 10 blocks in an MCU of an
 * interleaved scan, or an interval of more than QS_HIP_READ_MAX_INTERVAL_BLOCKS blocks in any scan -- counted in that
 * scan's own MCUs, one block per MCU in a one-component scan -- QS_HIP_ENOTSUP; a scan that uses a table its record does
 * not hold QS_HIP_EINVAL (a DC scan uses Td of each component, an AC scan Ta of its one, a DC refinement none).
 *   info     per job nscans, levels and per scan mcus / intervals; *workspace_bytes; no device touched;
 *   prepare  the pairs' descriptors (geometry, derived code tables, offsets) and the level lists into the workspace, and
 *            the plan under the workspace's address; may synchronise `stream`, never inside a capture;
 *   run      ENQUEUES launches only (graph-capturable, a linear graph): per chunk of QS_HIP_READ_CHUNK jobs 1 (arrays
 *            zeroed), 4 per 32 pairs (the scans' ends and RSTn markers), 1 (checks) and one decode launch per level.
 *            A workspace never prepared, or prepared for another number of jobs: QS_HIP_EINVAL.
 * d_file[i]: device memory (any alignment) holding the whole file; file_bytes[i]: how many bytes may be read there --
 * every read is bounded by it.  The scans' offsets are fixed at prepare, like the tables of the calls above: a run (or a
 * graph replay) on another file of the same header layout reads that file; on a file whose scans do not start at the
 * prepared offsets it ends with a non-zero status (the SOS header in front of every prepared offset is compared with
 * the scan's record: status 1), never with an access outside the file or the arrays.
 * d_status[i] (device int32), the largest over all scans and lanes of the job: 0 ok; 1 the RSTn count or order of a scan
 * does not fit its interval, or a scan does not start at its prepared offset (no scan of such a job is decoded); 2 an
 * interval ran short or has a whole byte left over, or no marker ends a scan (the file stops inside it); 3 a bit pattern
 * without a code, a run passing Se, s != 1 in an AC refinement, or an EOB run longer than the blocks left in its
 * interval.  libjpeg only warns on, or silently accepts, some of these.  With a non-zero status the arrays' content is
 * unspecified, every store lies inside them, and other jobs are unaffected. */
typedef struct {
	qs_hip_encode_scan scan;                             /* comps_in_scan, component_index[] (frame order), Ss, Se, Ah, Al */
	int32_t dc_tbl[QS_HIP_MAXC], ac_tbl[QS_HIP_MAXC];    /* Td / Ta of each scan component */
	qs_hip_huff_table dc[4], ac[4];                      /* the DHT tables in effect at this SOS, by id */
	uint8_t has_dc[4], has_ac[4];
	int32_t restart_interval;                            /* the DRI in effect, in this scan's MCUs; 0: none */
	uint64_t offset;                                     /* of the first byte behind the SOS header, in the file */
} qs_hip_read_prog_scan;
typedef struct {
	const qs_hip_read_prog_scan *scans;
	int32_t nscans;
} qs_hip_read_prog_opts;
typedef struct {
	int32_t nscans, levels;
	int32_t mcus[QS_HIP_MAX_SCANS], intervals[QS_HIP_MAX_SCANS];
} qs_hip_read_prog_info;
int qs_hip_read_prog_device_batch_info(qs_hip_job *const *jobs, int njobs, const qs_hip_read_prog_opts *const *opts,
		qs_hip_read_prog_info *per_job, size_t *workspace_bytes);
int qs_hip_read_prog_device_batch_prepare(qs_hip_job *const *jobs, int njobs, const qs_hip_read_prog_opts *const *opts,
		void *d_workspace, size_t bytes, void *stream);
int qs_hip_read_prog_device_batch(qs_hip_job *const *jobs, int njobs, const uint8_t *const *d_file,
		const uint64_t *file_bytes, int32_t *d_status, void *d_workspace, size_t bytes, void *stream);
/* Host only.  The optimal table for symbol counts freq[0..255] (freq[256] is ignored: the reserved symbol always counts
 * 1) by the procedure of JPEG Annex K.2 as libjpeg 9 carries it out: what optimize_coding writes into its DHT.  Counts
 * that are all zero: bits all 0, no symbols, success.  A code length above 32: QS_HIP_EINVAL.  (csrc/qs_huff.h: the
 * procedure of the table kernel, in its host form.) */
int qs_hip_huff_optimal(const uint32_t freq[257], uint8_t bits[17], uint8_t huffval[256]);
/* Host only.  The standard table of Annex K.3: is_ac 0 / 1, tbl 0 (luminance) / 1 (chrominance). */
int qs_hip_huff_standard(int is_ac, int tbl, uint8_t bits[17], uint8_t huffval[256]);

/* ---- device compress (interleaved uint8 pixels in device memory -> the quantised coefficient arrays of device-resident jobs) ----
 * The inverse of the device decode: the arrays libjpeg 9 holds after jpeg_write_scanlines() -- what jpeg_read_coefficients()
 * returns for the file it writes -- for the same pixels, quant tables, sampling factors and colour space, bit for bit, with
 *   dct_method = JDCT_ISLOW, smoothing_factor = 0 and either chroma downsampling of libjpeg 9, chosen per job:
 *   QS_HIP_DOWNSAMPLE_BOX  do_fancy_downsampling = FALSE: box-filter chroma downsampling (jcsample.c), then the 8x8
 *                          jpeg_fdct_islow for every component.  What info / prepare without opts do.
 *   QS_HIP_DOWNSAMPLE_DCT  do_fancy_downsampling = TRUE, libjpeg 9's default (cjpeg, jpeg_set_defaults): 2x-subsampled
 *                          chroma goes through 16-point scaled forward DCTs instead of a box -- jpeg_fdct_16x16 of the
 *                          full-resolution samples for luma 2x2, jpeg_fdct_16x8 for 2x1, jpeg_fdct_8x16 for 1x2, the h2v1
 *                          box and then jpeg_fdct_16x8 for 4x1 -- and gives other chroma coefficients wherever chroma is
 *                          subsampled.  Luma, grayscale and 1x1 chroma are the same in both modes.  The inverse of the
 *                          device decode's chroma upsampling.  Through the _opts calls below.
 * OUT OF SCOPE: smoothing_factor != 0 and the other DCT methods (JDCT_IFAST, JDCT_FLOAT).
 * The `fancy` argument of info / prepare keeps its meaning: anything but 0 is QS_HIP_ENOTSUP (use the _opts calls).
 * Jobs are qs_hip_job records as the decode takes them, with coef[ci] the DEVICE arrays to FILL (wblk as the row stride,
 * 16-byte aligned), quant tables required (1 .. 65535, natural order, one per component; a 0: QS_HIP_EINVAL) and
 * image_width x image_height required.  Layouts, derived from ncomp and colorspace as in qs_hip_decode_info:
 *   grayscale (1 component, colorspace 1, taken as 1x1)                              <- height x width x 1
 *   RGB -> YCbCr (colorspace 3), chroma 1x1, luma 1x1, 2x1, 1x2, 2x2 or 4x1          <- height x width x 3
 *   RGB without a colour transform (colorspace 2), the same sampling                 <- height x width x 3
 * anything else: QS_HIP_ENOTSUP before anything is enqueued.  Each array must hold at least libjpeg's width_in_blocks x
 * height_in_blocks (QS_HIP_EINVAL otherwise; info reports them); exactly these blocks are written -- the blocks of a
 * larger array outside libjpeg's geometry (the dummy blocks of edge MCUs among them) are left as they are.  Edges follow
 * libjpeg: the right edge is replicated before downsampling; at the bottom the image is padded to a multiple of
 * max_v_samp rows with its last row, downsampled, and then the last DOWNSAMPLED row of each component is repeated (BOX);
 * the components that DCT scales take plain clamps, source column min(x, width - 1) and source row min(y, height - 1).
 * The same three-call pattern:
 *   info     per_job[i] = input shape, layout and block geometry of jobs[i]; *workspace_bytes; no device touched;
 *   prepare  writes the per-job descriptors (geometry, tables, their reciprocals) into the workspace; may synchronise
 *            `stream`, never inside a capture; once per geometry + table set;
 *   run      ENQUEUES the compress on `stream`: one kernel launch per QS_HIP_COMPRESS_CHUNK jobs (the pixels and arrays
 *            travel in its arguments), no allocation, no synchronisation, no copy (graph-capturable).  It must see the
 *            geometry and tables prepare saw.
 * d_pixels[i]: device buffer (any alignment) of (height - 1) * pitch[i] + width * channels bytes, rows pitch[i] >= width *
 * channels bytes apart; nothing else is read. */
#define QS_HIP_COMPRESS_CHUNK 44
typedef struct {
	int32_t width, height, channels;   /* input of job i: height rows of width * channels samples */
	int32_t layout;                    /* 0 grayscale, 1 RGB -> YCbCr, 2 RGB */
	int32_t wblk[QS_HIP_MAXC], hblk[QS_HIP_MAXC];   /* libjpeg's width_in_blocks / height_in_blocks: what is written */
} qs_hip_compress_info;
int qs_hip_compress_device_batch_info(qs_hip_job *const *jobs, int njobs, int fancy, qs_hip_compress_info *per_job,
		size_t *workspace_bytes);
int qs_hip_compress_device_batch_prepare(qs_hip_job *const *jobs, int njobs, int fancy, void *d_workspace, size_t bytes,
		void *stream);
int qs_hip_compress_device_batch(qs_hip_job *const *jobs, int njobs, const uint8_t *const *d_pixels, const size_t *pitch,
		void *d_workspace, size_t bytes, void *stream);
/* info / prepare with opts[i] for job i: opts NULL or opts[i] NULL is QS_HIP_DOWNSAMPLE_BOX, exactly info / prepare
 * with fancy = 0.  Any other value of `downsampling`, or a non-zero `reserved`: QS_HIP_EINVAL.  A batch may mix modes;
 * geometry (per_job, *workspace_bytes) does not depend on the mode.  The run call is unchanged: it works in the mode
 * the last prepare wrote into the workspace's descriptors. */
#define QS_HIP_DOWNSAMPLE_BOX 0   /* do_fancy_downsampling = FALSE */
#define QS_HIP_DOWNSAMPLE_DCT 1   /* libjpeg 9's default: 2x chroma through 16-point scaled forward DCTs */
typedef struct {
	int32_t downsampling;   /* QS_HIP_DOWNSAMPLE_* */
	int32_t reserved[3];    /* 0 */
} qs_hip_compress_opts;
int qs_hip_compress_device_batch_info_opts(qs_hip_job *const *jobs, int njobs, const qs_hip_compress_opts *const *opts,
		qs_hip_compress_info *per_job, size_t *workspace_bytes);
int qs_hip_compress_device_batch_prepare_opts(qs_hip_job *const *jobs, int njobs, const qs_hip_compress_opts *const *opts,
		void *d_workspace, size_t bytes, void *stream);

void qs_hip_free(void *p);
/* the job layer keeps freed device buffers (up to 6 GiB per device), pinned staging buffers (up
 * to 2 GiB) and HIP streams in process-wide caches, each entry tied to the device it was created
 * on and handed out only to callers whose current HIP device is that one (a host thread may
 * hipSetDevice() to any GPU before calling the job layer); this returns them to the driver.
 * qs_hip_do_quantsmooth_batch keeps at most QS_HIP_GROUP_WINDOW (6) groups of about 200k blocks
 * in flight, so its memory does not grow with the size of the batch.  (It also
 * starts eight helper threads on first use, for the host side of large transfers; they
 * sleep between jobs and live until the process ends.) */
void qs_hip_release_cache(void);

/* ---- plane layer (device pointers, async on `stream`) --------------------- */

int qs_hip_device_count(void);
const char *qs_hip_last_error(void);
/* Version of this interface: bumped whenever a struct layout or the meaning of an argument changes (5: round 5 --
 * qs_hip_plane_ref back to its 48-byte form, second planes through qs_hip_smooth_planes_next; 6: round 6 --
 * additions only: qs_hip_set_shard_schedule, the RCCL band entry points; 7: additions only -- the device-resident job,
 * qs_hip_device_info and its three calls, the device batch calls, qs_hip_decode_info and the device decode, the device entropy coder, the device scan reader, the device compress,
 * qs_hip_huff_optimal_device and the whole-file run qs_hip_encode_device_batch_files, the _opts calls of the compress,
 * the split route of the scan reader qs_hip_read_split_device_batch and its two calls, the _opts calls of the decode,
 * its _scaled calls with qs_hip_decode_scale_opts,
 * the progressive route of the scan reader qs_hip_read_prog_device_batch and its two calls).
 * A caller built against
 * this header can compare QS_HIP_ABI_VERSION with what the loaded library reports. */
#define QS_HIP_ABI_VERSION 7
int qs_hip_abi_version(void);

/* bytes of the per-component constant block; pixel-plane pitch and size */
size_t qs_hip_consts_bytes(void);
size_t qs_hip_plane_pitch(int wblk);
size_t qs_hip_plane_bytes(int wblk, int hblk);
/* byte offset of pixel (x = -QS apron .. , y) helpers for halo exchange:
 * row y (y = -1 .. hblk*8) of the plane starts at qs_hip_plane_row_offset(wblk, y)
 * and is qs_hip_plane_pitch(wblk) bytes long (apron columns included). */
size_t qs_hip_plane_row_offset(int wblk, int y);

/* Build the constant block for one component on the host (quant-derived values,
 * reference :2497-2540, and the weight tables, reference :251-301) into
 * `host_out` (qs_hip_consts_bytes() bytes); the caller copies it to the device. */
int qs_hip_consts_build(void *host_out, const uint16_t quant[64], int flags);

/* pass A: [first: dequantise + range check ->*d_status |= 1] IDCT into the plane
 * (reference :2589-2620).  first: 0, 1, or 1 | QS_HIP_FIRST_DEFER (see QS_HIP_PLANE_DEFER below).  rep_top/rep_bot: fill the y=-1 / y=h apron rows by
 * replication (0 when they are halo rows owned by a neighbouring band). */
int qs_hip_idct_plane(const void *d_consts, int16_t *d_coef, uint8_t *d_plane,
		int wblk, int hblk, int first, int rep_top, int rep_bot,
		int32_t *d_status, void *stream);

/* pass B: per-block recovery loop + rebalance (+ final clamp)
 * (reference :2627-2640 -> quantsmooth_block :564-1849; clamp :2668-2689).
 * Supported here: flags & (DIAGONALS | NO_REBALANCE | NO_REBALANCE_UV). */
int qs_hip_smooth_plane(const void *d_consts, int16_t *d_coef, const uint8_t *d_plane,
		int wblk, int hblk, int flags, int luma, int final_clamp, void *stream);
/* pass B that ALSO writes the pixel plane of the next iteration (pass A of iteration n + 1 fused into pass B of
 * iteration n: the kernel holds the block's final coefficients anyway).  d_plane_next must be a second plane of the
 * same geometry -- the other blocks of the launch still read d_plane -- and receives exactly what
 * qs_hip_idct_plane(first = 0, rep_top, rep_bot) would write after this call.  Reference :2589-2620 + :2627-2640. */
int qs_hip_smooth_plane_next(const void *d_consts, int16_t *d_coef, const uint8_t *d_plane, uint8_t *d_plane_next,
		int wblk, int hblk, int flags, int luma, int final_clamp, int rep_top, int rep_bot, void *stream);
/* the same for block rows [row0, row1) only: a band runs its interior rows while
 * the halo rows are still in flight and its first/last row afterwards */
int qs_hip_smooth_rows(const void *d_consts, int16_t *d_coef, const uint8_t *d_plane,
		int wblk, int hblk, int row0, int row1, int flags, int luma, int final_clamp, void *stream);

/* pass A / pass B over a SET of whole planes in one launch (any mix of sizes and quant
 * tables: the components of a job, or of many small jobs).  luma: as in
 * qs_hip_smooth_plane; d_status: the plane's range-check flag (pass A, first iteration). */
#define QS_HIP_MAX_PLANES 56
typedef struct {
	const void *d_consts;
	int16_t *d_coef;
	uint8_t *d_plane;
	int32_t *d_status;
	int32_t wblk, hblk, luma;
	int32_t band;  /* 0: a whole plane.  Bit 0 / bit 1: the plane is a band of block rows whose top /
	                * bottom apron row is a halo row received from the neighbouring band (pass A leaves it alone).
	                * Bit 2 (QS_HIP_PLANE_DEFER): deferred dequantisation, see below */
} qs_hip_plane_ref;   /* 48 bytes, unchanged since the plane-set calls appeared: every field must be set by the caller */
/* Deferred dequantisation (opt-in, per plane).  By default pass A of iteration 0 (first = 1) stores the dequantised
 * coefficients back to d_coef, and whoever looks at d_coef afterwards sees them.  A caller that runs the first pass A
 * and then, with NO reader of d_coef in between, the first qs_hip_smooth_planes[_next] launch over the same plane can
 * set QS_HIP_PLANE_DEFER in `band` for exactly these two calls: pass A then dequantises, range-checks (*d_status)
 * and writes the pixel plane as always but leaves d_coef as it found it (a third of the pass's memory traffic less),
 * and the smoothing launch forms the same products while it loads the coefficients.  What is in d_coef and in the
 * planes after the smoothing launch is byte for byte what the default gives.  The bit means "d_coef is still
 * quantised" to the smoothing launch: it must be clear in every later call.  qs_hip_idct_planes ignores it when
 * first = 0.  The single-plane pass A takes the same request as first = 1 | QS_HIP_FIRST_DEFER (the launch that
 * consumes it is a plane-set launch with QS_HIP_PLANE_DEFER; the single-plane smoothing calls have no such form). */
#define QS_HIP_PLANE_DEFER 4
#define QS_HIP_FIRST_DEFER 2
int qs_hip_idct_planes(const qs_hip_plane_ref *refs, int n, int first, void *stream);
int qs_hip_smooth_planes(const qs_hip_plane_ref *refs, int n, int flags, int final_clamp, void *stream);
/* qs_hip_smooth_planes that ALSO writes the next iteration's pixel planes (see qs_hip_smooth_plane_next):
 * d_plane_next[i] is the second plane of refs[i] -- same geometry, a different buffer -- or NULL for a plane that gets
 * none; d_plane_next == NULL is qs_hip_smooth_planes.  The second planes travel in a PARALLEL array on purpose: the
 * struct above keeps its size and stride, so callers compiled against an earlier header (who neither zero nor know a
 * trailing field) stay correct. */
int qs_hip_smooth_planes_next(const qs_hip_plane_ref *refs, uint8_t *const *d_plane_next, int n, int flags,
		int final_clamp, void *stream);

/* JOINT_YUV chroma predictor + fdct_clamp for one chroma plane (reference :577-579,
 * 893-921, 343-347, 551-561); d_luma_lowres = luma at this plane's resolution and
 * geometry.  rebalance/final_clamp: run them here (LOW_QUALITY chroma, which skips
 * the recovery loop) instead of in qs_hip_smooth_plane. */
int qs_hip_joint_plane(const void *d_consts, int16_t *d_coef, const uint8_t *d_plane,
		const uint8_t *d_luma_lowres, int wblk, int hblk,
		int rebalance, int final_clamp, void *stream);
/* LOW_QUALITY pass B: range filter + fdct_clamp + rebalance (reference :924-938, 1161-1178) */
int qs_hip_lowq_plane(const void *d_consts, int16_t *d_coef, const uint8_t *d_plane,
		int wblk, int hblk, int rebalance, int final_clamp, void *stream);
/* box-downsample the luma plane by ws x hs into a plane of lwblk x lhblk blocks,
 * replicated out to its edges and apron (reference :2753-2815) */
int qs_hip_downsample_plane(const uint8_t *d_luma, int ywblk, int yhblk, uint8_t *d_lowres,
		int lwblk, int lhblk, int ws, int hs, void *stream);
/* UPSAMPLE_UV: chroma plane -> full-resolution pixel buffer (pitch/size from the two
 * helpers), guided by luma (reference :1851-2393, 2714-2730); then qs_hip_fdct_plane
 * re-encodes it into ywblk x yhblk blocks (reference :2735-2750) */
size_t qs_hip_upsample_pitch(int image_width, int ws);
size_t qs_hip_upsample_bytes(int image_width, int image_height, int ws, int hs);
int qs_hip_upsample_plane(const uint8_t *d_chroma, const uint8_t *d_luma_lowres, int cwblk,
		const uint8_t *d_luma, int ywblk, int yhblk, uint8_t *d_pixels,
		int image_width, int image_height, int ws, int hs, void *stream);
/* the same with explicit geometry, for one band of a sharded image: w1 = chroma
 * width in pixels (image level), h1 = valid low-res rows in this band, first_rows =
 * how many of its leading rows belong to the image's first 8-row strip (they get
 * the reference's right-edge replicate, :2390-2393), pitch = row pitch of d_pixels */
int qs_hip_upsample_rows(const uint8_t *d_chroma, const uint8_t *d_luma_lowres, int cwblk,
		const uint8_t *d_luma, int ywblk, int yhblk, uint8_t *d_pixels, size_t pitch,
		int w1, int h1, int first_rows, int ws, int hs, void *stream);
int qs_hip_fdct_plane(const uint8_t *d_pixels, size_t pitch, int16_t *d_coef, int wblk, int hblk, void *stream);

/* final +-1023 clamp alone (reference :2668-2689) */
int qs_hip_clamp_plane(int16_t *d_coef, int wblk, int hblk, void *stream);
/* dequantise only (reference :2551-2566) */
int qs_hip_dequant_plane(const void *d_consts, int16_t *d_coef, int wblk, int hblk, void *stream);

#ifdef __cplusplus
}
#endif
#endif
