"""What the host drivers of the device stages (csrc/qs_decode_job.cpp, qs_compress_job.cpp, qs_encode_job.cpp,
qs_read_job.cpp, qs_device_job.cpp) and the job layer's entry points refuse, call by call: the exact error code and the
exact text of qs_hip_last_error().  Every case fails validation before the call asks for a device, so the table reads
the same with and without a GPU and nothing is ever launched on the fake device addresses below."""
import ctypes as C

EINVAL, ENOTSUP = -2, -4
Q = [16] * 64
WS, STOP, OUT, LEN, STATUS = 0x4000000, 0x5000000, 0x6000000, 0x7000000, 0x7100000
BASE = (0x100000, 0x200000, 0x300000, 0x400000)

# the workspace of one YCC job below, per stage (the info calls; the numbers are part of the messages)
DEC_WS, CMP_WS, ENC_WS, RD_WS, JOB_WS, BATCH_WS = 480, 1232, 58880, 8704, 235520, 237824

DEC, CMP, ENC, RD = ("qs_hip_decode_device_batch", "qs_hip_compress_device_batch", "qs_hip_encode_device_batch",
                     "qs_hip_read_device_batch")
FANCY = ("fancy != 0 is refused: pass 0 for the box filter of do_fancy_downsampling = FALSE; libjpeg 9's default (2x "
         "chroma through 16-point scaled DCTs) is QS_HIP_DOWNSAMPLE_DCT of the _opts calls")
RD_GEOM = ("image needs sampling factors 1..4 and, per component, at least libjpeg's width_in_blocks x height_in_blocks "
           "blocks")
ALIGN = "has no data or is not 16-byte aligned"


def _cases(pkg, hip):
    """[(id, call, code, message)]"""

    def job(shapes, hs=None, vs=None, cs=None, size=None, quants=None, ptrs=BASE, up=None, ncomp=None):
        n = len(shapes)
        j = hip.device_job(list(ptrs[:n]), shapes, quants if quants is not None else [Q] * n, hsamp=hs, vsamp=vs,
                           colorspace=cs, image_size=size)
        if up is not None:                                  # replacement chroma of 4 x 4 blocks at these addresses
            j.up_wblk = j.up_hblk = 4
            j.coef_up[0], j.coef_up[1] = up
        if ncomp is not None:
            j.ncomp = ncomp
        return j

    def ycc(shapes=((4, 4), (2, 2), (2, 2)), hs=(2, 1, 1), vs=(2, 1, 1), cs=3, size=(32, 32), **kw):
        return job(list(shapes), list(hs), list(vs), cs, size, **kw)

    def gray(shapes=((2, 2),), size=(16, 16), cs=1, **kw):
        return job(list(shapes), [1], [1], cs, size, **kw)

    def cmyk11():                                           # 4x2 + 1x1 + 1x1 + 1x1: 11 blocks in an MCU
        return job([(2, 4), (1, 1), (1, 1), (1, 1)], [4, 1, 1, 1], [2, 1, 1, 1], 4, (32, 16))

    bad = lambda: ycc(ncomp=5)
    odd = (BASE[0], BASE[1] + 2, BASE[2])
    zero_q = [[16] * 5 + [0] + [16] * 58, Q, Q]
    ro = lambda **kw: hip.read_opts(dc_tbl=[0, 1, 1, 0], ac_tbl=[0, 1, 1, 0], **kw)
    flags = pkg.flags_for_quality(3)
    out = []

    def add(name, call, code, msg):
        out.append((name, call, code, msg))

    # ---- decode -------------------------------------------------------------------------------------------------------
    di = lambda jobs: (lambda: hip.decode_batch_info(jobs))
    dr = lambda jobs, pitch=96, ws=WS, n=DEC_WS: (lambda: hip.decode_batch(jobs, None, [OUT] * len(jobs),
                                                                           [pitch] * len(jobs), ws, n))
    I, P, R = DEC + "_info", DEC + "_prepare", DEC
    add("decode: null job", di([None]), EINVAL, f"{I}: job 0: bad job")
    add("decode: ncomp 5", di([bad()]), EINVAL, f"{I}: job 0: bad job")
    add("decode: job 1 of 2", di([ycc(), bad()]), EINVAL, f"{I}: job 1: bad job")
    add("decode: njobs 0", di([]), EINVAL, f"{I}: 0 jobs (at least one)")
    add("decode: 0 x N", di([ycc(size=(0, 16))]), EINVAL, f"{I}: job 0: the decode needs image_width x image_height (got 0 x 16)")
    add("decode: 65501", di([ycc(size=(65501, 16))]), EINVAL, f"{I}: job 0: image of 65501 x 16 exceeds JPEG's 65500")
    add("decode: factor 5", di([ycc(hs=(5, 1, 1))]), EINVAL, f"{I}: job 0: component 0 has sampling factors 5x2")
    add("decode: colour space", di([ycc(cs=1)]), ENOTSUP,
        f"{I}: job 0: 3 components in colour space 1: the device decode covers grayscale, YCbCr and RGB (3 components)")
    add("decode: 2x1 chroma", di([ycc(hs=(2, 2, 1))]), ENOTSUP,
        f"{I}: job 0: chroma component 1 is sampled 2x1: the device decode needs 1x1 chroma")
    add("decode: 3x1 luma", di([ycc(hs=(3, 1, 1), vs=(1, 1, 1))]), ENOTSUP,
        f"{I}: job 0: luma sampling 3x1: the device decode covers 1x1, 2x1, 1x2, 2x2 and 4x1")
    add("decode: no quant table", di([ycc(quants=[Q, None, Q])]), EINVAL, f"{I}: job 0: component 1 has no quant table")
    add("decode: narrow array", di([ycc(shapes=((4, 3), (2, 2), (2, 2)))]), EINVAL,
        f"{I}: job 0: component 0 has 3 x 4 blocks, a 32 x 32 image needs 4 x 4")
    add("decode: short array", di([ycc(shapes=((4, 4), (2, 2), (1, 2)))]), EINVAL,
        f"{I}: job 0: component 2 has 2 x 1 blocks, a 32 x 32 image needs 2 x 2")
    add("decode: misaligned array", dr([ycc(ptrs=odd)]), EINVAL, f"{R}: job 0: component 1 {ALIGN}")
    add("decode: misaligned replacement chroma", dr([ycc(up=(0x900002, 0xa00000))]), EINVAL,
        f"{R}: job 0: component 1 (replacement chroma) {ALIGN}")
    add("decode: pitch", dr([ycc()], pitch=95), EINVAL, f"{R}: job 0: output pitch 95 for rows of 32 x 3 samples")
    add("decode: misaligned workspace", lambda: hip.decode_batch_prepare([ycc()], WS + 128, DEC_WS), EINVAL,
        f"{P}: workspace of {DEC_WS} bytes (256-byte aligned), the batch needs {DEC_WS}")
    add("decode: short workspace", dr([ycc()], n=DEC_WS - 1), EINVAL,
        f"{R}: workspace of {DEC_WS - 1} bytes (256-byte aligned), the batch needs {DEC_WS}")

    # ---- compress -----------------------------------------------------------------------------------------------------
    ci = lambda jobs, **kw: (lambda: hip.compress_batch_info(jobs, **kw))
    cr = lambda jobs, pitch=96, ws=WS, n=CMP_WS: (lambda: hip.compress_batch(jobs, [OUT] * len(jobs), [pitch] * len(jobs),
                                                                            ws, n))
    I, P, R = CMP + "_info", CMP + "_prepare", CMP
    add("compress: null job", ci([None]), EINVAL, f"{I}: job 0: bad job")
    add("compress: ncomp 5", ci([bad()]), EINVAL, f"{I}: job 0: bad job")
    add("compress: job 1 of 2", ci([ycc(), bad()]), EINVAL, f"{I}: job 1: bad job")
    add("compress: njobs 0", ci([]), EINVAL, f"{I}: 0 jobs (at least one)")
    add("compress: 0 x N", ci([ycc(size=(0, 16))]), EINVAL,
        f"{I}: job 0: the compress needs image_width x image_height (got 0 x 16)")
    add("compress: 65501", ci([ycc(size=(16, 65501))]), EINVAL, f"{I}: job 0: image of 16 x 65501 exceeds JPEG's 65500")
    add("compress: factor 5", ci([ycc(vs=(2, 5, 1))]), EINVAL, f"{I}: job 0: component 1 has sampling factors 1x5")
    add("compress: colour space", ci([gray(cs=3)]), ENOTSUP,
        f"{I}: job 0: 1 components in colour space 3: the device compress covers grayscale, YCbCr and RGB (3 components)")
    add("compress: 2x1 chroma", ci([ycc(hs=(2, 1, 2))]), ENOTSUP,
        f"{I}: job 0: chroma component 2 is sampled 2x1: the device compress needs 1x1 chroma")
    add("compress: 3x1 luma", ci([ycc(hs=(3, 1, 1), vs=(1, 1, 1))]), ENOTSUP,
        f"{I}: job 0: luma sampling 3x1: the device compress covers 1x1, 2x1, 1x2, 2x2 and 4x1")
    add("compress: no quant table", ci([ycc(quants=[None, Q, Q])]), EINVAL, f"{I}: job 0: component 0 has no quant table")
    add("compress: quantiser 0", ci([ycc(quants=zero_q)]), EINVAL, f"{I}: job 0: component 0 has a quantiser of 0")
    add("compress: narrow array", ci([ycc(shapes=((4, 3), (2, 2), (2, 2)))]), EINVAL,
        f"{I}: job 0: component 0 has 3 x 4 blocks, a 32 x 32 image needs 4 x 4")
    add("compress: short array", ci([ycc(shapes=((4, 4), (2, 2), (1, 2)))]), EINVAL,
        f"{I}: job 0: component 2 has 2 x 1 blocks, a 32 x 32 image needs 2 x 2")
    add("compress: 2^31 blocks", ci([gray(shapes=((65536, 65536),))]), EINVAL,
        f"{I}: job 0: component 0 has more than 2^31 blocks")
    add("compress: fancy", ci([ycc()], fancy=True), ENOTSUP, f"{I}: {FANCY}")
    add("compress: a bad job reports before fancy", ci([bad()], fancy=True), EINVAL, f"{I}: job 0: bad job")
    add("compress: fancy in prepare", lambda: hip.compress_batch_prepare([ycc()], WS, CMP_WS, fancy=True), ENOTSUP,
        f"{P}: {FANCY}")
    add("compress: downsampling 7", ci([ycc()], opts=[7]), EINVAL,
        f"{I}_opts: job 0: downsampling 7 (QS_HIP_DOWNSAMPLE_BOX or QS_HIP_DOWNSAMPLE_DCT)")
    add("compress: misaligned array", cr([ycc(ptrs=odd)]), EINVAL, f"{R}: job 0: component 1 {ALIGN}")
    add("compress: pitch", cr([ycc()], pitch=95), EINVAL, f"{R}: job 0: pixel pitch 95 for rows of 32 x 3 samples")
    add("compress: misaligned workspace", lambda: hip.compress_batch_prepare([ycc()], WS + 128, CMP_WS), EINVAL,
        f"{P}: workspace of {CMP_WS} bytes (256-byte aligned), the batch needs {CMP_WS}")
    add("compress: short workspace", cr([ycc()], n=CMP_WS - 1), EINVAL,
        f"{R}: workspace of {CMP_WS - 1} bytes (256-byte aligned), the batch needs {CMP_WS}")
    add("compress: short workspace in prepare_opts",
        lambda: hip.compress_batch_prepare([ycc()], WS, CMP_WS - 1, opts=["dct"]), EINVAL,
        f"{P}_opts: workspace of {CMP_WS - 1} bytes (256-byte aligned), the batch needs {CMP_WS}")

    # ---- entropy coder ------------------------------------------------------------------------------------------------
    ei = lambda jobs, **kw: (lambda: hip.encode_batch_info(jobs, **kw))
    er = lambda jobs, ws=WS, n=ENC_WS: (lambda: hip.encode_batch(jobs, None, [OUT] * len(jobs), [4096] * len(jobs), LEN,
                                                                 STATUS, ws, n))
    I, P, R = ENC + "_info", ENC + "_prepare", ENC
    add("encode: null job", ei([None]), EINVAL, f"{I}: job 0: bad job")
    add("encode: ncomp 5", ei([bad()]), EINVAL, f"{I}: job 0: bad job")
    add("encode: job 1 of 2", ei([ycc(), bad()]), EINVAL, f"{I}: job 1: bad job")
    add("encode: njobs 0", ei([]), EINVAL, f"{I}: 0 jobs (at least one)")
    add("encode: 0 x N", ei([ycc(size=(0, 16))]), EINVAL,
        f"{I}: job 0: the encoder needs image_width x image_height within 65500 (got 0 x 16)")
    add("encode: 65501", ei([ycc(size=(65501, 16))]), EINVAL,
        f"{I}: job 0: the encoder needs image_width x image_height within 65500 (got 65501 x 16)")
    add("encode: colour space", ei([ycc(cs=1)]), ENOTSUP,
        f"{I}: job 0: 3 components in colour space 1: the encoder covers grayscale (1), RGB and YCbCr (3), CMYK and YCCK (4)")
    add("encode: factor 5", ei([ycc(hs=(5, 1, 1))]), EINVAL, f"{I}: job 0: component 0 has sampling factors 5x2")
    add("encode: no blocks", ei([ycc(shapes=((4, 4), (0, 2), (2, 2)))]), EINVAL, f"{I}: job 0: component 1 has no blocks")
    add("encode: stride 0 and factor 5 in one component", ei([ycc(shapes=((4, 0), (2, 2), (2, 2)), hs=(5, 1, 1))]), EINVAL,
        f"{I}: job 0: component 0 has sampling factors 5x2")
    add("encode: narrow array", ei([ycc(shapes=((4, 3), (2, 2), (2, 2)))]), EINVAL,
        f"{I}: job 0: component 0 has 3 x 4 blocks, a 32 x 32 image sampled 2x2 needs 4 x 4")
    add("encode: short array", ei([ycc(shapes=((4, 4), (2, 2), (1, 2)))]), EINVAL,
        f"{I}: job 0: component 2 has 2 x 1 blocks, a 32 x 32 image sampled 1x1 needs 2 x 2")
    add("encode: 11 blocks in an MCU", ei([cmyk11()]), ENOTSUP, f"{I}: job 0: 11 blocks in an MCU; libjpeg takes at most 10")
    add("encode: restart_interval 70000", ei([ycc()], opts=[(70000, 0)]), EINVAL,
        f"{I}_opts: job 0: restart_interval 70000 (0 .. 65535), restart_in_rows 0 (0 or more)")
    add("encode: restart_in_rows -1", ei([ycc(), ycc()], opts=[None, (0, -1)]), EINVAL,
        f"{I}_opts: job 1: restart_interval 0 (0 .. 65535), restart_in_rows -1 (0 or more)")
    add("encode: misaligned array", er([ycc(ptrs=odd)]), EINVAL, f"{R}: job 0: component 1 {ALIGN}")
    add("encode: misaligned replacement chroma", er([ycc(up=(0x900002, 0xa00000))]), EINVAL,
        f"{R}: job 0: component 1 (replacement chroma) {ALIGN}")
    add("encode: misaligned workspace", lambda: hip.encode_batch_prepare([ycc()], None, WS + 128, ENC_WS), EINVAL,
        f"{P}: workspace of {ENC_WS} bytes (256-byte aligned), the batch needs {ENC_WS}")
    add("encode: short workspace in prepare_opts",
        lambda: hip.encode_batch_prepare([ycc()], None, WS, ENC_WS - 1, opts=[(1, 0)]), EINVAL,
        f"{P}_opts: workspace of {ENC_WS - 1} bytes (256-byte aligned), the batch needs {ENC_WS}")
    add("encode: short workspace", er([ycc()], n=ENC_WS - 1), EINVAL,
        f"{R}: workspace of {ENC_WS - 1} bytes (256-byte aligned), the batch needs {ENC_WS}")
    add("encode: short workspace of the histogram run",
        lambda: hip.encode_batch_histogram([ycc()], None, OUT, STATUS, WS, ENC_WS - 1), EINVAL,
        f"{R}_histogram: workspace of {ENC_WS - 1} bytes (256-byte aligned), the batch needs {ENC_WS}")

    # ---- scan reader --------------------------------------------------------------------------------------------------
    ri = lambda jobs, opts=None: (lambda: hip.read_batch_info(jobs, opts if opts is not None else [ro()] * len(jobs)))
    rr = lambda jobs, ws=WS, n=RD_WS: (lambda: hip.read_batch(jobs, [OUT] * len(jobs), [100] * len(jobs), STATUS, ws, n))
    I, P, R = RD + "_info", RD + "_prepare", RD

    def null_opts():
        per, total = (pkg.hipqs.ReadInfo * 1)(), C.c_size_t(0)
        hip._check(hip.lib.qs_hip_read_device_batch_info(hip._job_ptrs([ycc()]), 1, None, per, C.byref(total)))

    add("read: null job", ri([None]), EINVAL, f"{I}: job 0: bad job")
    add("read: ncomp 5", ri([bad()]), EINVAL, f"{I}: job 0: bad job")
    add("read: job 1 of 2", ri([ycc(), bad()]), EINVAL, f"{I}: job 1: bad job")
    add("read: njobs 0", ri([]), EINVAL, f"{I}: 0 jobs (at least one)")
    add("read: null opts", null_opts, EINVAL, f"{I}: null opts")
    add("read: no options for a job", ri([ycc()], [None]), EINVAL,
        f"{I}: job 0: no options (the tables of each component and the restart interval)")
    add("read: 0 x N", ri([ycc(size=(0, 16))]), EINVAL, f"{I}: job 0: a 0 x 16 {RD_GEOM}")
    add("read: 65501", ri([ycc(size=(65501, 16))]), EINVAL, f"{I}: job 0: a 65501 x 16 {RD_GEOM}")
    add("read: factor 5", ri([ycc(hs=(5, 1, 1))]), EINVAL, f"{I}: job 0: a 32 x 32 {RD_GEOM}")
    add("read: stride 0 and factor 5 in one component", ri([ycc(shapes=((4, 0), (2, 2), (2, 2)), hs=(5, 1, 1))]), EINVAL,
        f"{I}: job 0: a 32 x 32 {RD_GEOM}")
    add("read: narrow array", ri([ycc(shapes=((4, 3), (2, 2), (2, 2)))]), EINVAL, f"{I}: job 0: a 32 x 32 {RD_GEOM}")
    add("read: short array", ri([ycc(shapes=((4, 4), (2, 2), (1, 2)))]), EINVAL, f"{I}: job 0: a 32 x 32 {RD_GEOM}")
    add("read: 11 blocks in an MCU", ri([cmyk11()]), ENOTSUP,
        f"{I}: job 0: more than 10 blocks in an MCU; libjpeg takes at most 10")
    add("read: restart_interval 70000", ri([ycc()], [ro(restart_interval=70000)]), EINVAL,
        f"{I}: job 0: restart_interval 70000 (0 .. 65535)")
    add("read: restart_interval -1", ri([ycc()], [ro(restart_interval=-1)]), EINVAL,
        f"{I}: job 0: restart_interval -1 (0 .. 65535)")
    add("read: interval cap", ri([gray(shapes=((200, 200),), size=(1600, 1600))]), ENOTSUP,
        f"{I}: job 0: 40000 blocks in a restart interval (restart_interval 0, 40000 MCUs); one lane reads an interval, of "
        "at most 32768 blocks")
    add("read: table 4", ri([ycc()], [hip.read_opts(dc_tbl=[0, 4, 1], ac_tbl=[0, 1, 1])]), EINVAL,
        f"{I}: job 0: component 1 names tables 4 / 1 (0 .. 3)")
    add("read: table 2 not there", ri([ycc()], [hip.read_opts(dc_tbl=[0, 1, 1], ac_tbl=[0, 1, 2])]), EINVAL,
        f"{I}: job 0: component 2 uses a table the options do not hold (only 0 and 1 have a standard table)")
    add("read: 2^31 blocks", ri([gray(shapes=((65536, 65536),))]), EINVAL, f"{I}: job 0: component 0 has more than 2^31 blocks")
    add("read: misaligned workspace", lambda: hip.read_batch_prepare([ycc()], [ro()], WS + 128, RD_WS), EINVAL,
        f"{P}: workspace of {RD_WS} bytes (256-byte aligned), the batch needs {RD_WS}")
    add("read: short workspace", lambda: hip.read_batch_prepare([ycc()], [ro()], WS, RD_WS - 1), EINVAL,
        f"{P}: workspace of {RD_WS - 1} bytes (256-byte aligned), the batch needs {RD_WS}")
    add("read run: njobs 0", rr([]), EINVAL, f"{R}: 0 jobs (at least one)")
    add("read run: null d_status", lambda: hip.read_batch([ycc()], [OUT], [100], None, WS, RD_WS), EINVAL, f"{R}: null argument")
    add("read run: misaligned workspace", rr([ycc()], ws=WS + 128), EINVAL,
        f"{R}: workspace of {RD_WS} bytes (256-byte aligned): not what prepare was given")
    add("read run: workspace short of the descriptors", rr([ycc()], n=255), EINVAL,
        f"{R}: workspace of 255 bytes (256-byte aligned): not what prepare was given")
    # (the run call looks at its jobs after it has asked for a device: those refusals are not in this table)

    # ---- the device-resident job: one job (no "job 0" in the message) or a batch ---------------------------------------
    ONE, PREP1, RUN1 = "qs_hip_device_job_info", "qs_hip_device_job_prepare", "qs_hip_do_quantsmooth_device"
    I, P, R = "qs_hip_device_batch_info", "qs_hip_device_batch_prepare", "qs_hip_do_quantsmooth_device_batch"
    one = lambda j: (lambda: hip.device_job_info(j, flags, 3))
    bi = lambda jobs: (lambda: hip.device_batch_info(jobs, flags, 3))
    add("job: ncomp 5", one(bad()), EINVAL, f"{ONE}: bad job")
    add("job: no blocks", one(ycc(shapes=((4, 4), (0, 2), (2, 2)))), EINVAL, f"{ONE}: component 1 has no blocks")
    add("job: factor 5", one(ycc(hs=(5, 1, 1))), EINVAL, f"{ONE}: component 0 has sampling factors 5x2")
    add("job: too large", one(gray(shapes=((16384, 16384),))), EINVAL, f"{ONE}: component 0 is too large")
    add("job: misaligned array", lambda: hip.do_quantsmooth_device(ycc(ptrs=odd), flags, 3, WS, JOB_WS, STOP), EINVAL,
        f"{RUN1}: component 1 {ALIGN}")
    add("job: misaligned workspace", lambda: hip.device_job_prepare(ycc(), flags, 3, WS + 128, JOB_WS), EINVAL,
        f"{PREP1}: workspace of {JOB_WS} bytes (256-byte aligned), the job needs {JOB_WS}")
    add("job: short workspace", lambda: hip.do_quantsmooth_device(ycc(), flags, 3, WS, JOB_WS - 1, STOP), EINVAL,
        f"{RUN1}: workspace of {JOB_WS - 1} bytes (256-byte aligned), the job needs {JOB_WS}")
    add("batch: null job", bi([None]), EINVAL, f"{I}: job 0: bad job")
    add("batch: job 1 of 2", bi([ycc(), bad()]), EINVAL, f"{I}: job 1: bad job")
    add("batch: njobs 0", bi([]), EINVAL, f"{I}: 0 jobs (at least one)")
    add("batch: factor 5", bi([ycc(hs=(5, 1, 1))]), EINVAL, f"{I}: job 0: component 0 has sampling factors 5x2")
    add("batch: misaligned array", lambda: hip.do_quantsmooth_device_batch([ycc(ptrs=odd)], flags, 3, WS, BATCH_WS, STOP),
        EINVAL, f"{R}: job 0: component 1 {ALIGN}")
    add("batch: misaligned workspace", lambda: hip.device_batch_prepare([ycc()], flags, 3, WS + 128, BATCH_WS), EINVAL,
        f"{P}: workspace of {BATCH_WS} bytes (256-byte aligned), the batch needs {BATCH_WS}")
    add("batch: short workspace", lambda: hip.do_quantsmooth_device_batch([ycc()], flags, 3, WS, BATCH_WS - 1, STOP), EINVAL,
        f"{R}: workspace of {BATCH_WS - 1} bytes (256-byte aligned), the batch needs {BATCH_WS}")

    # ---- the job layer's entry points (qs_job.cpp, qs_batch.cpp) -------------------------------------------------------
    lib, ck = hip.lib, hip._check
    no_fn = pkg.hipqs.PROGRESS_FN()
    add("do_quantsmooth: null job", lambda: ck(lib.qs_hip_do_quantsmooth(None, 0, 3, 0, no_fn, None)), EINVAL,
        "qs_hip_do_quantsmooth: bad job")
    add("rows: null job", lambda: ck(lib.qs_hip_do_quantsmooth_rows(None, None, 0, 3, 0, no_fn, None)), EINVAL,
        "qs_hip_do_quantsmooth_rows: bad job")
    add("sharded: no devices", lambda: ck(lib.qs_hip_do_quantsmooth_sharded(C.byref(ycc()), 0, 3, None, 0)), EINVAL,
        "qs_hip_do_quantsmooth_sharded: empty device list")
    add("host batch: null results", lambda: ck(lib.qs_hip_do_quantsmooth_batch(hip._job_ptrs([ycc()]), 1, 0, 3, None)), EINVAL,
        "qs_hip_do_quantsmooth_batch: null argument")
    return out


def test_info_calls_give_the_workspace_sizes_the_messages_name(pkg, hip):
    j = lambda: hip.device_job([0x100000, 0x200000, 0x300000], [(4, 4), (2, 2), (2, 2)], [Q] * 3, hsamp=[2, 1, 1],
                               vsamp=[2, 1, 1], colorspace=3, image_size=(32, 32))
    flags = pkg.flags_for_quality(3)
    o = hip.read_opts(dc_tbl=[0, 1, 1], ac_tbl=[0, 1, 1])
    assert hip.decode_batch_info([j()])[1] == DEC_WS
    assert hip.compress_batch_info([j()])[1] == CMP_WS
    assert hip.encode_batch_info([j()])[1] == ENC_WS
    assert hip.encode_batch_info([j()], opts=[(1, 0)])[1] == ENC_WS
    assert hip.read_batch_info([j()], [o])[1] == RD_WS
    assert hip.device_job_info(j(), flags, 3)["workspace_bytes"] == JOB_WS
    assert hip.device_batch_info([j()], flags, 3)[1] == BATCH_WS


def test_every_refusal_has_its_code_and_its_message(pkg, hip):
    """one table: the call, QsHipError.code, the whole message"""
    cases = _cases(pkg, hip)
    assert len({c[0] for c in cases}) == len(cases)
    wrong = []
    for name, call, code, msg in cases:
        try:
            call()
            got = (0, "(the call succeeded)")
        except pkg.hipqs.QsHipError as e:
            got = (e.code, str(e))
        want = (code, f"libjpegqs_hip error {code}: {msg}")
        if got != want:
            wrong.append(f"{name}:\n    want {want}\n    got  {got}")
    assert not wrong, f"{len(wrong)} of {len(cases)} cases:\n" + "\n".join(wrong)
