"""The device compress with libjpeg 9's default DCT-scaled chroma downsampling, without a GPU: the host build of its
arithmetic (tests/compress_fancy_host.cpp over csrc/qs_compress.h -- the functions the lanes of a block run) against
libjpeg 9 with do_fancy_downsampling TRUE and against its exported jpeg_fdct_16x16 / _16x8 / _8x16, the bounds that
make wrapping 32-bit arithmetic exact, the same program under the address and undefined-behaviour sanitizers, and the
_opts info call -- no device touched."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import jpegqs_pkg
from compress_fancy_oracle import (FANCY_SIZES, KINDS, LAYOUTS, SHAPES, SUBSAMPLED, CompressFancy9, assert_same_arrays,
                                   extreme_blocks, pixels, tables)

pkg = jpegqs_pkg.load()


@pytest.fixture(scope="module")
def c9(tmp_path_factory):
    return CompressFancy9(tmp_path_factory.mktemp("c9f"))


@pytest.fixture(scope="module")
def hip():
    return pkg.HipQS()


def _blocks(shape):
    w, h = SHAPES[shape]
    rng = np.random.default_rng([w, h])
    b = rng.integers(0, 256, (2048, w * h)).astype(np.uint8)
    b[0] = 0
    b[1] = 255
    b[2:130] = rng.choice(np.array([0, 255], np.uint8), (128, w * h))
    return np.concatenate([b, extreme_blocks(w, h)])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_scaled_block_functions_equal_libjpegs(c9, shape):
    """random, all-0, all-255, two-valued and cosine-sign extreme blocks through jpeg_fdct_<shape> and the host build"""
    b = _blocks(shape)
    want = c9.fdct16("libjpeg", shape, b)
    got = c9.fdct16("host", shape, b)
    bad = np.argwhere(got != want)
    assert not len(bad), f"{shape}: {len(bad)} outputs differ, first at block {bad[0][0]} k {bad[0][1]}"
    assert want[0, 0] == -8192 and want[1, 0] == 8128 and not want[0, 1:].any()       # (the scale by 8, the centre)
    assert np.abs(want).max() < 1 << 17                                               # the quantiser's proven domain


def test_extreme_blocks_reach_the_pass_1_norm(c9):
    """a row of 0 / 255 by the sign of row k of the 16-point matrix gives that row's L1 norm times 127.5: the extreme
    blocks are the inputs the bound is about"""
    n = c9.norms()
    ext = extreme_blocks(16, 8)
    want = c9.fdct16("libjpeg", "16x8", ext)
    # blocks 4k (+) and 4k + 2 (-) hold row pattern k in every row: pass 1 gives (+-L1 * 127.5 + 2^10) >> 11 in each
    # (the row sums to zero, so 255 / 0 count as 127 / -128), and pass 2's first output is the mean of eight equal values
    for k in range(1, 8):
        a, b = int(want[4 * k][k]), int(want[4 * k + 2][k])
        exact = n[f"l1_16_{k}"] * 127.5 / 2048
        assert abs(a - exact) <= 1 and abs(b + exact) <= 1, (k, a, b, exact)


def test_bounds_make_32_bit_arithmetic_exact(c9):
    """the integer matrices of the 8- and 16-point passes (unit vectors through the host build), their rows' L1 norms,
    and what follows for 8-bit samples: every pass's sums stay below 2^31, so no pass needs 64 bits"""
    n = c9.norms()
    l16 = [n[f"l1_16_{i}"] for i in range(8)]
    l8 = [n[f"l1_8_{i}"] for i in range(8)]
    assert l16[0] == 16 and l8[0] == 8                                    # the plain sums
    assert all(n[f"rowsum_16_{i}"] == 0 and n[f"rowsum_8_{i}"] == 0 for i in range(1, 8))     # CENTERJSAMPLE drops out
    assert n["rowsum_16_0"] == 16 and n["rowsum_8_0"] == 8
    # the float model: row i of the N-point matrix is 2^13 sqrt(2) cos((2x+1) i pi / 2N); FIX() rounding moves a norm
    # by a few units per composed constant
    for N, l in ((16, l16), (8, l8)):
        x = np.arange(N)
        for i in range(1, 8):
            if N == 8 and i == 4:                           # the 8-point pass keeps output 4 a plain butterfly (<< 2)
                assert l[i] == 8
                continue
            ideal = 8192 * np.sqrt(2) * np.abs(np.cos((2 * x + 1) * i * np.pi / (2 * N))).sum()
            assert abs(l[i] - ideal) < 64, (N, i, l[i], ideal)
    assert max(l16[1:]) == n["l1max_16"] == 121088 and max(l8[1:]) == n["l1max_8"] == 60548
    # pass 1: |sum| <= L1 * 128 + 2^10, stored >> 11; the DC output is (sum - N * 128) << 2
    assert n["pass1_16"] == 121088 * 128 + 1024 < 1 << 24 and n["pass1_8"] == 60548 * 128 + 1024 < 1 << 23
    assert n["dmax_16"] == max(n["pass1_16"] >> 11, 16 * 128 * 4) == 8192
    assert n["dmax_8"] == max(n["pass1_8"] >> 11, 8 * 128 * 4) == 4096
    # pass 2: L1 * dmax + the rounding term
    assert n["pass2_16x16"] == 121088 * 8192 + (1 << 16) == 992018432
    assert n["pass2_8x16"] == 121088 * 4096 + (1 << 15)
    assert n["pass2_16x8"] == 60548 * 8192 + (1 << 15)
    assert max(n["pass2_16x16"], n["pass2_8x16"], n["pass2_16x8"]) < 1 << 30          # 2^29.89: a factor 2.16 of room
    assert n["needs64"] == 0
    assert 16 * 11590 * 11590 > 1 << 31                     # (the crude bound that raised the question does pass 2^31)
    assert max(n["wmax_16x16"], n["wmax_8x16"], n["wmax_16x8"]) < 1 << 13 and 8192 < 1 << 17      # AC and DC outputs


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,hs,vs,cs", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_host_build_equals_libjpeg_default(c9, name, hs, vs, cs, kind):
    """every layout x size x table kind: the arrays of the host build's dct mode are those of libjpeg 9 with
    do_fancy_downsampling TRUE, bit for bit; luma and every 1x1 layout also equal the box mode's"""
    rng = np.random.default_rng([len(name), hs[0], vs[0], cs, len(kind), 7])
    for size in FANCY_SIZES:
        px = pixels(rng, size, len(hs))
        q = tables(kind, len(hs), pkg.synth, rng)
        want = c9.libjpeg(px, q, hs, vs, cs)
        got = c9.host(px, q, hs, vs, cs)
        assert want["image_size"] == size and want["hsamp"] == got["hsamp"] and want["vsamp"] == got["vsamp"]
        assert_same_arrays(got["coefs"], want["coefs"], f"{name} {size} {kind}")
        box = c9.host(px, q, hs, vs, cs, mode="box")
        assert [c.shape for c in box["coefs"]] == [c.shape for c in got["coefs"]]
        same = len(hs) if hs[0] * vs[0] == 1 or size == (1, 1) else 1
        assert_same_arrays(got["coefs"][:same], box["coefs"][:same], f"{name} {size} {kind}: dct against box")


def test_host_box_mode_is_libjpegs_box_mode(c9):
    """the box mode of the two-mode host program is libjpeg with do_fancy_downsampling FALSE"""
    rng = np.random.default_rng(5)
    for name, hs, vs, cs in SUBSAMPLED:
        for size in [(33, 18), (65, 66)]:
            px = pixels(rng, size, 3)
            q = tables("q50", 3, pkg.synth)
            assert_same_arrays(c9.host(px, q, hs, vs, cs, mode="box")["coefs"],
                               c9.libjpeg_box(px, q, hs, vs, cs)["coefs"], f"{name} {size}")


def test_the_modes_differ_where_chroma_is_subsampled(c9):
    """8 x 8 at 2x2 with tables of 1: most chroma coefficients of libjpeg's two modes differ"""
    rng = np.random.default_rng(6)
    px = pixels(rng, (8, 8), 3)
    q = tables("ones", 3, pkg.synth)
    a = c9.libjpeg(px, q, [2, 1, 1], [2, 1, 1], 3)["coefs"]
    b = c9.libjpeg_box(px, q, [2, 1, 1], [2, 1, 1], 3)["coefs"]
    assert np.array_equal(a[0], b[0])
    assert (a[1] != b[1]).sum() > 32 and (a[2] != b[2]).sum() > 32


def test_sanitizer_build_runs_clean(c9):
    """the same stand-alone program under -fsanitize=address,undefined: the three block functions on their extreme
    blocks, and the grid's layouts at the sizes where the edge rules are at work"""
    exe = c9.build_fancy_host("compress_fancy_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                          "-fno-omit-frame-pointer"])
    for shape in SHAPES:
        b = _blocks(shape)[-400:]
        assert np.array_equal(c9.fdct16("host", shape, b, exe=exe), c9.fdct16("libjpeg", shape, b))
    rng = np.random.default_rng(21)
    for name, hs, vs, cs in LAYOUTS:
        for size in [(1, 1), (33, 18), (65, 66), (63, 33)]:
            px = pixels(rng, size, len(hs))
            q = tables("edge", len(hs), pkg.synth, rng)
            got = c9.host(px, q, hs, vs, cs, exe=exe)
            assert_same_arrays(got["coefs"], c9.libjpeg(px, q, hs, vs, cs)["coefs"], f"sanitizer build, {name} {size}")


def _job(hip, size, hs, vs, cs):
    n = len(hs)
    mh, mv = (1, 1) if n == 1 else (max(hs), max(vs))
    shapes = [(-(-size[1] * (1 if n == 1 else vs[ci]) // (8 * mv)), -(-size[0] * (1 if n == 1 else hs[ci]) // (8 * mh)))
              for ci in range(n)]
    return hip.device_job([0x1000 * (ci + 1) for ci in range(n)], shapes, [np.full(64, 3, np.uint16)] * n, hsamp=hs,
                          vsamp=vs, colorspace=cs, image_size=size)


def _code(hip, jobs, opts):
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.compress_batch_info(jobs, opts=opts)
    return e.value.code


def test_info_opts_geometry_is_the_old_calls(c9, hip):
    """NULL opts, NULL entries, box and dct: the geometry and the workspace size of the call without opts -- and
    libjpeg's block counts with its default downsampling"""
    rng = np.random.default_rng(41)
    for name, hs, vs, cs in LAYOUTS:
        for size in [(1, 1), (33, 18), (70, 50)]:
            jobs = [_job(hip, size, hs, vs, cs)]
            old = hip.compress_batch_info(jobs)
            for opts in ([None], ["box"], ["dct"], [pkg.hipqs.CompressOpts()]):
                assert hip.compress_batch_info(jobs, opts=opts) == old, (name, size, opts)
            want = c9.libjpeg(pixels(rng, size, len(hs)), tables("ones", len(hs), pkg.synth), hs, vs, cs)
            assert list(zip(old[0][0]["hblk"], old[0][0]["wblk"])) == [c.shape[:2] for c in want["coefs"]]
    # the opts array itself NULL, through the C call
    jobs = [_job(hip, (33, 18), [2, 1, 1], [2, 1, 1], 3)] * 2
    per, total = (pkg.hipqs.CompressInfo * 2)(), C.c_size_t(0)
    assert hip.lib.qs_hip_compress_device_batch_info_opts(hip._job_ptrs(jobs), 2, None, per, C.byref(total)) == 0
    assert total.value == hip.compress_batch_info(jobs)[1]
    mixed = hip.compress_batch_info(jobs, opts=["dct", None])
    assert mixed == hip.compress_batch_info(jobs)


def test_info_opts_refusals(hip):
    ok = _job(hip, (32, 16), [2, 1, 1], [2, 1, 1], 3)
    for bad in (2, -1, 1 << 20):
        assert _code(hip, [ok], [bad]) == -2                              # unknown downsampling: QS_HIP_EINVAL
        assert "downsampling" in hip.lib.qs_hip_last_error().decode()
    for slot in range(3):
        o = pkg.hipqs.CompressOpts()
        o.downsampling = 1
        o.reserved[slot] = 1
        assert _code(hip, [ok], [o]) == -2                                # non-zero reserved
        assert "reserved" in hip.lib.qs_hip_last_error().decode()
    assert _code(hip, [ok, ok], ["dct", 7]) == -2
    assert "job 1" in hip.lib.qs_hip_last_error().decode()
    for opts in (["dct"], ["box"], [None]):
        assert _code(hip, [_job(hip, (32, 16), [2, 2, 2], [2, 2, 2], 3)], opts) == -4         # chroma factors of 2
        assert _code(hip, [_job(hip, (48, 16), [3, 1, 1], [1, 1, 1], 3)], opts) == -4         # 3x1 luma
        assert _code(hip, [_job(hip, (48, 16), [4, 1, 1], [2, 1, 1], 3)], opts) == -4         # 4x2 luma
        assert _code(hip, [_job(hip, (32, 16), [1, 1, 1, 1], [1, 1, 1, 1], 4)], opts) == -4   # CMYK
    job = _job(hip, (32, 16), [2, 1, 1], [2, 1, 1], 3)
    job.image_width = 40                                                  # more pixels than the arrays hold
    assert _code(hip, [job], ["dct"]) == -2
    with pytest.raises(ValueError):
        hip.compress_batch_info([ok], opts=["dct", "dct"])                # one entry per job
    with pytest.raises(ValueError, match="downsampling"):
        hip.compress_batch_info([ok], opts=["nonsense"])
    # the old argument keeps its meaning, and its text now names the way
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.compress_batch_info([ok], fancy=True)
    assert e.value.code == -4 and "fancy" in hip.lib.qs_hip_last_error().decode()
    assert "QS_HIP_DOWNSAMPLE_DCT" in hip.lib.qs_hip_last_error().decode()


def test_header_declares_the_opts_calls():
    hdr = (Path(__file__).resolve().parent.parent / "include" / "jpegqs_hip.h").read_text()
    assert re.search(r"#define QS_HIP_DOWNSAMPLE_BOX 0\b", hdr) and re.search(r"#define QS_HIP_DOWNSAMPLE_DCT 1\b", hdr)
    assert "qs_hip_compress_device_batch_info_opts(" in hdr and "qs_hip_compress_device_batch_prepare_opts(" in hdr
    lib = pkg.HipQS().lib
    assert lib.qs_hip_compress_device_batch_info_opts and lib.qs_hip_compress_device_batch_prepare_opts
    assert pkg.hipqs.DOWNSAMPLE_BOX == 0 and pkg.hipqs.DOWNSAMPLE_DCT == 1
    assert C.sizeof(pkg.hipqs.CompressOpts) == 16


def test_torch_layer_argument_errors_need_no_gpu():
    """ValueError for an unknown downsampling -- the call's default or an image's own -- and for fancy=True is decided
    before any device is touched"""
    tq = pkg.torch_qs
    with pytest.raises(ValueError, match="downsampling"):
        tq.compress_batch([dict(pixels=None)], downsampling="nonsense")
    with pytest.raises(ValueError, match="downsampling"):
        tq.compress_batch([dict(pixels=None, downsampling="nonsense")], downsampling="dct")
    with pytest.raises(ValueError, match="downsampling"):
        tq.compress(None, quality=50, downsampling=1)
    with pytest.raises(ValueError, match="fancy"):
        tq.compress_batch([dict(pixels=None)], fancy=True, downsampling="dct")
