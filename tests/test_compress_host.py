"""The device compress without a GPU: the host build of its arithmetic (tests/compress_host.cpp over
csrc/qs_compress.h -- the functions a lane runs) against libjpeg 9 (jpeg_write_scanlines with JDCT_ISLOW,
smoothing_factor 0, do_fancy_downsampling FALSE), the same program under the address and undefined-behaviour sanitizers,
libjpeg against itself, and the info call (shapes, workspace, unsupported and invalid input) -- no device touched."""
import numpy as np
import pytest

import jpegqs_pkg
from compress_oracle import (EDGE_VALUES, LAYOUTS, SIZES, Compress9, all_colours, assert_same_arrays, pixels, tables)
from encode_oracle import LibJpeg9Enc, parse_jpeg

pkg = jpegqs_pkg.load()


@pytest.fixture(scope="module")
def c9(tmp_path_factory):
    return Compress9(tmp_path_factory.mktemp("c9"))


@pytest.fixture(scope="module")
def hip():
    return pkg.HipQS()


@pytest.mark.parametrize("kind", ["ones", "q50", "edge"])
@pytest.mark.parametrize("name,hs,vs,cs", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_host_build_equals_libjpeg(c9, name, hs, vs, cs, kind):
    """every layout x size x table kind: the arrays of the host build are libjpeg's, bit for bit"""
    rng = np.random.default_rng([len(name), hs[0], vs[0], cs, len(kind)])
    for size in SIZES:
        px = pixels(rng, size, len(hs))
        q = tables(kind, len(hs), pkg.synth, rng)
        want = c9.libjpeg(px, q, hs, vs, cs)
        got = c9.host(px, q, hs, vs, cs)
        assert want["image_size"] == size and want["hsamp"] == got["hsamp"] and want["vsamp"] == got["vsamp"]
        for ci in range(len(hs)):
            assert np.array_equal(want["quants"][ci], q[ci])
        assert_same_arrays(got["coefs"], want["coefs"], f"{name} {size} {kind}")


def test_edge_tables_hold_every_value():
    rng = np.random.default_rng(3)
    t = np.concatenate(tables("edge", 3, pkg.synth, rng))
    assert set(t.tolist()) == set(EDGE_VALUES)


def test_all_colours_through_the_conversion(c9):
    """4096 x 4096 4:4:4 with each of the 2^24 RGB colours once and tables of 1: the colour conversion in full"""
    px = all_colours()
    q = tables("ones", 3, pkg.synth)
    want = c9.libjpeg(px, q, [1, 1, 1], [1, 1, 1], 3)
    got = c9.host(px, q, [1, 1, 1], [1, 1, 1], 3)
    assert_same_arrays(got["coefs"], want["coefs"], "all colours")


def _blocks():
    rng = np.random.default_rng(11)
    b = rng.integers(0, 256, (4096, 64)).astype(np.uint8)
    i = np.arange(64)
    b[0] = 0
    b[1] = 255
    b[2] = (((i >> 3) + i) & 1) * 255                       # checkerboard
    b[3] = 255 - b[2]
    b[4] = (i & 1) * 255                                    # vertical stripes
    b[5] = ((i >> 3) & 1) * 255                             # horizontal stripes
    b[6:262] = rng.choice(np.array([0, 255], np.uint8), (256, 64))       # extreme blocks
    return b


def test_fdct_islow_blocks(c9):
    """the exported jpeg_fdct_islow on random, all-0, all-255, checkerboard and two-valued blocks"""
    b = _blocks()
    want = c9.fdct("libjpeg", b)
    got = c9.fdct("host", b)
    assert np.array_equal(got, want)
    assert want[0, 0] == -8192 and want[1, 0] == 8128 and not want[0, 1:].any()       # (the scale by 8, the centre)
    assert np.abs(want).max() < 1 << 17                                               # the quantiser's proven domain


def test_quantiser_equals_integer_division(c9):
    """qc_quant's reciprocal and correction against the plain division over |w| < 2^17 (tables 1..1024 and a sweep)"""
    assert c9._run(c9.host_exe, "quantcheck").strip() == "mismatches=0"


def test_sanitizer_build_runs_clean(c9):
    """the same stand-alone program under -fsanitize=address,undefined: blocks, the quantiser's inputs at both ends,
    and the image sizes where the edge rules are at work"""
    exe = c9.build_host("compress_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                              "-fno-omit-frame-pointer"])
    b = _blocks()[:300]
    assert np.array_equal(c9.fdct("host", b, exe=exe), c9.fdct("libjpeg", b))
    rng = np.random.default_rng(21)
    for name, hs, vs, cs in LAYOUTS:
        for size in [(1, 1), (33, 18), (65, 66)]:
            px = pixels(rng, size, len(hs))
            q = tables("edge", len(hs), pkg.synth, rng)
            got = c9.host(px, q, hs, vs, cs, exe=exe)
            assert_same_arrays(got["coefs"], c9.libjpeg(px, q, hs, vs, cs)["coefs"], f"sanitizer build, {name} {size}")


@pytest.mark.parametrize("name,hs,vs,cs", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_libjpeg_scan_of_pixels_equals_its_scan_of_the_arrays(c9, tmp_path_factory, name, hs, vs, cs):
    """libjpeg against itself: the scan of the file jpeg_write_scanlines wrote is the scan jpeg_write_coefficients
    writes from that file's arrays -- the dummy-block rule of the entropy coder also holds for files made from pixels"""
    enc = LibJpeg9Enc(tmp_path_factory.mktemp("enc"))
    rng = np.random.default_rng(31)
    for size in [(7, 9), (33, 18), (70, 50)]:
        px = pixels(rng, size, len(hs))
        q = tables("q50", len(hs), pkg.synth)
        im = c9.libjpeg(px, q, hs, vs, cs, keep_file=True)
        first = parse_jpeg(im["file"].read_bytes())
        again = parse_jpeg(enc.write(im))
        assert first["segment"] == again["segment"], f"{name} {size}"
        assert first["dc"] == again["dc"] and first["ac"] == again["ac"]


def _job(hip, size, hs, vs, cs, shapes=None, q=None):
    n = len(hs)
    if shapes is None:
        mh, mv = (1, 1) if n == 1 else (max(hs), max(vs))
        shapes = [(-(-size[1] * (1 if n == 1 else vs[ci]) // (8 * mv)), -(-size[0] * (1 if n == 1 else hs[ci]) // (8 * mh)))
                  for ci in range(n)]
    q = q or [np.full(64, 3, np.uint16)] * n
    return hip.device_job([0x1000 * (ci + 1) for ci in range(n)], shapes, q, hsamp=hs, vsamp=vs, colorspace=cs,
                          image_size=size)


@pytest.mark.parametrize("name,hs,vs,cs", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_info_reports_libjpegs_geometry(c9, hip, name, hs, vs, cs):
    rng = np.random.default_rng(41)
    for size in [(1, 1), (33, 18), (70, 50)]:
        want = c9.libjpeg(pixels(rng, size, len(hs)), tables("ones", len(hs), pkg.synth), hs, vs, cs)
        (per,), nbytes = hip.compress_batch_info([_job(hip, size, hs, vs, cs)])
        assert (per["width"], per["height"], per["channels"]) == (size[0], size[1], len(hs))
        assert per["layout"] == {1: 0, 3: 1, 2: 2}[cs]
        assert list(zip(per["hblk"], per["wblk"])) == [c.shape[:2] for c in want["coefs"]]
        assert nbytes > 0
    one = hip.compress_batch_info([_job(hip, (33, 18), hs, vs, cs)])[1]
    assert hip.compress_batch_info([_job(hip, (33, 18), hs, vs, cs)] * 3)[1] == 3 * one


def _code(hip, jobs, fancy=False):
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.compress_batch_info(jobs, fancy)
    return e.value.code


def test_info_rejects_unsupported_layouts_and_fancy_downsampling(hip):
    ok = _job(hip, (32, 16), [2, 1, 1], [2, 1, 1], 3)
    assert _code(hip, [ok], fancy=True) == -4                             # libjpeg 9's default: out of scope
    assert "fancy" in hip.lib.qs_hip_last_error().decode()
    assert _code(hip, [_job(hip, (32, 16), [1, 1, 1, 1], [1, 1, 1, 1], 4)]) == -4       # CMYK
    assert _code(hip, [_job(hip, (32, 16), [2, 2, 2], [2, 2, 2], 3)]) == -4             # chroma factors of 2
    assert _code(hip, [_job(hip, (48, 16), [3, 1, 1], [1, 1, 1], 3)]) == -4             # 3x1 luma
    assert _code(hip, [_job(hip, (48, 16), [2, 1, 1], [4, 1, 1], 3)]) == -4             # 2x4 luma
    assert _code(hip, [_job(hip, (48, 16), [4, 1, 1], [2, 1, 1], 3)]) == -4             # 4x2 luma
    assert _code(hip, [_job(hip, (32, 16), [1, 1, 1], [1, 1, 1], 7)]) == -4             # big-gamut YCC
    assert _code(hip, [_job(hip, (32, 16), [1], [1], 3)]) == -4                         # one component, YCbCr
    assert _code(hip, [ok, _job(hip, (32, 16), [1, 1, 1, 1], [1, 1, 1, 1], 4)]) == -4   # one bad job fails the batch
    assert "job 1" in hip.lib.qs_hip_last_error().decode()


def test_info_rejects_invalid_jobs(hip):
    job = _job(hip, (32, 16), [2, 1, 1], [2, 1, 1], 3)
    job.image_width = 0
    assert _code(hip, [job]) == -2                                        # a missing image size
    job = _job(hip, (32, 16), [2, 1, 1], [2, 1, 1], 3)
    job.image_width = 40                                                  # more pixels than the arrays hold
    assert _code(hip, [job]) == -2
    job = _job(hip, (32, 16), [2, 1, 1], [2, 1, 1], 3)
    job.has_quant[1] = 0
    assert _code(hip, [job]) == -2
    job = _job(hip, (32, 16), [2, 1, 1], [2, 1, 1], 3)
    job.quant[2][63] = 0                                                  # a quantiser of 0
    assert _code(hip, [job]) == -2
    assert _code(hip, []) == -2


def test_torch_layer_argument_errors_need_no_gpu():
    """ValueError for fancy=True and for unsupported sampling is decided before any device is touched"""
    tq = pkg.torch_qs
    with pytest.raises(ValueError, match="fancy"):
        tq.compress_batch([dict(pixels=None)], fancy=True)
    with pytest.raises(ValueError):
        tq.compress_batch([])
