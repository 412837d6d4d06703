"""The decode's triangle mode (upsampling="triangle": libjpeg-turbo's chroma upsampling) without
a GPU: the filter of csrc/qs_decode.h compiled for the host (tests/decode_triangle_host.cpp: whole images tile by tile as
the kernel's workgroups take them) against the recorded libjpeg-turbo pixels of tests/golden/triangle, live against
Pillow's libjpeg-turbo where Pillow imports, once under -fsanitize=address,undefined, and the validation of the new
options (qs_hip_decode_opts, decode(..., upsampling=...))."""
import ctypes as C

import numpy as np
import pytest

import jpegqs_pkg
from triangle_oracle import LAYOUTS, SIZES, TriHost, have_pillow, load_fixtures, pillow_decode, with_junk

pkg = jpegqs_pkg.load()


@pytest.fixture(scope="module")
def fixtures():
    f = load_fixtures()
    assert len(f) >= 60
    return f


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return TriHost(tmp_path_factory.mktemp("tri"))


def _blame(name, got, want):
    bad = np.argwhere(got != want)
    y, x, c = bad[0]
    return f"{name}: {len(bad)} samples differ, first at (y, x, channel) = ({y}, {x}, {c}): {got[y, x, c]} != turbo {want[y, x, c]}"


def test_fixtures_cover_the_layouts_sizes_and_the_filter_conditions(fixtures):
    names = {f["name"] for f in fixtures}
    for size in SIZES:
        assert f"ycc22_{size[0]}x{size[1]}" in names
    for layout in LAYOUTS:
        assert any(n.startswith(layout[0] + "_") for n in names), layout[0]
    for lay in ("ycc21", "ycc12"):
        assert {f"{lay}_{w}x{h}" for w, h in SIZES if (w, h) != (141, 93)} <= names
    assert {"sat22_66x18", "sat21_66x18", "sat12_66x18"} <= names
    for f in fixtures:                                      # the saturating cases clip on both sides, in both chroma planes
        if f["name"].startswith("sat"):
            for ci in (1, 2):
                assert f["ycc"][..., ci].min() == 0 and f["ycc"][..., ci].max() == 255, f["name"]


def test_host_filter_equals_the_recorded_turbo_pixels(fixtures, host):
    ims = [f["im"] for f in fixtures]
    for f, px in zip(fixtures, host.run(ims)):
        assert px.shape == f["pixels"].shape, f["name"]
        assert np.array_equal(px, f["pixels"]), _blame(f["name"], px, f["pixels"])
    with_ycc = [f for f in fixtures if f["ycc"] is not None]
    assert len(with_ycc) >= 30
    for f, c in zip(with_ycc, host.run([f["im"] for f in with_ycc], planes=True)):
        assert np.array_equal(c, f["ycc"]), _blame(f["name"] + " (components)", c, f["ycc"])


def test_junk_outside_the_geometry_reaches_no_pixel(fixtures, host):
    """arrays two block columns wider and one block row taller, every block outside libjpeg's geometry full of large
    coefficients: the clamp is at the downsampled size, so the same pixels"""
    some = [f for f in fixtures if f["im"]["image_size"] in ((5, 5), (17, 17), (65, 17), (129, 33), (130, 34))]
    assert len(some) >= 20
    for f, px in zip(some, host.run([with_junk(f["im"]) for f in some])):
        assert np.array_equal(px, f["pixels"]), _blame(f["name"] + " (padded arrays)", px, f["pixels"])


def test_host_filter_equals_pillow_live(fixtures, host, tmp_path):
    """the same comparison against the libjpeg-turbo Pillow carries here, SIMD and C code, where Pillow imports"""
    if not have_pillow():
        pytest.skip("Pillow with libjpeg-turbo is not installed")
    from encode_oracle import LibJpeg9Enc
    enc = LibJpeg9Enc(tmp_path)
    some = [f for f in fixtures if f["im"]["image_size"][0] <= 65]
    files = [enc.write(f["im"]) for f in some]
    got = host.run([f["im"] for f in some])
    comp = host.run([f["im"] for f in some], planes=True)
    for simd in (True, False):
        for f, g, c, (px, ycc) in zip(some, got, comp, pillow_decode(files, tmp_path, simd=simd)):
            assert np.array_equal(px, f["pixels"]), f"{f['name']}: Pillow (simd={simd}) no longer gives the recorded pixels"
            assert np.array_equal(g, px), _blame(f"{f['name']} (simd={simd})", g, px)
            if ycc is not None:
                assert np.array_equal(c, ycc), _blame(f"{f['name']} components (simd={simd})", c, ycc)


def test_sanitizer_build_over_the_fixtures(fixtures, tmp_path):
    """the stand-alone program with -fsanitize=address,undefined, once over every fixture and its padded variant: no
    report (the planes are heap blocks of the kernel's size), the same pixels"""
    san = TriHost(tmp_path, sanitize=True)
    ims = [f["im"] for f in fixtures] + [with_junk(f["im"], 1, 2, seed=9) for f in fixtures]
    for f, px in zip(fixtures + fixtures, san.run(ims)):
        assert np.array_equal(px, f["pixels"]), _blame(f["name"], px, f["pixels"])


# ---- the options -------------------------------------------------------------------------------------------------------

def _job(hip, hs=2, vs=2, size=(33, 17)):
    w, h = size
    shapes = [(-(-h // 8), -(-w // 8))] + [(-(-h // (8 * vs)), -(-w // (8 * hs)))] * 2
    return hip.device_job([0x1000 * (i + 1) for i in range(3)], shapes, [np.ones(64, np.uint16)] * 3, hsamp=[hs, 1, 1],
                          vsamp=[vs, 1, 1], colorspace=3, image_size=size)


def test_opts_validation_needs_no_device():
    hipqs = pkg.hipqs
    hip = pkg.HipQS()
    assert hip.lib.qs_hip_abi_version() == 7
    assert (hipqs.UPSAMPLE_DCT, hipqs.UPSAMPLE_TRIANGLE) == (0, 1) and C.sizeof(hipqs.DecodeOpts) == 4
    jobs = [_job(hip), _job(hip, 2, 1), _job(hip, 1, 2)]
    plain = hip.decode_batch_info(jobs)
    assert hip.decode_batch_info(jobs, [None, None, None]) == plain          # opts[i] NULL: dct
    assert hip.decode_batch_info(jobs, ["triangle", "dct", None]) == plain   # one batch may mix modes; same geometry
    assert hip.decode_batch_info(jobs, [1, 0, hipqs.DecodeOpts(1)]) == plain
    # opts NULL: the call itself
    per = (hipqs.DecodeInfo * 3)()
    total = C.c_size_t(0)
    assert hip.lib.qs_hip_decode_device_batch_info_opts(hip._job_ptrs(jobs), 3, None, per, C.byref(total)) == 0
    assert int(total.value) == plain[1] and [int(p.width) for p in per] == [33, 33, 33]
    for bad in (2, -1, 1 << 20):
        with pytest.raises(hipqs.QsHipError) as e:
            hip.decode_batch_info(jobs, [None, bad, None])
        assert e.value.code == -2 and "upsampling" in str(e.value) and "job 1" in str(e.value)
        with pytest.raises(hipqs.QsHipError) as e:                            # prepare: refused before any device is touched
            hip.decode_batch_prepare(jobs, 0x10000, 1 << 20, None, [bad, None, None])
        assert e.value.code == -2
    with pytest.raises(ValueError):
        hip.decode_batch_info(jobs, ["bilinear", None, None])
    with pytest.raises(ValueError):
        hip.decode_batch_info(jobs, ["triangle"])                             # one entry per job


def test_python_keyword_is_checked_before_anything_else():
    tq = pkg.torch_qs
    for bad in ("fancy", "", None, 1, "TRIANGLE"):
        with pytest.raises(ValueError, match="upsampling"):
            tq.decode([], None, image_size=(8, 8), upsampling=bad)
        with pytest.raises(ValueError, match="upsampling"):
            tq.decode_batch([dict(coefs=[], image_size=(8, 8))], upsampling=bad)
    with pytest.raises(ValueError, match="image 0: upsampling"):
        tq.decode_batch([dict(coefs=[], image_size=(8, 8), upsampling="box")])
