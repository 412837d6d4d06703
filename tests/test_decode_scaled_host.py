"""The device decode at libjpeg 9's reduced sizes (scale_denom 2, 4, 8) without a GPU: the host
build of the code a lane runs (tests/decode_scaled_host.cpp over csrc/qs_decode.h) against libjpeg 9's exported IDCTs and
its whole-image scaled decodes (tests/libjpeg9_decode_scaled.c), the same program under the address and
undefined-behaviour sanitizers, and the ABI and option checks that touch no device."""
import ctypes as C

import numpy as np
import pytest

import jpegqs_pkg
import decode_scaled_oracle as so
from decode_cases import header_constant
from decode_oracle import synth_image

pkg = jpegqs_pkg.load()


@pytest.fixture(scope="module")
def lj9(tmp_path_factory):
    return so.LibJpeg9Scaled(tmp_path_factory.mktemp("lj9s"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return so.ScaledHost(tmp_path_factory.mktemp("hosts"))


@pytest.fixture(scope="module")
def hip():
    return pkg.HipQS()


# ---- 1. the nine IDCTs, function by function -----------------------------------------------------------------------------

def _same(lj9, host, kind, coefs, tables, what):
    want, got = lj9.blocks(kind, coefs, tables), host.blocks(kind, coefs, tables)
    bad = np.flatnonzero((want != got).any(axis=(1, 2)))
    assert not len(bad), f"jpeg_idct_{kind}, {what}: {len(bad)} of {len(coefs)} blocks differ, first {int(bad[0])}"


@pytest.mark.parametrize("kind", so.KINDS)
def test_idct_on_random_blocks(lj9, host, kind):
    _same(lj9, host, kind, *so.random_blocks(sum(map(ord, kind))), "random blocks")


@pytest.mark.parametrize("kind", so.KINDS)
def test_idct_on_extreme_blocks(lj9, host, kind):
    """+-32767 and -32768 against tables from 0 to 65535: the 2-point and 1-point forms' own shifts and range-limit
    lookups, the 64-bit pass 1 of 4x4 / 8x4 / 4x8, sums that pass int32 in the kernels that need only their low bits"""
    _same(lj9, host, kind, *so.extreme_blocks(7), "extreme blocks")


@pytest.mark.parametrize("kind", ["4x4", "8x4", "4x8"])
def test_idct_around_the_pass1_bound(lj9, host, kind):
    coefs, tables, fast = so.bound_blocks(kind)
    assert fast.any() and (~fast).any()
    _same(lj9, host, kind, coefs, tables, "sign-aligned blocks around the 32-bit bound of pass 1")


def test_the_bounds_are_those_the_row_norms_give(host):
    info = host.info()
    # the 4-point pass 1's odd part: rows (FIX(0.541196100) + FIX(0.765366865), FIX(0.541196100)) = (10703, 4433) and
    # (FIX(0.541196100), FIX(0.541196100) - FIX(1.847759065)) = (4433, -10704)
    assert info["l1_4"] == max(10703 + 4433, 4433 + 10704) == so.L1_4 == 15137
    # the largest x with l1 * x + 2^10 <= 2^31 - 1: the sum, with the rounding term, is an int32 up to there and not beyond
    bound = (2 ** 31 - 1 - 2 ** 10) // info["l1_4"]
    assert info["l1_4"] * bound + 2 ** 10 <= 2 ** 31 - 1 < info["l1_4"] * (bound + 1) + 2 ** 10
    assert info["fast_bound4"] == bound == so.BOUND4 == header_constant("QS_DEC_FAST_BOUND4")
    assert info["fast_bound"] == header_constant("QS_DEC_FAST_BOUND") == 16384       # 4x8: the 8-point pass 1 of section 12
    assert (info["tile_w"], info["tile_h"]) == (so.TILE_W, so.TILE_H)


# ---- 2. whole images ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("denom", so.DENOMS)
def test_whole_images_against_libjpeg(lj9, host, denom):
    """every layout at the small sizes and at the edges of the tile's input footprint, arrays larger than the image
    needs with junk outside the geometry"""
    cases = so.expected_images(lj9, denom)
    assert len(cases) == len(so.LAYOUTS) * 15 and max(im["image_size"] for _, im, _ in cases) <= (513, 129)
    for label, im, want in cases:
        got = host.decode(im, denom)
        assert got.shape == want.shape and np.array_equal(got, want), label


def test_output_size_table():
    assert [so.scaled_size((141, 93), d) for d in so.DENOMS] == [(71, 47), (36, 24), (18, 12)]


# ---- 3. the same program under the sanitizers -----------------------------------------------------------------------------

def test_host_program_under_address_and_undefined_sanitizers(lj9, tmp_path_factory):
    """a stand-alone program: the output, each tile's planes and rows and every coefficient array are heap blocks of
    exactly the kernel's sizes, so a read or store outside them ends the run"""
    asan = so.ScaledHost(tmp_path_factory.mktemp("asan"), sanitize=True)
    for kind in so.KINDS:
        c, t = so.extreme_blocks(11)
        assert np.array_equal(asan.blocks(kind, c, t), lj9.blocks(kind, c, t)), kind
    for denom in so.DENOMS:
        for label, im in so.image_cases(denom):
            if im["image_size"] in ((1, 1), (9, 9), (15, 17), (141, 93), (64 * denom + 1, 16 * denom + 1),
                                    (64 * denom - 1, 16 * denom - 1)):
                assert np.array_equal(asan.decode(im, denom), lj9.decode(im, denom)), label


# ---- 4. ABI and options, no device ---------------------------------------------------------------------------------------

def _job(hip, im):
    return hip.device_job([0x1000 * (ci + 1) for ci in range(len(im["coefs"]))], [c.shape[:2] for c in im["coefs"]],
                          im["quants"], hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"],
                          image_size=im["image_size"])


def test_option_records_and_abi(hip):
    assert C.sizeof(pkg.hipqs.DecodeOpts) == 4                             # the old record keeps its size
    assert C.sizeof(pkg.hipqs.DecodeScaleOpts) == 8
    assert [f for f, _ in pkg.hipqs.DecodeScaleOpts._fields_] == ["upsampling", "scale_denom"]
    assert hip.lib.qs_hip_abi_version() == 7
    for name in ("qs_hip_decode_device_batch_info_scaled", "qs_hip_decode_device_batch_prepare_scaled"):
        assert hasattr(hip.lib, name)


def test_info_reports_the_scaled_sizes(hip):
    rng = np.random.default_rng(12)
    ycc = synth_image(rng, (141, 93), [2, 1, 1], [2, 1, 1], 3)
    gray = synth_image(rng, (513, 129), [1], [1], 1)
    jobs = [_job(hip, ycc), _job(hip, gray)]
    full, nbytes = hip.decode_batch_info(jobs)
    for d, a, b in ((1, (141, 93), (513, 129)), (2, (71, 47), (257, 65)), (4, (36, 24), (129, 33)), (8, (18, 12), (65, 17))):
        per, nb = hip.decode_batch_info(jobs, scales=[d, d])
        assert [(p["width"], p["height"], p["channels"], p["layout"]) for p in per] == [a + (3, 1), b + (1, 0)]
        assert nb == nbytes                                                 # the workspace does not depend on the scale
    per, _ = hip.decode_batch_info(jobs, scales=[None, 4])                  # NULL: full size
    assert (per[0]["width"], per[1]["width"]) == (141, 129)
    assert hip.decode_batch_info(jobs, scales=[1, 1])[0] == full
    per, _ = hip.decode_batch_info(jobs, opts=["triangle", "dct"], scales=[1, 8])   # one batch, both modes at 1
    assert (per[0]["width"], per[1]["width"]) == (141, 65)


def _code(hip, jobs, **kw):
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.decode_batch_info(jobs, **kw)
    return e.value.code


def test_refusals_of_the_c_abi(hip):
    rng = np.random.default_rng(13)
    jobs = [_job(hip, synth_image(rng, (32, 16), [2, 1, 1], [1, 1, 1], 3))]
    for bad in (0, 3, 5, 6, 7, 16, -2):
        assert _code(hip, jobs, scales=[bad]) == -2, bad                    # QS_HIP_EINVAL
    for d in (2, 4, 8):
        assert _code(hip, jobs, opts=["triangle"], scales=[d]) == -4, d     # QS_HIP_ENOTSUP, a stated limit
        assert "full size" in hip.lib.qs_hip_last_error().decode()
    cmyk = [_job(hip, synth_image(rng, (32, 16), [1, 1, 1, 1], [1, 1, 1, 1], 4))]
    assert _code(hip, cmyk, scales=[2]) == -4                               # the layouts are those of the full size


def test_value_errors_of_the_torch_interface():
    tq = pkg.torch_qs
    im = dict(coefs=[], quants=[np.ones(64, np.uint16)], hsamp=[1], vsamp=[1], colorspace=1, image_size=(8, 8))
    for bad in (0, 3, 16, "2", 2.0, True, None):
        with pytest.raises(ValueError, match="scale_denom"):
            tq.decode_batch([im], scale_denom=bad)
        with pytest.raises(ValueError, match="scale_denom"):
            tq.decode_batch([dict(im, scale_denom=bad if bad is not None else 5)])
    with pytest.raises(ValueError, match="scale_denom"):
        tq.decode_batch([im], scale_denom=[2, 2])
    with pytest.raises(ValueError, match="triangle"):
        tq.decode_batch([im], upsampling="triangle", scale_denom=2)
    with pytest.raises(ValueError, match="triangle"):
        tq.decode_batch([dict(im, upsampling="triangle"), im], scale_denom=[4, 1])
