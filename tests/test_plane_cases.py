"""The expectations of tests/test_gpu_plane_kernels.py without a GPU: the oracle port against the reference on every
adversarial plane-layer case (block() under every flag set, JOINT_YUV and LOW_QUALITY with their fdct_clamp, the
IDCT, fdct_float with roundf, upsample_row), plus checks of the numpy restatements and of the case generator.
Running these also records (QS_RECORD_REFERENCE=1) every reference call the GPU module makes."""
import numpy as np
import pytest

import plane_cases as pc


def _eq(a, b, what):
    msg = pc.first_diff(a, b, what)
    assert msg is None, msg


@pytest.mark.parametrize("name", [c[0] for c in pc.PASS_B_CASES + pc.UNREACHABLE_B_CASES])
def test_case_coefficients_are_reachable(name):
    """every coefficient lies in the interval of a multiple of its quantiser that passes the range check, and every
    kind of the case occurs; the huge table reaches +-32767"""
    q, c = pc.pass_b_case(name)
    qe = pc.eff(q).astype(np.int64)
    v = c.astype(np.int64)
    a = np.where(v < 0, -((-v + qe // 2) // qe), (v + qe // 2) // qe) * qe     # nearest multiple, ties away from zero
    lo, hi = pc._interval(a, qe)
    assert ((v >= lo) & (v <= hi)).all()
    assert ((a >= -0x800) & (a <= 0x7ff)).all()
    if name == "max-table":
        assert q.max() == 0x7ff
    if name == "huge-table":
        assert v.max() == 32767 and v.min() == -32767
    assert (pc.pass_b_case(name)[1] == c).all(), "the generator must be deterministic"


def test_pass_a_planes(oracle, reference):
    for name in [c[0] for c in pc.PASS_B_CASES]:
        _eq(pc.ref_plane(oracle, pc.pass_b_case(name)[1]), pc.ref_plane(reference, pc.pass_b_case(name)[1]), name)
    for s in (51, 52, 53):
        c = pc.raw_int16_case(s)
        _eq(pc.ref_plane(oracle, c), pc.ref_plane(reference, c), f"raw int16 {s}")


@pytest.mark.parametrize("name,stop", pc.STATUS_CASES)
def test_status_cases(oracle, reference, name, stop):
    """the range check: the reference's driver stops (returns 1) exactly on the cases that trip"""
    q, c = pc.status_case(name)
    assert pc.stops(q, c) == stop
    w = pc.dequant_wrap(q, c)
    _eq(pc.ref_plane(oracle, w), pc.ref_plane(reference, w), name)
    assert reference.do_quantsmooth([c], [q], 0, 1)["ret"] == int(stop)


@pytest.mark.parametrize("name", [c[0] for c in pc.PASS_B_CASES + pc.UNREACHABLE_B_CASES])
def test_pass_b_blocks(oracle, reference, name):
    for flags in pc.PASS_B_FLAGS:
        for luma in (1, 0):
            want = pc.pass_b_expected(reference, name, flags, luma)
            _eq(pc.pass_b_expected(oracle, name, flags, luma), want, f"{name} flags={flags} luma={luma}")
            if luma:
                c = want.reshape(pc.pass_b_case(name)[1].shape)
                _eq(pc.ref_plane(oracle, c), pc.ref_plane(reference, c), f"{name} next plane")


@pytest.mark.parametrize("name", ["std-mixed-kinds", "camera-checker", "max-table", "huge-table", "zeros-table"])
def test_joint_and_lowq_blocks(oracle, reference, name):
    for flags in (0, pc.F_DIAG, pc.F_NOREB):
        _eq(pc.joint_expected(oracle, name, flags), pc.joint_expected(reference, name, flags), f"joint {name} {flags}")
        for luma in (1, 0):
            _eq(pc.lowq_expected(oracle, name, flags, luma, False), pc.lowq_expected(reference, name, flags, luma, False),
                f"lowq {name} {flags} {luma}")
        _eq(pc.lowq_expected(oracle, name, flags, 0, True), pc.lowq_expected(reference, name, flags, 0, True),
            f"lowq+plane2 {name} {flags}")


@pytest.mark.parametrize("name", [n for n, *_ in pc.LARGE_CASES])
def test_large_case_samples(oracle, reference, name):
    """the sampled blocks of the large planes, and the oracle's pass A they read against the reference's"""
    q, c = pc.large_case(name)
    want, pos = pc.large_sample_expected(reference, oracle, name, pc.F_DIAG)
    got, _ = pc.large_sample_expected(oracle, oracle, name, pc.F_DIAG)
    _eq(got, want, name)
    plane = pc.apron_view(pc.oracle_plane(oracle, q, c), c.shape[1], c.shape[0])
    by = sorted({p[1] for p in pos})[:3] + [c.shape[0] - 1]
    for y in by:                    # the oracle's plane, block rows of the sample, against the reference's IDCT
        rows = pc.pixels(oracle, c[y:y + 1])
        _eq(plane[1 + y * 8:9 + y * 8, 1:-1], rows, f"{name} block row {y}")
    _eq(pc.oracle_band_smooth(oracle, q, c[:2], pc.oracle_plane(oracle, q, c[:2]), pc.F_DIAG),
        pc.pass_b_expected_plain(oracle, q, c[:2], pc.F_DIAG), f"{name} band_smooth")


@pytest.mark.parametrize("w,h,ws,hs", pc.UPSAMPLE_CASES)
def test_upsample_and_downsample(oracle, reference, w, h, ws, hs):
    g, ycoef, ccoef, luma, lowres, chroma = pc.upsample_inputs(reference, w, h, ws, hs, seed=w * h)
    go = pc.upsample_inputs(oracle, w, h, ws, hs, seed=w * h)
    for a, b in zip((luma, lowres, chroma), go[3:]):
        _eq(b, a, "inputs")
    ww, hh = g["ww"], g["hh"]
    whole = pc.upsample_expected(reference, g, luma, lowres, chroma, ws, hs)
    _eq(pc.upsample_expected(oracle, g, luma, lowres, chroma, ws, hs)[:hh, :ww], whole[:hh, :ww], "upsample")
    for f in pc.first_rows_list(g["h1"]):
        want = pc.upsample_expected(reference, g, luma, lowres, chroma, ws, hs, first_rows=f)
        _eq(pc.upsample_expected(oracle, g, luma, lowres, chroma, ws, hs, first_rows=f)[:hh, :ww], want[:hh, :ww],
            f"upsample first_rows={f}")
        if f == min(8, g["h1"]):    # the band view of the whole image is the reference's own
            _eq(want[:hh, :ww], whole[:hh, :ww], "first_rows = the first strip")
    if (ws, hs) == (2, 2):          # the reference's 4:2:0 fast path (a + 2) >> 2 is the box mean
        px = pc.pixels(reference, ycoef).astype(np.int64)
        d = pc.downsample_expected(pc.pixels(reference, ycoef), g["cwb"] * 8, g["chb"] * 8, 2, 2)
        y2, x2 = px.shape[0] // 2, px.shape[1] // 2
        fast = (px[0:2 * y2:2, 0:2 * x2:2] + px[1:2 * y2:2, 0:2 * x2:2] + px[0:2 * y2:2, 1:2 * x2:2]
                + px[1:2 * y2:2, 1:2 * x2:2] + 2) >> 2
        _eq(d[1:y2 + 1, 1:x2 + 1], fast, "4:2:0 fast path")


def test_fdct_roundf(oracle, reference):
    blocks = pc.fdct_blocks_of(pc.fdct_case())
    _eq(pc.fdct_expected(oracle, blocks), pc.fdct_expected(reference, blocks), "fdct")
    x = np.array([0.5, -0.5, 1.5, -2.5, 2.4999998, -0.49999997, 3.0], np.float32)
    assert pc.c_roundf(x).tolist() == [1.0, -1.0, 2.0, -3.0, 2.0, -0.0, 3.0]
