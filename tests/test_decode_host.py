"""The device decode to pixels without a GPU: the libjpeg 9 oracle against the reference's recorded decode-mode output,
and the info call (shapes, workspace, unsupported and invalid input) -- no device touched."""
import numpy as np
import pytest

import jpegqs_pkg
from decode_oracle import GOLD, LibJpeg9, synth_image

pkg = jpegqs_pkg.load()


@pytest.fixture(scope="module")
def lj9(tmp_path_factory):
    return LibJpeg9(tmp_path_factory.mktemp("lj9"))


@pytest.fixture(scope="module")
def hip():
    return pkg.HipQS()


# (source, --quality, niter) of the committed *.dec.ref.raw (oracle/decode_demo.c on the reference)
DEC_REF = [("gray64", 4, 2), ("rgb141x93_420", 3, 3), ("rgb128x96_420", 3, 2), ("rgb128x96_420", 5, 2),
           ("rgb141x93_444", 6, 3), ("gray64", 6, 2), ("rgb141x93_444", 5, 2)]


@pytest.mark.parametrize("src,quality,niter", DEC_REF)
def test_oracle_decode_of_smoothed_golden_equals_the_reference_decode_mode(lj9, oracle, src, quality, niter):
    """libjpeg 9's decode of the smoothed arrays (smoothed by the CPU oracle port) is what the reference's decode mode
    handed out: this ties the oracle to the compiled reference's recorded pixels"""
    im = lj9.read(GOLD / f"{src}.jpg")
    got = oracle.do_quantsmooth(im["coefs"], im["quants"], pkg.flags_for_quality(quality), niter, hsamp=im["hsamp"],
                                vsamp=im["vsamp"], colorspace=im["colorspace"], image_size=im["image_size"])
    assert got["ret"] == 0 and not got["up"]
    px = lj9.decode(got["coefs"], got["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"])
    want = (GOLD / f"{src}.q{quality}.dec.ref.raw").read_bytes()
    assert px.tobytes() == want


def _job(hip, im, coef_up=None):
    job = hip.device_job([0x1000 * (ci + 1) for ci in range(len(im["coefs"]))], [c.shape[:2] for c in im["coefs"]],
                         im["quants"], hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"],
                         image_size=im["image_size"])
    return job


@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 1), (1, 2), (2, 2), (4, 1)])
def test_info_shapes_and_workspace(hip, hs, vs):
    rng = np.random.default_rng(hs * 10 + vs)
    ycc = synth_image(rng, (77, 45), [hs, 1, 1], [vs, 1, 1], 3)
    rgb = synth_image(rng, (33, 9), [hs, 1, 1], [vs, 1, 1], 2)
    gray = synth_image(rng, (20, 70), [hs], [vs], 1)
    per, nbytes = hip.decode_batch_info([_job(hip, ycc), _job(hip, rgb), _job(hip, gray)])
    assert [(p["height"], p["width"], p["channels"], p["layout"]) for p in per] == \
        [(45, 77, 3, 1), (9, 33, 3, 2), (70, 20, 1, 0)]
    per1, nbytes1 = hip.decode_batch_info([_job(hip, ycc)])
    assert 0 < nbytes1 < nbytes and nbytes % 3 == 0 and nbytes == 3 * nbytes1


def _code(hip, jobs):
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.decode_batch_info(jobs)
    return e.value.code


def test_info_rejects_unsupported_layouts(hip):
    rng = np.random.default_rng(5)
    cmyk = synth_image(rng, (32, 16), [1, 1, 1, 1], [1, 1, 1, 1], 4)
    assert _code(hip, [_job(hip, cmyk)]) == -4
    ycck = synth_image(rng, (32, 16), [1, 1, 1, 1], [1, 1, 1, 1], 5)
    assert _code(hip, [_job(hip, ycck)]) == -4
    chroma2 = synth_image(rng, (32, 16), [2, 2, 2], [2, 2, 2], 3)     # 4:2:0 written with chroma factors of 2
    assert _code(hip, [_job(hip, chroma2)]) == -4
    odd = synth_image(rng, (48, 16), [3, 1, 1], [1, 1, 1], 3)          # 3x1 luma
    assert _code(hip, [_job(hip, odd)]) == -4
    bg = synth_image(rng, (32, 16), [1, 1, 1], [1, 1, 1], 7)           # big-gamut YCC (libjpeg 9 JCS_BG_YCC)
    assert _code(hip, [_job(hip, bg)]) == -4
    ok = synth_image(rng, (32, 16), [1], [1], 1)
    assert _code(hip, [_job(hip, ok), _job(hip, cmyk)]) == -4             # one bad job fails the batch
    assert "job 1" in hip.lib.qs_hip_last_error().decode()


def test_info_rejects_invalid_jobs(hip):
    rng = np.random.default_rng(6)
    im = synth_image(rng, (32, 16), [2, 1, 1], [2, 1, 1], 3)
    job = _job(hip, im)
    job.image_width = 0
    assert _code(hip, [job]) == -2                                        # a missing image size
    job = _job(hip, im)
    job.image_width = 40                                                  # more pixels than the arrays hold
    assert _code(hip, [job]) == -2
    job = _job(hip, im)
    job.has_quant[1] = 0
    assert _code(hip, [job]) == -2
    assert _code(hip, []) == -2
