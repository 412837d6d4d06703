"""The device decode's triangle mode (torch_qs.decode / decode_batch with upsampling="triangle",
qs_hip_decode_device_batch_prepare_opts) on the GPU against the recorded libjpeg-turbo pixels of tests/golden/triangle
(tests/golden/make_triangle_golden.py; checked on the CPU by tests/test_decode_triangle_host.py).  Only the fixtures are
read: neither Pillow nor libjpeg-turbo is needed here.  The jobs that stay in the dct mode are compared with libjpeg 9
(tests/libjpeg9_decode.c), as the rest of the decode's tests do.  Every output buffer sits between sentinel margins."""
import numpy as np
import pytest

import jpegqs_pkg
from decode_oracle import LibJpeg9
from helpers import MARGIN, Guarded
from triangle_oracle import kw, load_fixtures, with_junk

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tq():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible to torch")
    return pkg.torch_qs


@pytest.fixture(scope="module")
def fixtures():
    return load_fixtures()


@pytest.fixture(scope="module")
def by_name(fixtures):
    return {f["name"]: f for f in fixtures}


def _dev(im):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in im["coefs"]]


def _decode(tq, ims, modes=None, **more):
    """decode_batch with every output between sentinel margins -> host pixels per image"""
    shapes = [(im["image_size"][1], im["image_size"][0], 1 if len(im["coefs"]) == 1 else 3) for im in ims]
    guards = [Guarded(h * w * c) for h, w, c in shapes]
    batch = [dict(coefs=_dev(im), quants=im["quants"], **kw(im)) for im in ims]
    if modes is not None:
        for b, m in zip(batch, modes):
            b["upsampling"] = m
    tq.decode_batch(batch, outs=[g.view.view(s) for g, s in zip(guards, shapes)], **more)
    torch.cuda.synchronize()
    for k, g in enumerate(guards):
        try:
            g.check()
        except AssertionError as e:
            raise AssertionError(f"image {k}: {e}") from None
    return [g.view.cpu().numpy().reshape(s) for g, s in zip(guards, shapes)]


def _blame(name, got, want, who="turbo"):
    bad = np.argwhere(got != want)
    y, x, c = bad[0]
    return f"{name}: {len(bad)} samples differ, first at (y, x, channel) = ({y}, {x}, {c}): {got[y, x, c]} != {who} {want[y, x, c]}"


def test_every_fixture_in_one_batch(tq, fixtures):
    """every layout and size, the saturating blocks among them: more jobs than one launch chunk, all in triangle mode"""
    assert len(fixtures) > 44
    got = _decode(tq, [f["im"] for f in fixtures], upsampling="triangle")
    for f, px in zip(fixtures, got):
        assert np.array_equal(px, f["pixels"]), _blame(f["name"], px, f["pixels"])


def test_single_decode_and_workspace_follow_the_mode(tq, by_name):
    """decode() itself; one Workspace through a change of mode and back: it is prepared again each time"""
    f = by_name["ycc22_17x17"]
    im, dev = f["im"], _dev(f["im"])
    ws = tq.Workspace()
    a = tq.decode(dev, im["quants"], **kw(im), upsampling="triangle", workspace=ws).cpu().numpy()
    key = ws.key
    b = tq.decode(dev, im["quants"], **kw(im), workspace=ws).cpu().numpy()
    assert ws.key != key
    c = tq.decode(dev, im["quants"], **kw(im), upsampling="triangle", workspace=ws).cpu().numpy()
    assert ws.key == key
    assert np.array_equal(a, f["pixels"]) and np.array_equal(c, f["pixels"])
    assert not np.array_equal(a, b)                          # (DCT-scaled chroma: other pixels)


def test_arrays_larger_than_the_image_with_junk_outside(tq, fixtures):
    """every array two block columns wider and one block row taller, every block outside libjpeg's geometry full of large
    coefficients: the clamp is at the downsampled size, so no junk reaches a pixel and the row stride is the array's"""
    some = [f for f in fixtures if f["im"]["image_size"] in ((2, 2), (5, 5), (17, 17), (65, 17), (129, 33), (130, 34), (141, 93))]
    assert len(some) >= 25
    got = _decode(tq, [with_junk(f["im"]) for f in some], upsampling="triangle")
    for f, px in zip(some, got):
        assert np.array_equal(px, f["pixels"]), _blame(f["name"] + " (padded arrays)", px, f["pixels"])


def test_a_batch_of_45_that_alternates_modes(tq, fixtures, tmp_path):
    """more jobs than QS_HIP_DECODE_CHUNK, dct and triangle alternating: the dct jobs are libjpeg 9's pixels (today's
    decode), the triangle jobs their fixtures"""
    lj9 = LibJpeg9(tmp_path)
    pool = [f for f in fixtures if f["name"].split("_")[0] in ("ycc22", "ycc21", "ycc12", "ycc41", "rgb22", "ycc11")]
    picks = [pool[(7 * k) % len(pool)] for k in range(45)]
    modes = ["dct" if k % 2 == 0 else "triangle" for k in range(45)]
    assert len(picks) > pkg.hipqs.DECODE_CHUNK and {f["name"].split("_")[0] for f in picks[1::2]} >= {"ycc22", "ycc21", "ycc12"}
    got = _decode(tq, [f["im"] for f in picks], modes=modes)
    for k, (f, m, px) in enumerate(zip(picks, modes, got)):
        im = f["im"]
        if m == "dct":
            want = lj9.decode(im["coefs"], im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"])
            assert np.array_equal(px, want), _blame(f"job {k} ({f['name']}, dct)", px, want, "libjpeg 9")
        else:
            assert np.array_equal(px, f["pixels"]), _blame(f"job {k} ({f['name']}, triangle)", px, f["pixels"])
    # the keyword default with per-image overrides: the same batch, the modes swapped
    swapped = _decode(tq, [f["im"] for f in picks[:6]], modes=[None, "dct", None, "dct", None, "dct"], upsampling="triangle")
    for k in (0, 2, 4):
        f, px = picks[k], swapped[k]
        assert np.array_equal(px, f["pixels"]), _blame(f"job {k} ({f['name']}, the keyword's mode)", px, f["pixels"])
    for k in (1, 3, 5):                                     # (the odd jobs ran in triangle mode above and in dct here)
        im = picks[k]["im"]
        want = lj9.decode(im["coefs"], im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"])
        assert np.array_equal(swapped[k], want), _blame(f"job {k} (dct by its own key)", swapped[k], want, "libjpeg 9")


def _turbo_rgb(ycc):
    """libjpeg-turbo's ycc_rgb_convert (jdcolor.c: five-digit constants) on (H, W, 3) components"""
    fix = lambda x: int(x * 65536 + 0.5)
    y, cb, cr = (ycc[..., k].astype(np.int64) for k in range(3))
    r = y + ((fix(1.40200) * (cr - 128) + 32768) >> 16)
    g = y + ((-fix(0.34414) * (cb - 128) + 32768 - fix(0.71414) * (cr - 128)) >> 16)
    b = y + ((fix(1.77200) * (cb - 128) + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def test_replacement_chroma_under_both_stops(tq, by_name):
    """UPSAMPLE_UV jobs: with stop 1 the original 2x2 chroma is decoded in triangle mode, with stop 0 the replacement
    chroma at 1x1.  A: the 2x2 fixture as it is, stop 1.  B: the 1x1 fixture's luma over the 2x2 fixture's chroma, with the
    1x1 fixture's chroma as the replacement: stop 0 gives the 1x1 fixture's pixels, stop 1 the two fixtures' recorded
    components -- luma of the one, upsampled chroma of the other -- through turbo's colour conversion"""
    f22, f11 = by_name["ycc22_65x17"], by_name["ycc11_65x17"]
    a, b = f22["im"], f11["im"]
    assert a["coefs"][0].shape == b["coefs"][0].shape and all(np.array_equal(p, q) for p, q in zip(a["quants"], b["quants"]))
    mixed = dict(a, coefs=[b["coefs"][0], a["coefs"][1], a["coefs"][2]])
    assert np.array_equal(_turbo_rgb(f22["ycc"]), f22["pixels"])               # (the restatement above is turbo's)
    want_b1 = _turbo_rgb(np.concatenate([f11["ycc"][..., :1], f22["ycc"][..., 1:]], axis=2))
    jobs = [(a, 1, f22["pixels"]), (mixed, 0, f11["pixels"]), (mixed, 1, want_b1)]
    up = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in b["coefs"][1:]]
    result = dict(stop=torch.tensor([s for _, s, _ in jobs], dtype=torch.int32, device="cuda"),
                  images=[dict(coef_up=up, quants=im["quants"]) for im, _, _ in jobs])
    r = tq.decode_batch([dict(coefs=_dev(im), **kw(im)) for im, _, _ in jobs], result=result, upsampling="triangle")
    for k, ((im, stop, want), px) in enumerate(zip(jobs, r["images"])):
        px = px.cpu().numpy()
        assert np.array_equal(px, want), _blame(f"job {k} (stop {stop})", px, want)


def test_misaligned_output_with_an_odd_pitch(tq, by_name):
    f = by_name["ycc22_65x17"]
    im = f["im"]
    w, h = im["image_size"]
    off, pitch = 1, w * 3 + 8
    assert pitch % 2 == 1
    g = Guarded(off + h * pitch)
    view = g.view[off:off + h * pitch].view(h, pitch)[:, :w * 3].view(h, w, 3)
    assert view.data_ptr() % 4 == off and view.stride(0) == pitch
    out = tq.decode(_dev(im), im["quants"], **kw(im), out=view, upsampling="triangle")
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr()
    g.check()
    host = g.raw.cpu().numpy()[MARGIN:len(g.raw) - MARGIN]
    assert (host[:off] == 0xA5).all(), "bytes before the misaligned base changed"
    rows = host[off:].reshape(h, pitch)
    assert (rows[:, w * 3:] == 0xA5).all(), "a row gap changed"
    px = rows[:, :w * 3].reshape(h, w, 3)
    assert np.array_equal(px, f["pixels"]), _blame(f["name"], px, f["pixels"])


def test_smoothing_and_triangle_decode_in_one_captured_graph(tq, by_name):
    """quantsmooth_ and the triangle decode captured together, replayed twice on new inputs: each replay equals the eager
    run on the same inputs, and the mode is the workspace's (other pixels than the dct mode)"""
    im = by_name["ycc22_130x34"]["im"]
    flags = pkg.flags_for_quality(3)
    src = _dev(im)
    work = [t.clone() for t in src]
    ws1, ws2 = None, tq.Workspace()

    def step(mode="triangle", ws=None):
        for a, b in zip(work, src):
            a.copy_(b)
        res = tq.quantsmooth_(work, im["quants"], flags, 1, **kw(im), workspace=ws1)
        return res, tq.decode(work, **kw(im), result=res, upsampling=mode, workspace=ws2 if ws is None else ws)

    res, _ = step()                                            # eager: prepares both workspaces
    ws1 = res["workspace"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _gres, gout = step()
    rng = np.random.default_rng(12)
    for rep in range(2):
        for s, c in zip(src, im["coefs"]):
            base = torch.from_numpy(np.ascontiguousarray(c)).cuda()
            noise = torch.from_numpy(rng.integers(-1, 2, c.shape).astype(np.int16)).cuda()
            s.copy_(base + noise * (base != 0).to(torch.int16))
        g.replay()
        torch.cuda.synchronize()
        got = gout.cpu().numpy().copy()
        _, eager = step()
        _, dct = step("dct", tq.Workspace())
        torch.cuda.synchronize()
        assert np.array_equal(got, eager.cpu().numpy()), f"replay {rep}"
        assert not np.array_equal(got, dct.cpu().numpy()), f"replay {rep}: the dct mode's pixels"
