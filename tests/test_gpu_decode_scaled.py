"""The device decode at libjpeg 9's reduced sizes (torch_qs.decode / decode_batch with scale_denom=2, 4, 8;
qs_hip_decode_device_batch_prepare_scaled) on the GPU, sample for sample against libjpeg 9 itself
(tests/libjpeg9_decode_scaled.c: whole-image decodes with scale_num / scale_denom = 1 / N, and its exported reduced
IDCTs).  The cases are those tests/test_decode_scaled_host.py runs through the host build; every output buffer sits
between sentinel margins."""
import numpy as np
import pytest

import decode_scaled_oracle as so
import jpegqs_pkg
from decode_cases import header_constant, small_image
from decode_oracle import GOLD, LibJpeg9
from helpers import MARGIN, Guarded
from triangle_oracle import load_fixtures

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lj9(tmp_path_factory):
    return so.LibJpeg9Scaled(tmp_path_factory.mktemp("lj9s"))


@pytest.fixture(scope="module")
def lj9full(tmp_path_factory):
    return LibJpeg9(tmp_path_factory.mktemp("lj9"))


@pytest.fixture(scope="module")
def tq():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible to torch")
    return pkg.torch_qs


def _dev(im):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in im["coefs"]]


def _kw(im):
    return dict(hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"], image_size=im["image_size"])


def _shape(im, denom):
    w, h = so.scaled_size(im["image_size"], denom)
    return h, w, 1 if len(im["coefs"]) == 1 else 3


def _decode(tq, ims, denoms, modes=None, **more):
    """decode_batch with image k at 1 / denoms[k], every output between sentinel margins -> host pixels per image"""
    shapes = [_shape(im, d) for im, d in zip(ims, denoms)]
    guards = [Guarded(h * w * c) for h, w, c in shapes]
    batch = [dict(coefs=_dev(im), quants=im["quants"], **_kw(im)) for im in ims]
    for b, m in zip(batch, modes or []):
        b["upsampling"] = m
    tq.decode_batch(batch, outs=[g.view.view(s) for g, s in zip(guards, shapes)], scale_denom=list(denoms), **more)
    torch.cuda.synchronize()
    for k, g in enumerate(guards):
        try:
            g.check()
        except AssertionError as e:
            raise AssertionError(f"image {k}: {e}") from None
    return [g.view.cpu().numpy().reshape(s) for g, s in zip(guards, shapes)]


def _diff(got, want):
    if got.shape != want.shape:
        return f"shape {got.shape} != libjpeg {want.shape}"
    bad = np.argwhere(got != want)
    y, x, c = bad[0]
    return f"{len(bad)} samples differ, first at (y, x, channel) = ({y}, {x}, {c}): {got[y, x, c]} != libjpeg {want[y, x, c]}"


# ---- whole images ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("denom", so.DENOMS)
def test_every_layout_and_size_in_one_batch(tq, lj9, denom):
    """the CPU test's cases: every layout at the small sizes and at the edges of the tile's input footprint, arrays
    larger than the image needs with junk outside the geometry; 105 jobs, three launch chunks"""
    cases = so.expected_images(lj9, denom)
    got = _decode(tq, [im for _, im, _ in cases], [denom] * len(cases))
    for (label, _, want), px in zip(cases, got):
        assert px.shape == want.shape and np.array_equal(px, want), f"{label}: " + _diff(px, want)


def test_one_batch_mixes_denominators_and_a_triangle_job(tq, lj9, lj9full):
    """denominators 1, 2, 4 and 8 side by side and, at 1, one job in the triangle mode: the reduced jobs against the
    scaled oracle, the full-size dct jobs against libjpeg 9's full decode, the triangle job against its fixture"""
    fx = {f["name"]: f for f in load_fixtures()}["ycc22_17x17"]
    ims, denoms, modes, want = [], [], [], []
    for k, (label, im) in enumerate(so.image_cases(2)[5::7]):
        d = (1, 2, 4, 8)[k % 4]
        ims.append(im)
        denoms.append(d)
        modes.append("dct")
        want.append(lj9.decode(im, d) if d > 1 else
                    lj9full.decode(im["coefs"], im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"]))
    ims.insert(3, fx["im"])
    denoms.insert(3, 1)
    modes.insert(3, "triangle")
    want.insert(3, fx["pixels"])
    assert set(denoms) == {1, 2, 4, 8} and len(ims) <= 44
    got = _decode(tq, ims, denoms, modes)
    for k, (px, w) in enumerate(zip(got, want)):
        assert px.shape == w.shape and np.array_equal(px, w), f"job {k} at 1/{denoms[k]} ({modes[k]}): " + _diff(px, w)


# ---- the IDCTs on extreme blocks and at the pass-1 bounds -------------------------------------------------------------

# (luma hs, vs, denom): the kinds with a bound are 4x4 (luma and 1x1 chroma at 1/2, 2x2 chroma at 1/4), 8x4 (2x1 and
# 4x1 chroma at 1/2) and 4x8 (1x2 chroma at 1/2); the others get extreme blocks
BLOCK_CASES = [(1, 1, 2), (2, 1, 2), (4, 1, 2), (1, 2, 2), (2, 2, 4), (2, 2, 8), (2, 1, 4), (1, 2, 4), (4, 1, 4),
               (2, 1, 8), (1, 2, 8), (4, 1, 8), (1, 1, 4), (1, 1, 8)]


@pytest.mark.parametrize("hs,vs,denom", BLOCK_CASES)
def test_extreme_and_bound_blocks_against_the_libjpeg_idcts(tq, lj9, hs, vs, denom):
    """RGB images without a colour transform put every IDCT's samples straight into the output.  Blocks within and
    beyond the 32-bit bound of pass 1 alternate from lane to lane (a checkerboard); one image per quant table"""
    lk, ck = so.kind_of(1, 1, denom)[0], so.kind_of(hs, vs, denom)[0]
    lg, cg = so.bound_groups(lk), so.bound_groups(ck)
    rng = np.random.default_rng(hs * 100 + vs * 10 + denom)
    tables = [np.full(64, 65535), np.zeros(64), rng.integers(0, 65536, 64), rng.choice(np.array([1, 255, 65535, 32768]), 64)]
    ims = []
    for t in range(4):
        groups = [lg[t % len(lg)] if lg else so.extreme_group(t, tables[t])]
        groups += [cg[(t + ci) % len(cg)] if cg else so.extreme_group(10 * ci + t, tables[(t + ci) % 4]) for ci in (1, 2)]
        ims.append(so.block_image(hs, vs, groups))
    got = _decode(tq, ims, [denom] * len(ims))
    for k, (im, px) in enumerate(zip(ims, got)):
        want = so.block_expected(lj9, im, denom)
        assert np.array_equal(px, want), f"{hs}x{vs} at 1/{denom}, luma {lk}, chroma {ck}, image {k}: " + _diff(px, want)


# ---- launches and addressing ------------------------------------------------------------------------------------------

def test_a_batch_of_45_that_alternates_denominators(tq, lj9, lj9full):
    """more jobs than QS_HIP_DECODE_CHUNK = 44: the second chunk holds one job; full-size and reduced jobs alternate, so
    both kernels' tile prefixes skip jobs in every chunk"""
    assert header_constant("QS_DEC_CHUNK") == 44
    rng = np.random.default_rng(45)
    ims, denoms = [], []
    for k in range(45):
        hs, vs, cs = so.LAYOUTS[k % len(so.LAYOUTS)]
        n = 1 if cs == 1 else 3
        size = (int(rng.integers(1, 150)), int(rng.integers(1, 70)))
        ims.append(small_image(rng, size, [hs] + [1] * (n - 1), [vs] + [1] * (n - 1), cs))
        denoms.append((1, 2, 4, 8, 2)[k % 5] if k < 44 else 4)
    got = _decode(tq, ims, denoms)
    for k, (im, d, px) in enumerate(zip(ims, denoms, got)):
        want = lj9.decode(im, d) if d > 1 else \
            lj9full.decode(im["coefs"], im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"])
        assert px.shape == want.shape and np.array_equal(px, want), f"job {k} at 1/{d}: " + _diff(px, want)


def test_misaligned_outputs_and_odd_pitches(tq, lj9):
    rng = np.random.default_rng(62)
    cases = [((131, 37), [1], [1], 1, 2), ((129, 33), [1, 1, 1], [1, 1, 1], 3, 2), ((141, 93), [2, 1, 1], [2, 1, 1], 3, 4),
             ((513, 129), [4, 1, 1], [1, 1, 1], 3, 8)]
    ims = [small_image(rng, *c[:4]) for c in cases]
    denoms = [c[4] for c in cases]
    offs = [1, 2, 3, 0]
    shapes = [_shape(im, d) for im, d in zip(ims, denoms)]
    pitches = [w * c + extra for (h, w, c), extra in zip(shapes, (0, 1, 61, 4001))]
    guards, views = [], []
    for (h, w, c), off, pitch in zip(shapes, offs, pitches):
        g = Guarded(off + h * pitch)
        guards.append(g)
        views.append(g.view[off:off + h * pitch].view(h, pitch)[:, :w * c].view(h, w, c))
        assert views[-1].data_ptr() % 4 == off and views[-1].stride(0) == pitch
    r = tq.decode_batch([dict(coefs=_dev(im), quants=im["quants"], **_kw(im), scale_denom=d) for im, d in zip(ims, denoms)],
                        outs=views)
    torch.cuda.synchronize()
    for k, (im, d, (h, w, c), off, pitch, g, v) in enumerate(zip(ims, denoms, shapes, offs, pitches, guards, views)):
        assert r["images"][k].data_ptr() == v.data_ptr()
        g.check()
        host = g.raw.cpu().numpy()[MARGIN:len(g.raw) - MARGIN]
        assert (host[:off] == 0xA5).all(), f"job {k}: bytes before the misaligned base changed"
        rows = host[off:off + h * pitch].reshape(h, pitch)
        assert (rows[:, w * c:] == 0xA5).all(), f"job {k}: the guard band between the rows changed"
        want = lj9.decode(im, d)
        assert np.array_equal(rows[:, :w * c].reshape(h, w, c), want), f"job {k}: " + _diff(rows[:, :w * c].reshape(h, w, c), want)


def test_outs_are_checked_against_the_scaled_size_and_the_workspace_follows_the_scale(tq, lj9):
    rng = np.random.default_rng(63)
    im = small_image(rng, (141, 93), [2, 1, 1], [2, 1, 1], 3)
    dev = _dev(im)
    with pytest.raises(ValueError, match="shape"):
        tq.decode(dev, im["quants"], **_kw(im), scale_denom=2, out=torch.empty((93, 141, 3), dtype=torch.uint8, device="cuda"))
    ws = tq.Workspace()
    a = tq.decode(dev, im["quants"], **_kw(im), scale_denom=2, workspace=ws)
    key = ws.key
    b = tq.decode(dev, im["quants"], **_kw(im), scale_denom=4, workspace=ws)
    assert ws.key != key
    c = tq.decode(dev, im["quants"], **_kw(im), workspace=ws)
    d = tq.decode(dev, im["quants"], **_kw(im), scale_denom=2, workspace=ws)
    assert ws.key == key
    assert tuple(a.shape) == (47, 71, 3) and tuple(b.shape) == (24, 36, 3) and tuple(c.shape) == (93, 141, 3)
    assert np.array_equal(a.cpu().numpy(), lj9.decode(im, 2)) and np.array_equal(d.cpu().numpy(), lj9.decode(im, 2))
    assert np.array_equal(b.cpu().numpy(), lj9.decode(im, 4))


# ---- UPSAMPLE_UV: two geometries, chosen on the device -------------------------------------------------------------------

def _uv_batch(lj9full):
    """UPSAMPLE_UV jobs on 4:2:0 and 4:2:2 goldens, one of each with a planted range-check trip (stop 1)"""
    ims = [lj9full.read(GOLD / f"{src}.jpg") for src in ("rgb141x93_420", "rgb128x96_420", "rgb120x88_422_rst", "rgb141x93_420")]
    for k in (1, 2):
        im = ims[k]
        im["quants"][2] = im["quants"][2].copy()
        im["quants"][2][0] = max(int(im["quants"][2][0]), 3)
        im["coefs"][2] = im["coefs"][2].copy()
        im["coefs"][2][0, 0, 0] = 1000
    return ims


@pytest.mark.parametrize("denom", [2, 4])
def test_upsample_uv_jobs_under_both_stops(tq, lj9, lj9full, denom):
    """stop 0: the replacement chroma at 1x1, through the luma's IDCT; stop 1: the original chroma and sampling.  The
    expectation is libjpeg 9's scaled decode of the geometry the stop selects"""
    ims = _uv_batch(lj9full)
    coefs = [_dev(im) for im in ims]
    res = tq.quantsmooth_batch_([dict(coefs=c, quants=im["quants"], **_kw(im)) for c, im in zip(coefs, ims)],
                                pkg.flags_for_quality(6), 2)
    out = tq.decode_batch([dict(coefs=c, **_kw(im)) for c, im in zip(coefs, ims)], result=res, scale_denom=denom)
    stops = res["stop"].cpu().numpy().tolist()                # (read only now, for the expectation)
    assert stops == [0, 1, 1, 0]
    for k, (im, c, r, px) in enumerate(zip(ims, coefs, res["images"], out["images"])):
        host = [t.cpu().numpy() for t in c]
        assert r["coef_up"] is not None
        if stops[k] == 0:
            sel = dict(im, coefs=[host[0]] + [u.cpu().numpy() for u in r["coef_up"]], quants=r["quants"],
                       hsamp=[1, 1, 1], vsamp=[1, 1, 1])
        else:
            sel = dict(im, coefs=host, quants=r["quants"])
        want = lj9.decode(sel, denom)
        assert np.array_equal(px.cpu().numpy(), want), f"job {k} (stop {stops[k]}) at 1/{denom}: " + _diff(px.cpu().numpy(), want)


def test_smooth_and_scaled_decode_in_one_captured_graph(tq, lj9, lj9full):
    """one graph of smoothing plus the decode at mixed reduced sizes, replayed twice on changed coefficients: the replay
    gives libjpeg 9's scaled pixels of what the smoothing left"""
    ims = _uv_batch(lj9full)[:3]
    denoms = [2, 4, 8]
    flags = pkg.flags_for_quality(6)
    src = [_dev(im) for im in ims]
    work = [[t.clone() for t in s] for s in src]
    batch = [dict(coefs=w, quants=im["quants"], **_kw(im)) for w, im in zip(work, ims)]
    ws1, ws2 = None, tq.Workspace()

    def step():
        for w, s in zip(work, src):
            for a, b in zip(w, s):
                a.copy_(b)
        res = tq.quantsmooth_batch_(batch, flags, 2, workspace=ws1)
        return res, tq.decode_batch([dict(coefs=w, **_kw(im)) for w, im in zip(work, ims)], result=res, workspace=ws2,
                                    scale_denom=denoms)

    res, out = step()                                          # eager: prepares both workspaces
    ws1 = res["workspace"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gres, gout = step()
    rng = np.random.default_rng(4)
    for rep in range(2):
        for s, im in zip(src, ims):                            # new inputs: perturbed luma
            base = torch.from_numpy(im["coefs"][0]).cuda()
            noise = torch.from_numpy(rng.integers(-1, 2, im["coefs"][0].shape).astype(np.int16)).cuda()
            s[0].copy_(base + noise * (base != 0).to(torch.int16))
        g.replay()
        torch.cuda.synchronize()
        stops = gres["stop"].cpu().numpy().tolist()
        for k, (im, d, w, r, px) in enumerate(zip(ims, denoms, work, gres["images"], gout["images"])):
            host = [t.cpu().numpy() for t in w]
            if stops[k] == 0:
                sel = dict(im, coefs=[host[0]] + [u.cpu().numpy() for u in r["coef_up"]], quants=r["quants"],
                           hsamp=[1, 1, 1], vsamp=[1, 1, 1])
            else:
                sel = dict(im, coefs=host, quants=r["quants"])
            want = lj9.decode(sel, d)
            assert np.array_equal(px.cpu().numpy(), want), f"replay {rep}, image {k} (stop {stops[k]}) at 1/{d}: " + \
                _diff(px.cpu().numpy(), want)
