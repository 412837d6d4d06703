"""The device decode to pixels (torch_qs.decode / decode_batch, qs_hip_decode_device_batch) on the GPU, against libjpeg 9
itself (tests/libjpeg9_decode.c) and the reference's recorded decode-mode pixels."""
import numpy as np
import pytest

import jpegqs_pkg
from decode_oracle import GOLD, LibJpeg9, synth_image

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
FLAGS = pkg.hipqs.FLAGS


@pytest.fixture(scope="module")
def lj9(tmp_path_factory):
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


def _smooth_and_decode(tq, im, flags, niter):
    coefs = _dev(im)
    res = tq.quantsmooth_(coefs, im["quants"], flags, niter, **_kw(im))
    px = tq.decode(coefs, **_kw(im), result=res)
    return px.cpu().numpy(), res, coefs


DEC_REF = [("gray64", 4, 2), ("rgb141x93_420", 3, 3), ("rgb128x96_420", 3, 2), ("rgb128x96_420", 5, 2),
           ("rgb141x93_444", 6, 3), ("gray64", 6, 2), ("rgb141x93_444", 5, 2)]


@pytest.mark.parametrize("src,quality,niter", DEC_REF)
def test_smooth_then_decode_equals_the_reference_decode_mode(tq, lj9, src, quality, niter):
    im = lj9.read(GOLD / f"{src}.jpg")
    px, res, _ = _smooth_and_decode(tq, im, pkg.flags_for_quality(quality), niter)
    assert int(res["stop"].item()) == 0
    assert px.tobytes() == (GOLD / f"{src}.q{quality}.dec.ref.raw").read_bytes()


# CLI goldens (-q Q -n 3): libjpeg 9's decode of the reference CLI's output file is the truth.  For UPSAMPLE_UV on 4:2:0
# that file is the 1x1-sampled JPEG holding the smoothed arrays, which libjpeg 9 decodes where the decode mode cannot.
@pytest.mark.parametrize("src,quality", [("rgb141x93_420", 6), ("rgb141x93_420", 4), ("rgb120x88_422_rst", 5),
                                         ("rgb120x88_422_rst", 6), ("rgb120x88_422_rst", 2), ("gray64", 3)])
def test_smooth_then_decode_equals_libjpeg_on_the_reference_cli_output(tq, lj9, src, quality):
    im = lj9.read(GOLD / f"{src}.jpg")
    px, res, _ = _smooth_and_decode(tq, im, pkg.flags_for_quality(quality), 3)
    ref = lj9.read(GOLD / f"{src}.q{quality}.ref.jpg")
    want = lj9.decode(ref["coefs"], ref["quants"], ref["hsamp"], ref["vsamp"], ref["colorspace"], ref["image_size"])
    assert px.shape == want.shape and np.array_equal(px, want)


LAYOUTS = [([1], [1], 1), ([2], [2], 1), ([1, 1, 1], [1, 1, 1], 3), ([2, 1, 1], [1, 1, 1], 3), ([1, 1, 1], [2, 1, 1], 3),
           ([2, 1, 1], [2, 1, 1], 3), ([4, 1, 1], [1, 1, 1], 3), ([1, 1, 1], [1, 1, 1], 2), ([2, 1, 1], [2, 1, 1], 2),
           ([4, 1, 1], [1, 1, 1], 2)]


@pytest.mark.parametrize("size", [(8, 8), (141, 93), (67, 131), (200, 17)])
def test_every_layout_against_libjpeg(tq, lj9, size):
    """seeded in-range arrays and random tables, no smoothing, every supported layout in one batch, sizes that are not
    MCU multiples"""
    rng = np.random.default_rng(size[0] * 1000 + size[1])
    ims = [synth_image(rng, size, hs, vs, cs) for hs, vs, cs in LAYOUTS]
    r = tq.decode_batch([dict(coefs=_dev(im), quants=im["quants"], **_kw(im)) for im in ims])
    for k, (im, px) in enumerate(zip(ims, r["images"])):
        want = lj9.decode(im["coefs"], im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"])
        assert np.array_equal(px.cpu().numpy(), want), f"layout {LAYOUTS[k]} at {size}"


def test_extreme_coefficients_and_tables_against_the_libjpeg_idcts(tq, lj9):
    """blocks of +-32767 / -32768 with tables up to 65535 (and 0): pass 1 products beyond int32.  RGB images without
    colour conversion put every IDCT's samples straight into the output: luma through jpeg_idct_islow, chroma through
    jpeg_idct_16x16 / _16x8 / _8x16 (4:1:1: _16x8 and 2x replication), compared with those functions of libjpeg 9"""
    rng = np.random.default_rng(99)
    tables = [np.full(64, 65535, np.uint16), np.zeros(64, np.uint16), rng.integers(0, 65536, 64).astype(np.uint16),
              rng.choice(np.array([1, 255, 65535, 32768], np.uint16), 64)]
    kinds = {(1, 1): "islow", (2, 2): "16x16", (2, 1): "16x8", (1, 2): "8x16", (4, 1): "16x8"}
    images, want = [], []
    for (hs, vs), kind in kinds.items():
        for t in range(len(tables)):
            size = (8 * hs * 3 - 3, 8 * vs * 2 - 1)
            coefs, quants, exp = [], [], []
            for ci in range(3):
                cw, ch = (8 * hs, 8 * vs) if ci else (8, 8)
                nby, nbx = -(-size[1] // ch), -(-size[0] // cw)
                blk = rng.integers(-32768, 32768, (nby * nbx, 64)).astype(np.int16)
                ext = rng.random((nby * nbx, 64)) < 0.7
                blk[ext] = rng.choice(np.array([32767, -32768], np.int16), int(ext.sum()))
                q = tables[(t + ci) % len(tables)]
                coefs.append(blk.reshape(nby, nbx, 64))
                quants.append(q)
                k = kind if ci else "islow"
                out = lj9.blocks(k, blk, np.broadcast_to(q, blk.shape))
                if ci and (hs, vs) == (4, 1):
                    out = np.repeat(out, 2, axis=2)
                r, c = out.shape[1:]
                plane = out.reshape(nby, nbx, r, c).transpose(0, 2, 1, 3).reshape(nby * r, nbx * c)
                exp.append(plane[:size[1], :size[0]])
            images.append(dict(coefs=[torch.from_numpy(c).cuda() for c in coefs], quants=quants,
                               hsamp=[hs, 1, 1], vsamp=[vs, 1, 1], colorspace=2, image_size=size))
            want.append(np.stack(exp, axis=2))
    r = tq.decode_batch(images)
    for k, (px, w) in enumerate(zip(r["images"], want)):
        assert np.array_equal(px.cpu().numpy(), w), f"image {k}"


def _stop_batch(lj9):
    """UPSAMPLE_UV jobs on 4:2:0 and 4:2:2 goldens, one of each with a planted range-check trip in its last component
    (a DC of 1000 against a table entry >= 3), between a grayscale and a 4:4:4 job"""
    ims = []
    for src in ("gray64", "rgb141x93_420", "rgb128x96_420", "rgb141x93_444", "rgb120x88_422_rst", "rgb141x93_420"):
        ims.append(lj9.read(GOLD / f"{src}.jpg"))
    for k in (2, 4, 5):
        im = ims[k]
        im["quants"][2] = im["quants"][2].copy()
        im["quants"][2][0] = max(int(im["quants"][2][0]), 3)
        im["coefs"][2] = im["coefs"][2].copy()
        im["coefs"][2][0, 0, 0] = 1000
    return ims


def _expected(lj9, im, coefs, res, stop):
    """libjpeg 9's decode of what the smoothing left: the replacement chroma at 1x1 when it stood, else the original"""
    q = res["quants"]
    host = [c.cpu().numpy() for c in coefs]
    if res["coef_up"] is not None and stop == 0:
        up = [u.cpu().numpy() for u in res["coef_up"]]
        return lj9.decode([host[0]] + up, q, [1, 1, 1], [1, 1, 1], im["colorspace"], im["image_size"])
    return lj9.decode(host, q, im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"])


def test_stops_pick_the_geometry_on_the_device(tq, lj9):
    ims = _stop_batch(lj9)
    coefs = [_dev(im) for im in ims]
    flags = pkg.flags_for_quality(6)
    res = tq.quantsmooth_batch_([dict(coefs=c, quants=im["quants"], **_kw(im)) for c, im in zip(coefs, ims)], flags, 2)
    out = tq.decode_batch([dict(coefs=c, **_kw(im)) for c, im in zip(coefs, ims)], result=res)
    stops = res["stop"].cpu().numpy().tolist()                # (read only now, for the expectation)
    assert stops == [0, 0, 1, 0, 1, 1]
    assert res["images"][2]["coef_up"] is not None and res["images"][1]["coef_up"] is not None
    for k, (im, c, r, px) in enumerate(zip(ims, coefs, res["images"], out["images"])):
        assert np.array_equal(px.cpu().numpy(), _expected(lj9, im, c, r, stops[k])), f"job {k} (stop {stops[k]})"


def test_smooth_and_decode_in_one_captured_graph(tq, lj9):
    ims = _stop_batch(lj9)[1:4]
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
        return res, tq.decode_batch([dict(coefs=w, **_kw(im)) for w, im in zip(work, ims)], result=res, workspace=ws2)

    res, out = step()                                          # eager: prepares both workspaces
    ws1 = res["workspace"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gres, gout = step()
    rng = np.random.default_rng(3)
    for rep in range(3):
        for s, im in zip(src, ims):                            # new inputs: perturbed luma, a trip in one of them
            base = torch.from_numpy(im["coefs"][0]).cuda()
            noise = torch.from_numpy(rng.integers(-1, 2, im["coefs"][0].shape).astype(np.int16)).cuda()
            s[0].copy_(base + noise * (base != 0).to(torch.int16))
        src[rep % 3][2].view(-1)[0] = 1000 if rep == 1 else int(ims[rep % 3]["coefs"][2].reshape(-1)[0])
        g.replay()
        torch.cuda.synchronize()
        got = [p.cpu().numpy().copy() for p in gout["images"]]
        gstop = gres["stop"].cpu().numpy().tolist()
        eres, eout = step()                                    # eager on the same inputs
        torch.cuda.synchronize()
        assert eres["stop"].cpu().numpy().tolist() == gstop
        for k, (a, b) in enumerate(zip(got, eout["images"])):
            assert np.array_equal(a, b.cpu().numpy()), f"replay {rep}, image {k}"


def test_large_420_image_against_libjpeg(tq, lj9):
    rng = np.random.default_rng(8192)
    im = synth_image(rng, (8192, 8192), [2, 1, 1], [2, 1, 1], 3, amp=30)
    px = tq.decode(_dev(im), im["quants"], **_kw(im))
    want = lj9.decode(im["coefs"], im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"])
    assert np.array_equal(px.cpu().numpy(), want)


def test_output_pitch_and_sentinels(tq, lj9):
    rng = np.random.default_rng(17)
    im = synth_image(rng, (45, 29), [2, 1, 1], [1, 1, 1], 3)
    h, w = 29, 45
    pitch, margin = 160, 4096
    buf = torch.full((2 * margin + h * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
    view = buf[margin:margin + h * pitch].view(h, pitch)[:, :w * 3].view(h, w, 3)
    px = tq.decode(_dev(im), im["quants"], **_kw(im), out=view)
    assert px.data_ptr() == view.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:margin] == 0xA5).all() and (host[margin + h * pitch:] == 0xA5).all()
    rows = host[margin:margin + h * pitch].reshape(h, pitch)
    assert (rows[:, w * 3:] == 0xA5).all()
    want = lj9.decode(im["coefs"], im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"])
    assert np.array_equal(rows[:, :w * 3].reshape(h, w, 3), want)


def test_unsupported_input_writes_nothing(tq):
    rng = np.random.default_rng(18)
    ok = synth_image(rng, (32, 16), [1], [1], 1)
    cmyk = synth_image(rng, (32, 16), [1, 1, 1, 1], [1, 1, 1, 1], 4)
    outs = [torch.full((16, 32, 1), 0x5A, dtype=torch.uint8, device="cuda"),
            torch.full((16, 32, 3), 0x5A, dtype=torch.uint8, device="cuda")]
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        tq.decode_batch([dict(coefs=_dev(ok), quants=ok["quants"], **_kw(ok)),
                         dict(coefs=_dev(cmyk), quants=cmyk["quants"], **_kw(cmyk))], outs=outs)
    assert e.value.code == -4
    torch.cuda.synchronize()
    assert all(bool((o == 0x5A).all()) for o in outs)
