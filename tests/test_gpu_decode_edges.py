"""The device decode (torch_qs.decode_batch, qs_hip_decode_device_batch) at the decisions tests/test_gpu_decode.py leaves
alone: the 32-bit / 64-bit split of pass 1 at its bound, more than one launch chunk (and a stop word read in the second),
block arrays wider than the image needs, sizes around the 64 x 16 output tile, every (Cb, Cr) pair, and misaligned
outputs with odd pitches.  Everything is compared with libjpeg 9 for exact equality (tests/libjpeg9_decode.c), and every
output buffer sits between sentinel margins.  The cases come from tests/decode_cases.py (checked on the CPU by
tests/test_decode_cases.py)."""
import numpy as np
import pytest

import decode_cases as dc
import jpegqs_pkg
from decode_oracle import GOLD, LibJpeg9, synth_image
from helpers import MARGIN, Guarded

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


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


def _want(lj9, im):
    return lj9.decode(im["coefs"], im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"])


def _decode(tq, ims, devs=None, result=None):
    """decode_batch with every output between sentinel margins -> (host pixels per image, what decode_batch returned)"""
    devs = [_dev(im) for im in ims] if devs is None else devs
    shapes = [(im["image_size"][1], im["image_size"][0], 1 if len(im["coefs"]) == 1 else 3) for im in ims]
    guards = [Guarded(h * w * c) for h, w, c in shapes]
    batch = [dict(coefs=d, **_kw(im)) if result is not None else dict(coefs=d, quants=im["quants"], **_kw(im))
             for d, im in zip(devs, ims)]
    r = tq.decode_batch(batch, result=result, outs=[g.view.view(s) for g, s in zip(guards, shapes)])
    torch.cuda.synchronize()
    for k, g in enumerate(guards):
        try:
            g.check()
        except AssertionError as e:
            raise AssertionError(f"image {k}: {e}") from None
    return [g.view.cpu().numpy().reshape(s) for g, s in zip(guards, shapes)], r


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    y, x, c = bad[0]
    return f"{len(bad)} samples differ, first at (y, x, channel) = ({y}, {x}, {c}): {got[y, x, c]} != libjpeg {want[y, x, c]}"


# ---- 1. the pass-1 bound --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hs,vs", list(dc.KIND_OF))
def test_pass1_bound_against_the_libjpeg_idcts(tq, lj9, hs, vs):
    """RGB images (no colour transform: every IDCT's samples go straight out) of sign-aligned blocks on both sides of
    QS_DEC_FAST_BOUND, fast and slow blocks side by side in every wave: luma through jpeg_idct_islow, chroma through the
    sampling's scaled IDCT.  One image per quant table (a component has one table: 1, 2, 3 and the 35081 column)."""
    ims = dc.bound_images(hs, vs)
    got, _ = _decode(tq, ims)
    for im, px in zip(ims, got):
        want = dc.bound_expected(lj9, im)
        assert px.shape == want.shape
        assert np.array_equal(px, want), f"sampling {hs}x{vs}, table max {int(im['quants'][0].max())}: " + \
            dc.bound_blame(im, px, want)


# ---- 2. launch chunks -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [44, 45, 91])
def test_batches_across_launch_chunks(tq, lj9, tmp_path, n):
    assert dc.header_constant("QS_DEC_CHUNK") == 44        # (the sizes above: one full chunk, one more, two and three)
    ims = dc.chunk_batch(n)
    got, r = _decode(tq, ims)
    for k, (im, px) in enumerate(zip(ims, got)):
        want = _want(lj9, im)
        assert np.array_equal(px, want), f"job {k} of {n} ({im['image_size']}, {im['hsamp']}x{im['vsamp']}): " + \
            _first_diff(px, want)
    if n == 91:
        # the prepared descriptors: each job's first workgroup counts from the start of its own chunk's launch
        info = dc.DecodeHost(tmp_path).info()
        size, chunk = info["job_size"], info["chunk"]
        rec = r["workspace"].buf[:n * size].cpu().numpy().reshape(n, size)
        field = lambda name: np.ascontiguousarray(rec[:, info[name]:info[name] + 4]).view(np.int32).reshape(-1)
        tiles = [dc.tile_count(im["image_size"]) for im in ims]
        assert field("job_tiles").tolist() == tiles
        assert field("job_tile0").tolist() == [sum(tiles[k - k % chunk:k]) for k in range(n)]


def test_stop_words_of_the_second_chunk(tq, lj9):
    """52 UPSAMPLE_UV jobs from the 4:2:0 / 4:2:2 goldens; job k + 44 is job k's image with the opposite outcome of the
    range check, so a job of the second chunk that read a first-chunk stop word would decode the wrong geometry"""
    from test_gpu_decode import _expected, _stop_batch
    planted = _stop_batch(lj9)                              # [1] a clean 4:2:0 job; [5], [2], [4] with the planted trip
    clean = [planted[1]] + [lj9.read(GOLD / f"{s}.jpg") for s in ("rgb128x96_420", "rgb120x88_422_rst")]
    tripped = [planted[5], planted[2], planted[4]]
    for a, b in zip(clean, tripped):                       # the same image but for the plant
        assert a["image_size"] == b["image_size"] and a["hsamp"] == b["hsamp"] and a["vsamp"] == b["vsamp"]
        assert np.array_equal(a["coefs"][0], b["coefs"][0]) and int(b["coefs"][2][0, 0, 0]) == 1000 != int(a["coefs"][2][0, 0, 0])
    pool = [(im, 0) for im in clean] + [(im, 1) for im in tripped]
    chunk = dc.header_constant("QS_DEC_CHUNK")
    picks = [(5 * k + k // 6) % 6 for k in range(chunk)]
    picks += [(p + 3) % 6 for p in picks[:8]]              # k + 44: the same image, the other outcome
    ims, want_stop = [pool[p][0] for p in picks], [pool[p][1] for p in picks]
    assert len(ims) >= 50
    for side in (want_stop[:chunk], want_stop[chunk:]):
        assert 0 in side and 1 in side
    for k in range(8):
        assert ims[k]["image_size"] == ims[k + chunk]["image_size"] and want_stop[k] != want_stop[k + chunk]
    devs = [_dev(im) for im in ims]
    res = tq.quantsmooth_batch_([dict(coefs=d, quants=im["quants"], **_kw(im)) for d, im in zip(devs, ims)],
                                pkg.flags_for_quality(6), 2)
    got, _ = _decode(tq, ims, devs=devs, result=res)
    stops = res["stop"].cpu().numpy().tolist()
    assert stops == want_stop
    assert all(r["coef_up"] is not None for r, p in zip(res["images"], picks) if p % 3 != 2)     # (the 4:2:0 jobs)
    for k, (im, d, r, px) in enumerate(zip(ims, devs, res["images"], got)):
        want = _expected(lj9, im, d, r, stops[k])
        assert np.array_equal(px, want), f"job {k} (stop {stops[k]}): " + _first_diff(px, want)


# ---- 3. array stride ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(141, 93), (67, 131)])
def test_arrays_larger_than_the_image_needs(tq, lj9, size):
    """every layout with its arrays padded to whole MCUs and by +3 block columns / +2 block rows of +-32767: libjpeg's
    decode of the unpadded arrays, so no sample may come from a poisoned block or from the wrong row stride"""
    rng = np.random.default_rng(size[0] * 7 + size[1])
    base = [synth_image(rng, size, hs, vs, cs) for hs, vs, cs in dc.layouts()]
    want = [_want(lj9, im) for im in base]
    ims, names = [], []
    for im in base:
        ew, eh = zip(*dc.mcu_extra(im))
        ims += [dc.padded(im, ew, eh), dc.padded(im, 3, 2)]
        names += [f"MCU padding {ew} x {eh}", "+3 columns, +2 rows"]
    assert any(a.shape != b.shape for im, p in zip(base, ims[0::2]) for a, b in zip(im["coefs"], p["coefs"]))
    got, _ = _decode(tq, ims)
    for k, px in enumerate(got):
        im = ims[k]
        assert np.array_equal(px, want[k // 2]), \
            f"{im['hsamp']}x{im['vsamp']} colour space {im['colorspace']} at {size}, {names[k]}: " + _first_diff(px, want[k // 2])


# ---- 4. tile edges --------------------------------------------------------------------------------------------------

def test_sizes_around_the_output_tile(tq, lj9):
    ims = dc.edge_sizes()
    got, _ = _decode(tq, ims)
    for im, px in zip(ims, got):
        want = _want(lj9, im)
        assert px.shape == want.shape
        assert np.array_equal(px, want), \
            f"{im['hsamp']}x{im['vsamp']} colour space {im['colorspace']} at {im['image_size']}: " + _first_diff(px, want)


# ---- 5. colour conversion -------------------------------------------------------------------------------------------

def _colour_blame(im, px, want):
    y, x, c = np.argwhere(px != want)[0]
    ph, pw = 8 * im["vsamp"][0], 8 * im["hsamp"][0]
    ycc = [int(im["coefs"][0][y // 8, x // 8, 0]) + 128] + [int(im["coefs"][ci][y // ph, x // pw, 0]) + 128 for ci in (1, 2)]
    return f"(Y, Cb, Cr) blocks {ycc} at ({y}, {x}): {px[y, x].tolist()} != libjpeg {want[y, x].tolist()}"


def test_every_chroma_pair_444(tq, lj9):
    ims = [dc.colour_grid(y) for y in dc.GRID_Y]
    got, _ = _decode(tq, ims)
    for y, im, px in zip(dc.GRID_Y, ims, got):
        want = _want(lj9, im)
        assert np.array_equal(px, want), f"Y {y}: " + _colour_blame(im, px, want)


def test_every_chroma_pair_420(tq, lj9):
    im = dc.colour_grid_420()
    (px,), _ = _decode(tq, [im])
    want = _want(lj9, im)
    assert np.array_equal(px, want), _colour_blame(im, px, want)


# ---- 6. output addressing -------------------------------------------------------------------------------------------

def test_misaligned_outputs_and_odd_pitches(tq, lj9):
    rng = np.random.default_rng(61)
    cases = [((67, 19), [1], [1], 1), ((65, 17), [1, 1, 1], [1, 1, 1], 3), ((70, 33), [2, 1, 1], [2, 1, 1], 3),
             ((97, 18), [4, 1, 1], [1, 1, 1], 3)]
    ims = [synth_image(rng, *c) for c in cases]
    chans = [1, 3, 3, 3]
    offs = [1, 2, 3, 0]
    pitches = [im["image_size"][0] * c + extra for im, c, extra in zip(ims, chans, (0, 1, 61))] + [4096]
    guards, views = [], []
    for im, c, off, pitch in zip(ims, chans, offs, pitches):
        w, h = im["image_size"]
        g = Guarded(off + h * pitch)
        guards.append(g)
        views.append(g.view[off:off + h * pitch].view(h, pitch)[:, :w * c].view(h, w, c))
        assert views[-1].data_ptr() % 4 == off and views[-1].stride(0) == pitch
    r = tq.decode_batch([dict(coefs=_dev(im), quants=im["quants"], **_kw(im)) for im in ims], outs=views)
    torch.cuda.synchronize()
    for k, (im, c, off, pitch, g, v) in enumerate(zip(ims, chans, offs, pitches, guards, views)):
        assert r["images"][k].data_ptr() == v.data_ptr()
        g.check()
        w, h = im["image_size"]
        host = g.raw.cpu().numpy()[MARGIN:len(g.raw) - MARGIN]
        assert (host[:off] == 0xA5).all(), f"job {k}: bytes before the misaligned base changed"
        rows = host[off:].reshape(h, pitch)
        assert (rows[:, w * c:] == 0xA5).all(), f"job {k}: a row gap changed"
        want = _want(lj9, im)
        px = rows[:, :w * c].reshape(h, w, c)
        assert np.array_equal(px, want), f"job {k} (base + {off}, pitch {pitch}): " + _first_diff(px, want)
