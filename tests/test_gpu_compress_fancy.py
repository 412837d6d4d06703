"""The device compress with libjpeg 9's default DCT-scaled chroma downsampling (QS_HIP_DOWNSAMPLE_DCT of
qs_hip_compress_device_batch_info_opts / _prepare_opts, torch_qs.compress(downsampling="dct")) on the GPU, against
libjpeg 9 itself (tests/libjpeg9_compress_fancy.c: jpeg_write_scanlines with JDCT_ISLOW, smoothing_factor 0 and
do_fancy_downsampling TRUE; the arrays read back with jpeg_read_coefficients)."""
import numpy as np
import pytest

import jpegqs_pkg
from compress_fancy_oracle import (FANCY_SIZES, KINDS, LAYOUTS, SHAPES, CompressFancy9, assert_same_arrays, extreme_image,
                                   pixels, tables)
from helpers import Guarded

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A
BY_NAME = {l[0]: l[1:] for l in LAYOUTS}


@pytest.fixture(scope="module")
def c9(tmp_path_factory):
    return CompressFancy9(tmp_path_factory.mktemp("c9f"))


@pytest.fixture(scope="module")
def tq():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible to torch")
    return pkg.torch_qs


def _shapes(size, hs, vs):
    n = len(hs)
    mh, mv = (1, 1) if n == 1 else (max(hs), max(vs))
    return [(-(-size[1] * (1 if n == 1 else vs[ci]) // (8 * mv)), -(-size[0] * (1 if n == 1 else hs[ci]) // (8 * mh)))
            for ci in range(n)]


class AbiImage:
    """one job of a C ABI run in `mode` ("dct", "box" or None = a NULL opts entry): the pixels at a misaligned base
    with an odd row pitch, and the arrays to fill, each between sentinel margins; extra = (rows, columns) of blocks
    beyond libjpeg's geometry"""

    def __init__(self, gpu, k, px, q, hs, vs, cs, mode="dct", extra=(0, 0)):
        h, w, n = px.shape
        self.px, self.q, self.hs, self.vs, self.cs, self.mode = px, q, hs, vs, cs, mode
        self.pitch = w * n + 1 + 2 * (k % 3)                                   # odd, and more than a row
        self.base = 1 + k % 3                                                  # the first pixel's address modulo 4
        self.pix = Guarded(self.base + (h - 1) * self.pitch + w * n)
        rows = np.zeros((h, self.pitch), np.uint8)
        rows[:, :w * n] = px.reshape(h, w * n)
        flat = rows.reshape(-1)[:(h - 1) * self.pitch + w * n]
        self.pix.view[self.base:] = torch.from_numpy(flat.copy()).cuda()
        self.need = _shapes((w, h), hs, vs)
        self.shapes = [(hb + extra[0], wb + extra[1]) for hb, wb in self.need]
        self.arr = [Guarded(hb * wb * 64, torch.int16) for hb, wb in self.shapes]
        for a in self.arr:
            a.view.fill_(SENTINEL)
        self.job = gpu.device_job([a.view.data_ptr() for a in self.arr], self.shapes, q, hsamp=hs, vsamp=vs,
                                  colorspace=cs, image_size=(w, h))

    def want(self, c9):
        f = c9.libjpeg if self.mode == "dct" else c9.libjpeg_box
        return f(self.px, self.q, self.hs, self.vs, self.cs)["coefs"]

    def check(self, c9, what):
        want = self.want(c9)
        for ci, (a, (hb, wb), (nh, nw)) in enumerate(zip(self.arr, self.shapes, self.need)):
            a.check()
            got = a.view.cpu().numpy().reshape(hb, wb, 64)
            assert_same_arrays([got[:nh, :nw]], [want[ci]], f"{what}, component {ci}")
            outside = got.copy()
            outside[:nh, :nw] = SENTINEL
            assert (outside == SENTINEL).all(), f"{what}, component {ci}: a block outside libjpeg's geometry was written"
        self.pix.check()


def _run_abi(gpu, images):
    jobs, opts = [im.job for im in images], [im.mode for im in images]
    per, nbytes = gpu.compress_batch_info(jobs, opts=opts)
    ws = Guarded(nbytes)
    assert ws.view.data_ptr() % 256 == 0
    gpu.compress_batch_prepare(jobs, ws.view.data_ptr(), nbytes, opts=opts)
    gpu.compress_batch(jobs, [im.pix.view.data_ptr() + im.base for im in images], [im.pitch for im in images],
                       ws.view.data_ptr(), nbytes)
    torch.cuda.synchronize()
    ws.check()
    return per


@pytest.mark.parametrize("name", [l[0] for l in LAYOUTS])
def test_grid_through_the_c_abi(gpu, c9, name):
    """every size x table kind of one layout as one batch in the dct mode: odd pitches, misaligned pixel bases,
    guarded buffers; luma and the 1x1 layouts are also the box mode's arrays"""
    hs, vs, cs = BY_NAME[name]
    rng = np.random.default_rng([7, len(name), hs[0], vs[0], cs, 16])
    images = []
    for kind in KINDS:
        for size in FANCY_SIZES:
            images.append((AbiImage(gpu, len(images), pixels(rng, size, len(hs)), tables(kind, len(hs), pkg.synth, rng),
                                    hs, vs, cs), f"{name} {size} {kind}"))
    per = _run_abi(gpu, [im for im, _ in images])
    for (im, what), p in zip(images, per):
        assert list(zip(p["hblk"], p["wblk"])) == im.need
        im.check(c9, what)
        same = len(hs) if hs[0] * vs[0] == 1 or im.px.shape[:2] == (1, 1) else 1
        box = c9.libjpeg_box(im.px, im.q, hs, vs, cs)["coefs"]
        got = [a.view.cpu().numpy().reshape(hb, wb, 64) for a, (hb, wb) in zip(im.arr, im.shapes)]
        assert_same_arrays(got[:same], box[:same], f"{what}: against the box mode")


def test_sizes_around_the_tile(gpu, c9):
    """63, 64, 65 x 15, 16, 17 pixels -- one tile less one, exact, plus one, both ways -- and 33 x 18, 20, 34 (where a
    repeated downsampled row would differ from the plain clamp) in the subsampled layouts and gray: 60 jobs, so the
    batch also crosses a launch chunk"""
    rng = np.random.default_rng(64)
    images = []
    for name in ("gray", "ycc2x1", "ycc1x2", "ycc2x2", "rgb4x1"):
        hs, vs, cs = BY_NAME[name]
        for size in [(w, h) for w in (63, 64, 65) for h in (15, 16, 17)] + [(33, 18), (33, 20), (33, 34)]:
            images.append((AbiImage(gpu, len(images), pixels(rng, size, len(hs)), tables("q50", len(hs), pkg.synth),
                                    hs, vs, cs), f"{name} {size}"))
    _run_abi(gpu, [im for im, _ in images])
    for im, what in images:
        im.check(c9, what)


@pytest.mark.parametrize("shape,name", [("16x16", "rgb2x2"), ("16x8", "rgb2x1"), ("8x16", "rgb1x2"), ("16x8", "rgb4x1")])
def test_extreme_blocks_inside_a_wave(gpu, c9, shape, name):
    """the cosine-sign blocks that reach each pass's L1 norm, tiled into the chroma planes of an RGB-kept image so that
    extreme and plain blocks alternate among the eight a wave transforms together; tables of 1"""
    hs, vs, cs = BY_NAME[name]
    rng = np.random.default_rng([len(shape), hs[0], vs[0]])
    size = (141, 93)
    if name == "rgb4x1":                                   # the h2v1 box runs first: double every column
        half = np.stack([extreme_image(rng, shape, (71, 93)) for _ in range(3)], axis=-1)
        px = np.repeat(half, 2, axis=1)[:, :141]
    else:
        px = np.stack([extreme_image(rng, shape, size) for _ in range(3)], axis=-1)
    im = AbiImage(gpu, 2, np.ascontiguousarray(px), tables("ones", 3, pkg.synth), hs, vs, cs)
    _run_abi(gpu, [im])
    im.check(c9, f"extreme {shape} blocks in {name}")
    assert np.abs(im.want(c9)[1][..., 1:]).max() > 900     # (the bound's region: |w| / 8 up to 946 off the DC)


def test_one_batch_mixes_the_modes(gpu, c9):
    """45 jobs alternating box / dct (every fifth box job through a NULL opts entry), each against its own oracle: the
    mode travels per job, and the batch crosses a launch chunk"""
    rng = np.random.default_rng(45)
    names = [l[0] for l in LAYOUTS if l[1][0] * l[2][0] > 1]
    images = []
    for i in range(pkg.hipqs.COMPRESS_CHUNK + 1):
        hs, vs, cs = BY_NAME[names[(i // 2) % len(names)]]
        size = (int(rng.integers(1, 141)), int(rng.integers(1, 93)))
        mode = "dct" if i & 1 else (None if i % 10 == 0 else "box")
        images.append(AbiImage(gpu, i, pixels(rng, size, 3), tables("q50" if i % 3 else "edge", 3, pkg.synth, rng),
                               hs, vs, cs, mode=mode))
    _run_abi(gpu, images)
    for i, im in enumerate(images):
        im.check(c9, f"job {i} ({im.mode})")
    differ = sum(any((a != b).any() for a, b in zip(c9.libjpeg(im.px, im.q, im.hs, im.vs, im.cs)["coefs"][1:],
                                                    c9.libjpeg_box(im.px, im.q, im.hs, im.vs, im.cs)["coefs"][1:]))
                 for im in images[:8])
    assert differ >= 4                                     # (the two oracles do differ on such jobs)


@pytest.mark.parametrize("name,size", [("ycc2x2", (17, 9)), ("ycc4x1", (70, 50)), ("rgb2x1", (33, 18)), ("rgb1x2", (65, 66))])
def test_wider_arrays_keep_their_other_blocks(gpu, c9, name, size):
    """a caller array larger than libjpeg's geometry: exactly width_in_blocks x height_in_blocks blocks are written, with
    the caller's row stride"""
    hs, vs, cs = BY_NAME[name]
    rng = np.random.default_rng(17)
    im = AbiImage(gpu, 1, pixels(rng, size, len(hs)), tables("q50", len(hs), pkg.synth), hs, vs, cs, extra=(1, 3))
    _run_abi(gpu, [im])
    im.check(c9, f"{name} {size} in wider arrays")


@pytest.mark.parametrize("name,size", [("ycc2x2", (141, 93)), ("ycc4x1", (70, 50))])
def test_compress_then_encode_equals_libjpegs_default_file(tq, c9, name, size):
    """compress(downsampling="dct") -> encode: the whole file libjpeg writes from the pixels with its default
    downsampling"""
    hs, vs, cs = BY_NAME[name]
    rng = np.random.default_rng(93)
    px = pixels(rng, size, len(hs))
    im = tq.compress(torch.from_numpy(px).cuda(), quality=50, hsamp=hs, vsamp=vs, downsampling="dct")
    assert sorted(im) == ["coefs", "colorspace", "hsamp", "image_size", "quants", "vsamp"]
    data = tq.encode(**im)
    q = tables("q50", len(hs), pkg.synth)
    want = c9.libjpeg(px, q, hs, vs, cs, keep_file=True)["file"].read_bytes()
    assert data == want
    box = tq.encode(**tq.compress(torch.from_numpy(px).cuda(), quality=50, hsamp=hs, vsamp=vs))
    assert box != want                                         # (the box mode's file is another one)


def test_compress_smooth_decode_in_one_captured_graph(tq, c9):
    """compress(dct) -> quantsmooth_ -> decode captured in one torch.cuda.graph and replayed on new pixels equals the
    eager run; the eager arrays are libjpeg's"""
    rng = np.random.default_rng(95)
    size, hs, vs = (141, 70), [2, 1, 1], [2, 1, 1]
    px = torch.from_numpy(pixels(rng, size, 3)).cuda()
    flags = pkg.flags_for_quality(3)
    ws = [tq.Workspace(), None, tq.Workspace()]

    def step():
        im = tq.compress(px, quality=40, hsamp=hs, vsamp=vs, downsampling="dct", workspace=ws[0])
        first = [c.clone() for c in im["coefs"]]
        res = tq.quantsmooth_(im["coefs"], im["quants"], flags, 2, hsamp=hs, vsamp=vs, colorspace=3, image_size=size,
                              workspace=ws[1])
        return im, first, res, tq.decode(im["coefs"], hsamp=hs, vsamp=vs, colorspace=3, image_size=size, result=res,
                                         workspace=ws[2])

    im, first, res, _ = step()                                 # eager: prepares the three workspaces
    ws[1] = res["workspace"]
    torch.cuda.synchronize()
    q = [pkg.synth.quality_table(pkg.synth.STD_LUMA if ci == 0 else pkg.synth.STD_CHROMA, 40) for ci in range(3)]
    assert all(np.array_equal(a, b) for a, b in zip(q, im["quants"]))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gim, gfirst, gres, gout = step()
    for rep in range(2):
        host = pixels(rng, size, 3)
        px.copy_(torch.from_numpy(host).cuda())
        g.replay()
        torch.cuda.synchronize()
        got, gstop = gout.cpu().numpy().copy(), int(gres["stop"].item())
        gf = [c.cpu().numpy().copy() for c in gfirst]
        eim, efirst, eres, eout = step()                       # eager on the same pixels
        torch.cuda.synchronize()
        assert gstop == int(eres["stop"].item())
        assert np.array_equal(got, eout.cpu().numpy()), f"replay {rep}"
        assert got.shape == (size[1], size[0], 3)
        for ci, (x, y) in enumerate(zip(gim["coefs"], eim["coefs"])):
            assert torch.equal(x, y), f"replay {rep}, component {ci}"
        assert_same_arrays(gf, c9.libjpeg(host, q, hs, vs, 3)["coefs"], f"replay {rep}: the compress inside the graph")


def test_a_change_of_mode_prepares_the_workspace_again(tq, c9):
    """one Workspace through box, dct, box: each call gives its own mode's arrays, so the mode is part of what the
    workspace is prepared for; a per-image key overrides the call's default; inside a capture a workspace prepared for
    the other mode raises, as one prepared for another geometry does"""
    rng = np.random.default_rng(97)
    size, hs, vs = (70, 50), [2, 1, 1], [2, 1, 1]
    host = pixels(rng, size, 3)
    px = torch.from_numpy(host).cuda()
    q = tables("q50", 3, pkg.synth)
    want = dict(dct=c9.libjpeg(host, q, hs, vs, 3)["coefs"], box=c9.libjpeg_box(host, q, hs, vs, 3)["coefs"])
    ws = tq.Workspace()
    keys = []
    for mode in ("box", "dct", "box", "dct"):
        im = tq.compress(px, quants=q, hsamp=hs, vsamp=vs, downsampling=mode, workspace=ws)
        assert_same_arrays([c.cpu().numpy() for c in im["coefs"]], want[mode], f"{mode} on the shared workspace")
        keys.append(ws.key)
    assert keys[0] == keys[2] != keys[1] == keys[3]
    same = tq.compress(px, quants=q, hsamp=hs, vsamp=vs, downsampling="dct", workspace=ws)
    assert ws.key == keys[3]
    assert_same_arrays([c.cpu().numpy() for c in same["coefs"]], want["dct"], "dct again, no prepare")
    # the per-image key wins over the call's default; one batch, both modes
    one = dict(pixels=px, quants=q, hsamp=hs, vsamp=vs)
    r = tq.compress_batch([dict(one, downsampling="box"), one, dict(one, downsampling="dct")], downsampling="dct")
    for k, mode in enumerate(("box", "dct", "dct")):
        assert_same_arrays([c.cpu().numpy() for c in r["images"][k]["coefs"]], want[mode], f"batch image {k}")
    # inside a capture
    box_ws = tq.compress_batch([one], downsampling="box")["workspace"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="capture"):
        with torch.cuda.graph(g):
            kept = px + 0                                      # (the capture is not empty)
            tq.compress(px, quants=q, hsamp=hs, vsamp=vs, downsampling="dct", workspace=box_ws)
    torch.cuda.synchronize()
    del kept
    after = tq.compress(px, quants=q, hsamp=hs, vsamp=vs, downsampling="box", workspace=box_ws)
    assert_same_arrays([c.cpu().numpy() for c in after["coefs"]], want["box"], "the box workspace after the refusal")


def test_refusals_write_nothing(gpu, tq):
    """QS_HIP_EINVAL from the _opts calls for an unknown mode and non-zero reserved fields, QS_HIP_ENOTSUP for `fancy`
    as before; nothing is written"""
    rng = np.random.default_rng(96)
    px = pixels(rng, (48, 16), 3)
    q = tables("q50", 3, pkg.synth)
    ok = AbiImage(gpu, 0, px, q, [2, 1, 1], [2, 1, 1], 3)
    nbytes = gpu.compress_batch_info([ok.job], opts=["dct"])[1]
    ws = Guarded(nbytes)
    bad = pkg.hipqs.CompressOpts()
    bad.downsampling, bad.reserved[2] = 1, 5
    for call, code in ((lambda: gpu.compress_batch_prepare([ok.job], ws.view.data_ptr(), nbytes, opts=[2]), -2),
                       (lambda: gpu.compress_batch_prepare([ok.job], ws.view.data_ptr(), nbytes, opts=[bad]), -2),
                       (lambda: gpu.compress_batch_prepare([ok.job], ws.view.data_ptr(), nbytes, fancy=True), -4),
                       (lambda: gpu.compress_batch_prepare([ok.job], ws.view.data_ptr(), nbytes, fancy=True, opts=["dct"]), -4)):
        with pytest.raises(pkg.hipqs.QsHipError) as e:
            call()
        assert e.value.code == code
    torch.cuda.synchronize()
    ws.check()
    assert bool((ws.view == 0xA5).all())
    for a in ok.arr:
        a.check()
        assert bool((a.view == SENTINEL).all())
    dev = torch.from_numpy(px).cuda()
    with pytest.raises(ValueError, match="downsampling"):
        tq.compress(dev, quality=50, downsampling="fancy")
    with pytest.raises(ValueError, match="fancy"):
        tq.compress(dev, quality=50, fancy=True, downsampling="dct")
