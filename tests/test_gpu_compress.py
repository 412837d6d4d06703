"""The device compress (torch_qs.compress / compress_batch, qs_hip_compress_device_batch) on the GPU, against libjpeg 9
itself (tests/libjpeg9_compress.c: jpeg_write_scanlines with JDCT_ISLOW, smoothing_factor 0, do_fancy_downsampling
FALSE; the arrays read back with jpeg_read_coefficients)."""
import numpy as np
import pytest

import jpegqs_pkg
from compress_oracle import LAYOUTS, SIZES, Compress9, all_colours, assert_same_arrays, pixels, tables
from encode_oracle import parse_jpeg
from helpers import Guarded

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A
BY_NAME = {l[0]: l[1:] for l in LAYOUTS}


@pytest.fixture(scope="module")
def c9(tmp_path_factory):
    return Compress9(tmp_path_factory.mktemp("c9"))


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
    """one job of a C ABI run: the pixels at a misaligned base with an odd row pitch, and the arrays to fill, each
    between sentinel margins; extra = (rows, columns) of blocks beyond libjpeg's geometry"""

    def __init__(self, gpu, k, px, q, hs, vs, cs, extra=(0, 0)):
        h, w, n = px.shape
        self.px, self.q, self.hs, self.vs, self.cs = px, q, hs, vs, cs
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

    def check(self, c9, what):
        want = c9.libjpeg(self.px, self.q, self.hs, self.vs, self.cs)["coefs"]
        for ci, (a, (hb, wb), (nh, nw)) in enumerate(zip(self.arr, self.shapes, self.need)):
            a.check()
            got = a.view.cpu().numpy().reshape(hb, wb, 64)
            assert_same_arrays([got[:nh, :nw]], [want[ci]], f"{what}, component {ci}")
            outside = got.copy()
            outside[:nh, :nw] = SENTINEL
            assert (outside == SENTINEL).all(), f"{what}, component {ci}: a block outside libjpeg's geometry was written"
        self.pix.check()


def _run_abi(gpu, images):
    jobs = [im.job for im in images]
    per, nbytes = gpu.compress_batch_info(jobs)
    ws = Guarded(nbytes)
    assert ws.view.data_ptr() % 256 == 0
    gpu.compress_batch_prepare(jobs, ws.view.data_ptr(), nbytes)
    gpu.compress_batch(jobs, [im.pix.view.data_ptr() + im.base for im in images], [im.pitch for im in images],
                       ws.view.data_ptr(), nbytes)
    torch.cuda.synchronize()
    ws.check()
    return per


@pytest.mark.parametrize("name", [l[0] for l in LAYOUTS])
def test_grid_through_the_c_abi(gpu, c9, name):
    """every size x table kind of one layout as one batch: odd pitches, misaligned pixel bases, guarded buffers"""
    hs, vs, cs = BY_NAME[name]
    rng = np.random.default_rng([7, len(name), hs[0], vs[0], cs])
    images = []
    for kind in ("ones", "q50", "edge"):
        for size in SIZES:
            images.append((AbiImage(gpu, len(images), pixels(rng, size, len(hs)), tables(kind, len(hs), pkg.synth, rng),
                                    hs, vs, cs), f"{name} {size} {kind}"))
    per = _run_abi(gpu, [im for im, _ in images])
    for (im, what), p in zip(images, per):
        assert list(zip(p["hblk"], p["wblk"])) == im.need
        im.check(c9, what)


def test_sizes_around_the_tile(gpu, c9):
    """63, 64, 65 x 15, 16, 17 pixels -- one tile less one, exact, plus one, both ways -- in six layouts: 54 jobs, so the
    batch also crosses a launch chunk"""
    rng = np.random.default_rng(64)
    images = []
    for name in ("gray", "ycc1x1", "ycc2x1", "ycc1x2", "ycc2x2", "rgb4x1"):
        hs, vs, cs = BY_NAME[name]
        for w in (63, 64, 65):
            for h in (15, 16, 17):
                images.append((AbiImage(gpu, len(images), pixels(rng, (w, h), len(hs)), tables("q50", len(hs), pkg.synth),
                                        hs, vs, cs), f"{name} {w}x{h}"))
    _run_abi(gpu, [im for im, _ in images])
    for im, what in images:
        im.check(c9, what)


def test_aligned_rows_take_the_dword_loads(gpu, c9, tq):
    """a contiguous tensor wider than one tile: rows that start 4-byte aligned (the dword path) next to the edge tile"""
    rng = np.random.default_rng(65)
    for name, size in (("ycc2x2", (200, 40)), ("gray", (136, 33)), ("rgb1x1", (128, 16))):
        hs, vs, cs = BY_NAME[name]
        px = pixels(rng, size, len(hs))
        q = tables("q50", len(hs), pkg.synth)
        im = tq.compress(torch.from_numpy(px).cuda(), quants=q, hsamp=hs, vsamp=vs, colorspace=cs)
        want = c9.libjpeg(px, q, hs, vs, cs)
        assert_same_arrays([c.cpu().numpy() for c in im["coefs"]], want["coefs"], f"{name} {size}")
        assert im["image_size"] == size and im["hsamp"] == hs and im["vsamp"] == vs and im["colorspace"] == cs


def test_all_colours(tq, c9):
    """4096 x 4096 4:4:4 holding each of the 2^24 RGB colours once, tables of 1"""
    px = all_colours()
    q = tables("ones", 3, pkg.synth)
    im = tq.compress(torch.from_numpy(px).cuda(), quants=q)
    want = c9.libjpeg(px, q, [1, 1, 1], [1, 1, 1], 3)
    assert_same_arrays([c.cpu().numpy() for c in im["coefs"]], want["coefs"], "all colours")


@pytest.mark.parametrize("njobs", [pkg.hipqs.COMPRESS_CHUNK + 1, 2 * pkg.hipqs.COMPRESS_CHUNK + 3])
def test_batches_beyond_a_launch_chunk(gpu, c9, njobs):
    """one job more than a launch chunk, and two chunks plus three: job i carries image i mod 13 (13 and the chunk of 44
    have no common factor, so a job that landed on another chunk's descriptor or addresses shows)"""
    rng = np.random.default_rng(44)
    names = [l[0] for l in LAYOUTS]
    protos = []
    for k in range(13):
        hs, vs, cs = BY_NAME[names[k % len(names)]]
        size = (int(rng.integers(1, 150)), int(rng.integers(1, 40)))
        protos.append((pixels(rng, size, len(hs)), tables("q50" if k % 2 else "edge", len(hs), pkg.synth, rng), hs, vs, cs))
    images = [AbiImage(gpu, i, *protos[i % 13]) for i in range(njobs)]
    _run_abi(gpu, images)
    want = [c9.libjpeg(*p)["coefs"] for p in protos]
    for i, im in enumerate(images):
        got = [a.view.cpu().numpy().reshape(hb, wb, 64) for a, (hb, wb) in zip(im.arr, im.shapes)]
        assert_same_arrays(got, want[i % 13], f"job {i} of {njobs}")
        for a in im.arr:
            a.check()


@pytest.mark.parametrize("name,size", [("ycc2x2", (17, 9)), ("ycc4x1", (70, 50)), ("gray", (33, 18)), ("rgb1x2", (65, 66))])
def test_wider_arrays_keep_their_other_blocks(gpu, c9, name, size):
    """a caller array larger than libjpeg's geometry (room for the MCUs' dummy blocks and more): exactly
    width_in_blocks x height_in_blocks blocks are written, with the caller's row stride"""
    hs, vs, cs = BY_NAME[name]
    rng = np.random.default_rng(17)
    im = AbiImage(gpu, 1, pixels(rng, size, len(hs)), tables("q50", len(hs), pkg.synth), hs, vs, cs, extra=(1, 3))
    _run_abi(gpu, [im])
    im.check(c9, f"{name} {size} in wider arrays")


@pytest.mark.parametrize("name,size", [("ycc2x2", (141, 93)), ("gray", (77, 45))])
def test_compress_then_encode_equals_libjpegs_file(tq, c9, name, size):
    """compress -> encode: the scan bytes and the parsed header fields of the file libjpeg writes from the pixels"""
    hs, vs, cs = BY_NAME[name]
    rng = np.random.default_rng(93)
    px = pixels(rng, size, len(hs))
    im = tq.compress(torch.from_numpy(px).cuda(), quality=50, hsamp=hs, vsamp=vs)
    data = tq.encode(**im)
    q = tables("q50", len(hs), pkg.synth)
    want = c9.libjpeg(px, q, hs, vs, cs, keep_file=True)["file"].read_bytes()
    assert data == want                                        # (tables below 256: the whole file is libjpeg's)
    a, b = parse_jpeg(data), parse_jpeg(want)
    assert a["segment"] == b["segment"] and a["tail"] == b["tail"]
    pa, pb = pkg.jpeg_file.parse(data), pkg.jpeg_file.parse(want)
    for key in ("image_size", "colorspace", "hsamp", "vsamp", "dc", "ac", "dc_tbl", "ac_tbl", "restart_interval", "sof"):
        assert pa[key] == pb[key], key
    for x, y, z in zip(pa["quants"], pb["quants"], q):
        assert np.array_equal(x, y) and np.array_equal(x, z)


@pytest.mark.parametrize("name,size", [("ycc2x2", (141, 93)), ("ycc2x1", (120, 88)), ("gray", (77, 45))])
def test_compress_encode_with_restarts_then_read_returns_the_arrays(tq, name, size):
    hs, vs, cs = BY_NAME[name]
    rng = np.random.default_rng(94)
    big = torch.from_numpy(pixels(rng, (size[0] + 5, size[1]), len(hs))).cuda()
    im = tq.compress(big[:, 2:2 + size[0]], quality=75, hsamp=hs, vsamp=vs)          # a view: pitch beyond the row
    data = tq.encode(**im, restart_interval=16)
    back = tq.read(data)
    assert int(back["status"].item()) == 0
    assert back["image_size"] == size and back["hsamp"] == hs and back["vsamp"] == vs and back["colorspace"] == cs
    for ci, (x, y) in enumerate(zip(back["coefs"], im["coefs"])):
        assert torch.equal(x, y), f"component {ci}"
        assert np.array_equal(back["quants"][ci], im["quants"][ci])


def test_compress_smooth_decode_in_one_captured_graph(tq):
    """compress -> quantsmooth_ -> decode captured in one torch.cuda.graph and replayed on new pixels"""
    rng = np.random.default_rng(95)
    size, hs, vs = (150, 70), [2, 1, 1], [2, 1, 1]
    px = torch.from_numpy(pixels(rng, size, 3)).cuda()
    flags = pkg.flags_for_quality(3)
    ws = [tq.Workspace(), None, tq.Workspace()]
    outs = None

    def step():
        im = tq.compress(px, quality=40, hsamp=hs, vsamp=vs, out=outs, workspace=ws[0])
        res = tq.quantsmooth_(im["coefs"], im["quants"], flags, 2, hsamp=hs, vsamp=vs, colorspace=3, image_size=size,
                              workspace=ws[1])
        return im, res, tq.decode(im["coefs"], hsamp=hs, vsamp=vs, colorspace=3, image_size=size, result=res,
                                  workspace=ws[2])

    im, res, _ = step()                                        # eager: prepares the three workspaces
    ws[1] = res["workspace"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gim, gres, gout = step()
    for rep in range(3):
        px.copy_(torch.from_numpy(pixels(rng, size, 3)).cuda())
        g.replay()
        torch.cuda.synchronize()
        got, gstop = gout.cpu().numpy().copy(), int(gres["stop"].item())
        eim, eres, eout = step()                               # eager on the same pixels
        torch.cuda.synchronize()
        assert gstop == int(eres["stop"].item())
        assert np.array_equal(got, eout.cpu().numpy()), f"replay {rep}"
        assert got.shape == (size[1], size[0], 3)
        for ci, (x, y) in enumerate(zip(gim["coefs"], eim["coefs"])):
            assert torch.equal(x, y), f"replay {rep}, component {ci}"


def test_unsupported_input_writes_nothing(gpu, tq):
    """QS_HIP_ENOTSUP from every call for unsupported sampling and for fancy downsampling; ValueError from the torch layer"""
    rng = np.random.default_rng(96)
    px = pixels(rng, (48, 16), 3)
    q = tables("q50", 3, pkg.synth)
    ok = AbiImage(gpu, 0, px, q, [2, 1, 1], [2, 1, 1], 3)
    bad = AbiImage(gpu, 1, px, q, [3, 1, 1], [1, 1, 1], 3)
    nbytes = gpu.compress_batch_info([ok.job, ok.job])[1]
    ws = Guarded(nbytes)
    for call in (lambda: gpu.compress_batch_info([ok.job, bad.job]),
                 lambda: gpu.compress_batch_prepare([ok.job, bad.job], ws.view.data_ptr(), nbytes),
                 lambda: gpu.compress_batch([ok.job, bad.job], [ok.pix.view.data_ptr(), bad.pix.view.data_ptr()],
                                            [ok.pitch, bad.pitch], ws.view.data_ptr(), nbytes),
                 lambda: gpu.compress_batch_info([ok.job], fancy=True),
                 lambda: gpu.compress_batch_prepare([ok.job], ws.view.data_ptr(), nbytes, fancy=True)):
        with pytest.raises(pkg.hipqs.QsHipError) as e:
            call()
        assert e.value.code == -4
    torch.cuda.synchronize()
    for im in (ok, bad):
        for a in im.arr:
            a.check()
            assert bool((a.view == SENTINEL).all())
    dev = torch.from_numpy(px).cuda()
    with pytest.raises(ValueError, match="fancy"):
        tq.compress(dev, quality=50, fancy=True)
    with pytest.raises(ValueError, match="sampling"):
        tq.compress(dev, quality=50, hsamp=[3, 1, 1], vsamp=[1, 1, 1])
    with pytest.raises(ValueError, match="sampling"):
        tq.compress(dev, quality=50, hsamp=[2, 2, 2], vsamp=[2, 2, 2])
    with pytest.raises(ValueError):
        tq.compress(dev, quality=50, quants=q)
    with pytest.raises(ValueError):
        tq.compress(dev)
