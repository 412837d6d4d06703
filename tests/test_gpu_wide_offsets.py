"""The device stages past 2^31 and 2^32 bytes, bits and blocks.

Part B, addressing: tiny images (24 x 4104, gray and 4:2:0) whose pixel rows or coefficient blocks lie in buffers of more
than 2^32 bytes -- a row pitch of a megabyte, an array stride of 65 600 blocks -- compared bit for bit with libjpeg 9 on
the narrow image, every byte the stage does not own still holding its sentinel (checked on the device).
Part C, long scans: the periodic scans of tests/wide_cases.py at a scan of a little more than 2^32 bits and of a little
more than 2^32 bytes; what is expected is one period, proven against libjpeg 9 in tests/test_wide_cases.py, repeated on
the device.  The files the readers get are built from that period, never taken from the coder's output.

Every case asserts from the tensors it built that the offset it is about passes its threshold, prints its peak device
memory, and releases its tensors."""
import gc

import numpy as np
import pytest

import decode_cases as dc
import jpegqs_pkg
import wide_cases as W
from compress_fancy_oracle import CompressFancy9
from compress_oracle import pixels as synth_pixels
from decode_oracle import LibJpeg9, blocks_needed, synth_image
from decode_scaled_oracle import LibJpeg9Scaled, scaled_size
from encode_oracle import synth_scan_image
from encode_prog_oracle import LibJpeg9EncProg
from encode_rst_oracle import LibJpeg9EncRst, parse_rst
from helpers import MARGIN, Guarded
from read_oracle import LibjpegReader, expected_arrays
from read_prog_oracle import expected_arrays as expected_arrays_prog
from triangle_oracle import TriHost

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
jpeg_file = pkg.jpeg_file

P31, P32 = 1 << 31, 1 << 32
SIZE = (24, 4104)                                       # (width, height): 3 x 513 blocks, 1539 in all
LAYOUTS = {"gray": ([1], [1], 1), "420": ([2, 1, 1], [2, 1, 1], 3)}
SENT8 = 0xA5
SENT16 = int(np.array([0xA5A5], np.uint16).view(np.int16)[0])
SENT64 = int.from_bytes(b"\xa5" * 8, "little", signed=True)
POISON32 = int(np.array([32767, -32767], np.int16).view(np.int32)[0])       # +32767, -32767 in every pair of values
CHUNK = 1 << 27                                         # elements a device comparison takes at a time
ONES = [np.ones(64, np.uint16)]


@pytest.fixture(scope="module")
def tq():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible to torch")
    return pkg.torch_qs


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp
    return dict(lj9=LibJpeg9(d("lj9")), scaled=LibJpeg9Scaled(d("scaled")), tri=TriHost(d("tri")), enc=LibJpeg9EncRst(d("enc")),
                prog=LibJpeg9EncProg(d("prog")), reader=LibjpegReader(d("reader")), c9=CompressFancy9(d("c9")))


FAULT_TEXTS = ("illegal memory access", "hardware exception", "unspecified launch failure", "HSA_STATUS_ERROR",
               "device-side assert", "hipErrorLaunchFailure")


@pytest.fixture(autouse=True)
def _memory_and_faults(request):
    """Each case's peak device memory on stdout.  A device FAULT (FAULT_TEXTS: the device is then in no state to run
    anything, and a shared machine must not be handed more work after one) ends the session with exit status 3, which is
    session-level behaviour on purpose; any other error at the synchronisation -- an allocation failure among them -- is
    an ordinary error of the case, with its message."""
    torch.cuda.reset_peak_memory_stats()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        if any(t in str(e) for t in FAULT_TEXTS):
            pytest.exit(f"{request.node.name}: the device reported {e}; nothing more is run on it", returncode=3)
        raise
    print(f"\n[{request.node.name}] peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    gc.collect()
    torch.cuda.empty_cache()


# ---- checks that stay on the device ----------------------------------------------------------------------------------------

def _all_equal(t, value):
    """every element of a contiguous tensor equals value, compared in chunks of CHUNK elements"""
    flat = t.reshape(-1)
    bad = torch.zeros((), dtype=torch.bool, device=flat.device)
    for a in range(0, flat.numel(), CHUNK):
        bad |= (flat[a:a + CHUNK] != value).any()
    return not bool(bad)


def _margins_hold(g):
    return bool((g.raw[:MARGIN] == SENT8).all()) and bool((g.raw[g.raw.numel() - MARGIN:] == SENT8).all())


def _all_sentinel(g):
    """the whole Guarded region, margins included, holds the sentinel"""
    return _all_equal(g.raw.view(torch.int64), SENT64)


def _guarded(n, dtype=None):
    item = 1 if dtype is None else torch.empty(0, dtype=dtype).element_size()
    return Guarded(-(-n * item // 8) * 8 // item, dtype)


def _tiling_mismatch(buf, period, count):
    """the first index at which buf[:count] differs from `period` repeated, or -1; buf and period one-dimensional on the
    device"""
    L = period.numel()
    full = count // L
    rows = max(1, CHUNK // L)
    for r0 in range(0, full, rows):
        r1 = min(full, r0 + rows)
        ne = buf[r0 * L:r1 * L].view(r1 - r0, L) != period
        if bool(ne.any()):
            return r0 * L + int(ne.view(-1).nonzero()[0])
    rest = count - full * L
    if rest:
        ne = buf[full * L:count] != period[:rest]
        if bool(ne.any()):
            return full * L + int(ne.nonzero()[0])
    return -1


def _dev_bytes(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _parts_mismatch(buf, parts):
    """buf against the concatenation of W.Tiled parts -> None, or a description of the first difference"""
    at = 0
    for k, t in enumerate(parts):
        if t.head and not torch.equal(buf[at:at + len(t.head)], _dev_bytes(t.head)):
            return f"part {k}: the bytes in front of its scan, at byte {at}"
        at += len(t.head)
        bad = _tiling_mismatch(buf[at:at + t.body_len()], _dev_bytes(t.period), t.body_len())
        if bad >= 0:
            return f"part {k}: byte {bad} of the tiled bytes (period {len(t.period)}), byte {at + bad} of the buffer"
        at += t.body_len()
        if t.tail and not torch.equal(buf[at:at + len(t.tail)], _dev_bytes(t.tail)):
            return f"part {k}: the bytes behind its scan, at byte {at}"
        at += len(t.tail)
    return None


def _device_file(parts):
    """the concatenation of W.Tiled parts in a Guarded device buffer -> (guard, the file as a view of it)"""
    total = sum(len(t) for t in parts)
    room = total + max(len(t.period) for t in parts)       # (the last repetition is written whole, then cut)
    g = _guarded(room)
    at = 0
    for t in parts:
        L, h = len(t.period), len(t.head)
        g.view[at:at + h] = _dev_bytes(t.head)
        g.view[at + h:at + h + t.n * L].view(t.n, L).copy_(_dev_bytes(t.period))
        at += h + t.body_len()
        if t.tail:
            g.view[at:at + len(t.tail)] = _dev_bytes(t.tail)
        at += len(t.tail)
    assert at == total
    g.view[total:] = SENT8
    return g, g.view[:total]


# ---- part B: images --------------------------------------------------------------------------------------------------------

def _kw(im):
    return dict(hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"], image_size=im["image_size"])


def _image(layout, seed=1):
    hs, vs, cs = LAYOUTS[layout]
    return synth_image(np.random.default_rng([seed, len(hs)]), SIZE, hs, vs, cs)


def _scan_image(layout, seed=2):
    hs, vs, cs = LAYOUTS[layout]
    return synth_scan_image(np.random.default_rng([seed, len(hs)]), SIZE, hs, vs, cs)


def _dev(im):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in im["coefs"]]


@pytest.fixture(scope="module")
def _arena():
    g = _guarded(P32 + (1 << 25))
    yield g
    del g


@pytest.fixture
def arena(_arena):
    """2^32 + 2^25 bytes of sentinel between margins: the pixel buffer of every case.  Filled again behind each case, so
    that one that fails before it has restored its rows does not fail the cases behind it"""
    yield _arena
    _arena.raw.fill_(SENT8)


def _pitch_for(rows, past):
    """an odd row pitch that puts row rows - 1 at least `past` bytes behind row 0"""
    return (-(-past // (rows - 1))) | 1


def _wide_rows(arena, off, h, pitch, w, c):
    """-> (the rows as (h, pitch), the image as (h, w, c)) at byte `off` of the arena"""
    assert off + h * pitch <= arena.view.numel()
    rows = arena.view[off:off + h * pitch].view(h, pitch)
    return rows, rows[:, :w * c].view(h, w, c)


def _expected_pixels(tools, im, mode, denom):
    if denom != 1:
        return tools["scaled"].decode(im, denom)
    if mode == "triangle" and len(im["coefs"]) > 1:
        return tools["tri"].run([im])[0]                 # (the host build, pinned to libjpeg-turbo by the fixtures)
    return tools["lj9"].decode(im["coefs"], im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"])


DECODE_MODES = [("dct", 1, P32), ("dct", 1, P31), ("triangle", 1, P32), ("dct", 2, P32), ("dct", 4, P32), ("dct", 8, P32)]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("mode,denom,past", DECODE_MODES, ids=[f"{m}-1/{d}-past2^{p.bit_length() - 1}" for m, d, p in DECODE_MODES])
def test_decode_into_rows_past_the_threshold(tq, tools, arena, layout, mode, denom, past):
    """decode_batch with outs= a view whose last row starts `past` bytes behind its first: odd pitch, misaligned base"""
    im = _image(layout)
    w, h = scaled_size(SIZE, denom)
    c = 1 if layout == "gray" else 3
    off = 1 + (denom + c) % 3
    pitch = _pitch_for(h, past)
    rows, view = _wide_rows(arena, off, h, pitch, w, c)
    last = view[h - 1].data_ptr() - view.data_ptr()
    assert last >= past and (past == P32 or last < P32) and view.data_ptr() % 4 == off and view.stride(0) % 2 == 1
    r = tq.decode_batch([dict(coefs=_dev(im), quants=im["quants"], **_kw(im))], outs=[view], upsampling=mode,
                        scale_denom=denom)
    torch.cuda.synchronize()
    assert r["images"][0].data_ptr() == view.data_ptr()
    got = view.cpu().numpy()
    rows[:, :w * c] = SENT8
    assert _all_sentinel(arena), "a byte outside the image's rows changed (row gaps, the bytes around them, the margins)"
    want = _expected_pixels(tools, im, mode, denom)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert not len(bad), f"{len(bad)} samples differ, first at (y, x, channel) = {tuple(bad[0])}"


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("mode", ["box", "dct"])
def test_compress_from_rows_past_2_32(tq, tools, arena, layout, mode):
    hs, vs, cs = LAYOUTS[layout]
    c = len(hs)
    w, h = SIZE
    px = synth_pixels(np.random.default_rng([3, c]), SIZE, c)
    quants = [pkg.synth.quality_table(pkg.synth.STD_LUMA if ci == 0 else pkg.synth.STD_CHROMA, 75) for ci in range(c)]
    off, pitch = 3, _pitch_for(h, P32)
    rows, view = _wide_rows(arena, off, h, pitch, w, c)
    assert view[h - 1].data_ptr() - view.data_ptr() >= P32
    view.copy_(torch.from_numpy(px).cuda())
    r = tq.compress_batch([dict(pixels=view, quants=quants, hsamp=hs, vsamp=vs, colorspace=cs)], downsampling=mode)
    torch.cuda.synchronize()
    assert np.array_equal(view.cpu().numpy(), px), "the compress changed its input"
    rows[:, :w * c] = SENT8
    assert _all_sentinel(arena)
    c9 = tools["c9"]
    want = (c9.libjpeg if mode == "dct" else c9.libjpeg_box)(px, quants, hs, vs, cs)["coefs"]
    for ci, (a, b) in enumerate(zip(r["images"][0]["coefs"], want)):
        a = a.cpu().numpy()
        assert a.shape == b.shape
        bad = np.argwhere((a != b).any(axis=2))
        assert not len(bad), f"component {ci}: {len(bad)} blocks differ, first at (by, bx) = {tuple(bad[0])}"


def test_a_wide_job_in_the_second_launch_chunk(tq, tools, arena):
    """46 decode jobs, the last of them -- in the second launch chunk -- the 4:2:0 image with rows a megabyte apart"""
    chunk = dc.header_constant("QS_DEC_CHUNK")
    ims = dc.chunk_batch(chunk + 1) + [_image("420")]
    assert len(ims) == 46 > chunk
    w, h = SIZE
    rows, view = _wide_rows(arena, 2, h, _pitch_for(h, P32), w, 3)
    assert view[h - 1].data_ptr() - view.data_ptr() >= P32
    shapes = [(im["image_size"][1], im["image_size"][0], 1 if len(im["coefs"]) == 1 else 3) for im in ims[:-1]]
    guards = [Guarded(a * b * c) for a, b, c in shapes]
    tq.decode_batch([dict(coefs=_dev(im), quants=im["quants"], **_kw(im)) for im in ims],
                    outs=[g.view.view(s) for g, s in zip(guards, shapes)] + [view])
    torch.cuda.synchronize()
    lj9 = tools["lj9"]
    got = [g.view.cpu().numpy().reshape(s) for g, s in zip(guards, shapes)] + [view.cpu().numpy()]
    rows[:, :w * 3] = SENT8
    assert _all_sentinel(arena)
    for k, (im, px) in enumerate(zip(ims, got)):
        if k < len(guards):
            guards[k].check()
        want = lj9.decode(im["coefs"], im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"])
        assert np.array_equal(px, want), f"job {k}"


# ---- part B: coefficient arrays of more than 2^25 blocks ----------------------------------------------------------------------

class BigArrays:
    """per component a Guarded int16 array (rows, stride, 64) with rows = the image's block rows + 1 and a stride that puts
    the image's LAST block row more than 2^32 bytes (2^31 values) behind the first"""

    def __init__(self, layout):
        hs, vs, _cs = LAYOUTS[layout]
        self.need = [blocks_needed(SIZE, hs, vs, ci) for ci in range(len(hs))]
        self.shapes = [(hb + 1, -(-(1 << 25) // (hb - 1)) + 64) for hb, _wb in self.need]
        self.guards = [_guarded(rows * stride * 64, torch.int16) for rows, stride in self.shapes]
        self.arrs = [g.view[:rows * stride * 64].view(rows, stride, 64) for g, (rows, stride) in zip(self.guards, self.shapes)]
        for t, (hb, _wb), (rows, stride) in zip(self.arrs, self.need, self.shapes):
            assert rows * stride > 1 << 25
            assert t[hb - 1, 0].data_ptr() - t.data_ptr() >= P32 and (hb - 1) * t.stride(0) >= P31

    def fill(self, value32=None):
        """poison (+-32767) for a stage that reads, the sentinel for one that writes"""
        for g in self.guards:
            if value32 is None:
                g.view.view(torch.int64).fill_(SENT64)
            else:
                g.view.view(torch.int32).fill_(value32)

    def put(self, coefs):
        for t, c in zip(self.arrs, coefs):
            t[:c.shape[0], :c.shape[1]] = torch.from_numpy(np.ascontiguousarray(c)).cuda()

    def corner(self, extra=0):
        return [t[:hb + extra, :wb + extra].cpu().numpy() for t, (hb, wb) in zip(self.arrs, self.need)]

    def rest_is(self, value64, extra=0, what=""):
        """with the image's corner overwritten, every value of every array is the fill, and the margins hold"""
        for ci, (g, t, (hb, wb)) in enumerate(zip(self.guards, self.arrs, self.need)):
            t[:hb + extra, :wb + extra].view(torch.int32).fill_(int(np.array([value64], np.int64).view(np.int32)[0]))
            assert _margins_hold(g), f"{what}: component {ci}: a sentinel margin changed"
            assert _all_equal(g.view.view(torch.int64), value64), f"{what}: component {ci}: a block outside the image changed"


POISON64 = int(np.array([POISON32, POISON32], np.int32).view(np.int64)[0])


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_stages_that_read_arrays_of_more_than_2_25_blocks(tq, tools, layout):
    """decode in three modes, encode_batch, encode_file_batch(optimize) and the progressive coder with refinement scans, on
    arrays whose blocks outside the image hold +-32767: libjpeg 9 on the unpadded arrays"""
    big = BigArrays(layout)
    big.fill(POISON32)
    im = _image(layout)
    big.put(im["coefs"])
    job = dict(coefs=big.arrs, quants=im["quants"], **_kw(im))
    for mode, denom in (("dct", 1), ("triangle", 1), ("dct", 2)):
        px = tq.decode_batch([job], upsampling=mode, scale_denom=denom)["images"][0].cpu().numpy()
        want = _expected_pixels(tools, im, mode, denom)
        assert px.shape == want.shape and np.array_equal(px, want), f"decode {mode} 1/{denom}"
    assert all(np.array_equal(a, b) for a, b in zip(big.corner(), im["coefs"]))
    im = _scan_image(layout)
    big.put(im["coefs"])
    job = dict(coefs=big.arrs, quants=im["quants"], **_kw(im))
    enc, prog = tools["enc"], tools["prog"]
    assert tq.encode_batch([job], restart_interval=5)[0] == enc.write(im, 5, 0), "encode_batch"
    r = tq.encode_file_batch([job], optimize=True)
    assert r["status"].cpu().tolist() == [0]
    assert r["files"][0][:int(r["len"][0])].cpu().numpy().tobytes() == enc.write(im, 0, 0, optimize=True), "optimize"
    script = jpeg_file.simple_progression(len(im["coefs"]), im["colorspace"])
    r = tq.encode_file_batch([job], scans=script, refinement=True, restart_interval=7)
    assert r["status"].cpu().tolist() == [0]
    assert r["files"][0][:int(r["len"][0])].cpu().numpy().tobytes() == prog.write(im, script, 7, 0), "progressive"
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(big.corner(), im["coefs"])), "a stage changed its input"
    big.rest_is(POISON64, what="inputs")


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_stages_that_write_arrays_of_more_than_2_25_blocks(tq, tools, layout):
    """compress (box and dct) writes the image's blocks and nothing else; the three readers zero the whole array and fill
    the image's blocks (and, 4:2:0, the dummy blocks of its edge MCUs): libjpeg 9's arrays of the same input"""
    hs, vs, cs = LAYOUTS[layout]
    n = len(hs)
    big = BigArrays(layout)
    c9, enc, prog, reader = tools["c9"], tools["enc"], tools["prog"], tools["reader"]
    px = synth_pixels(np.random.default_rng([4, n]), SIZE, n)
    quants = [pkg.synth.quality_table(pkg.synth.STD_LUMA if ci == 0 else pkg.synth.STD_CHROMA, 75) for ci in range(n)]
    for mode in ("box", "dct"):
        big.fill()
        tq.compress_batch([dict(pixels=torch.from_numpy(px).cuda(), quants=quants, hsamp=hs, vsamp=vs, colorspace=cs)],
                          downsampling=mode, outs=[big.arrs])
        torch.cuda.synchronize()
        want = (c9.libjpeg if mode == "dct" else c9.libjpeg_box)(px, quants, hs, vs, cs)["coefs"]
        for ci, (a, b) in enumerate(zip(big.corner(), want)):
            assert np.array_equal(a, b), f"compress {mode}: component {ci}"
        big.rest_is(SENT64, what=f"compress {mode}")
    im = _scan_image(layout)
    script = jpeg_file.simple_progression(n, im["colorspace"])
    files = [("intervals", enc.write(im, 4, 0), dict()), ("split", enc.write(im, 0, 0), dict(split=True)),
             ("progressive", prog.write(im, script, 4, 0), dict())]
    shapes = [(hb + 1, wb + 1) for hb, wb in big.need]
    for name, data, kw in files:
        big.fill()
        r = tq.read_batch([data], outs=[big.arrs], **kw)
        torch.cuda.synchronize()
        assert r["status"].cpu().tolist() == [0], name
        ref, clean = reader.read_bytes(data)
        assert clean
        want = expected_arrays_prog(ref, shapes, script) if name == "progressive" else expected_arrays(ref, shapes)
        for ci, (a, b) in enumerate(zip(big.corner(1), want)):
            assert np.array_equal(a, b), f"{name}: component {ci}"
        big.rest_is(0, extra=1, what=name)


# ---- part C: long scans ----------------------------------------------------------------------------------------------------

def _gray_job(coefs):
    hb, wb = coefs.shape[:2]
    return dict(coefs=[coefs], quants=ONES, hsamp=[1], vsamp=[1], colorspace=1, image_size=(8 * wb, 8 * hb))


def _restart_coefs(pattern, n, wb):
    assert (n * W.PERIOD) % wb == 0 and n * W.PERIOD // wb <= 8191
    return torch.from_numpy(pattern).cuda().repeat(n, 1).view(n * W.PERIOD // wb, wb, 64)


def _norestart_coefs(row, n):
    assert 8 * n <= 8191
    return torch.from_numpy(row).cuda().repeat(8 * n, 1).view(8 * n, len(row), 64)


def _run_scan(tq, job, out, cap, **kw):
    r = tq.encode_scan_batch([job], outs=[out.view[:cap]], **kw)
    torch.cuda.synchronize()
    return int(r["len"][0]), int(r["status"][0]), r["workspace"]


def test_encode_a_scan_of_more_than_2_32_bytes_with_restart_intervals(tq, tools):
    """encode_scan_batch, restart interval 32: the whole segment, then once more into 2^32 + 5 bytes"""
    pattern = W.restart_pattern()
    one = parse_rst(tools["enc"].write(W.restart_image(pattern, 1, W.WB_SMALL), W.RI, 0))["segment"]
    n = W.periods_past(W.BYTES, len(one) + 2, unit=W.WB_BYTES // W.PERIOD)
    t = W.tile_restart_segment(one, n)
    want = t.body_len()
    assert P32 <= want < 1.01 * P32
    job = _gray_job(_restart_coefs(pattern, n, W.WB_BYTES))
    out = _guarded(want + 4096)
    period = _dev_bytes(t.period)
    length, status, ws = _run_scan(tq, job, out, want + 4096, restart_interval=W.RI)
    assert (length, status) == (want, 0)
    assert _tiling_mismatch(out.view, period, want) == -1
    assert _all_equal(out.view[want:], SENT8) and _margins_hold(out), "bytes behind the segment changed"
    out.raw.fill_(SENT8)
    cap = P32 + 5
    r = tq.encode_scan_batch([job], outs=[out.view[:cap]], workspace=ws, restart_interval=W.RI)
    torch.cuda.synchronize()
    assert (int(r["len"][0]), int(r["status"][0])) == (want, 2)
    assert _tiling_mismatch(out.view, period, cap) == -1
    assert _all_equal(out.view[cap:], SENT8) and _margins_hold(out), "bytes at or beyond the capacity changed"
    assert _tiling_mismatch(job["coefs"][0].view(-1), torch.from_numpy(pattern).cuda().view(-1), n * W.PERIOD * 64) == -1


def test_encode_a_scan_of_more_than_2_32_bytes_without_restarts(tq, tools):
    row = W.norestart_row(W.SEED, W.WB_BYTES)
    one = parse_rst(tools["enc"].write(W.norestart_image(row, 1), 0, 0))["segment"]
    n = W.periods_past(W.BYTES, len(one))
    t = W.tile_norestart_segment(one, n)
    want = t.body_len()
    assert P32 <= want < 1.01 * P32
    job = _gray_job(_norestart_coefs(row, n))
    out = _guarded(want + 4096)
    length, status, _ws = _run_scan(tq, job, out, want + 4096)
    assert (length, status) == (want, 0)
    assert _tiling_mismatch(out.view, _dev_bytes(t.period), want) == -1
    assert _all_equal(out.view[want:], SENT8) and _margins_hold(out)


def _bits_size_n(make):
    """n of a scan of a little more than 2^32 bits, where the period's bytes depend (weakly) on n through the tables:
    make(n) -> the Tiled scan"""
    n = 2
    for _ in range(4):
        n = W.periods_past(W.BITS // 8, len(make(n).period), unit=W.WB_BITS // W.PERIOD)
    t = make(n)
    assert P32 <= 8 * t.body_len() < 1.01 * P32
    return n


def test_optimized_file_of_a_scan_of_more_than_2_32_bits(tq, tools):
    """encode_file_batch(optimize=True), restart interval 32: the counts are n times one pattern's, the tables libjpeg's of
    those counts, the file the framing, those tables and the tiled scan.  torch_qs.encode_file_batch hands out the tables of
    its run but not its d_counts: the counts are compared on encode_histogram_batch, the same kernel on the same job, and
    those of the file's own run only through the tables made of them"""
    pattern = W.restart_pattern()
    n = _bits_size_n(lambda k: W.optimized_restart(pattern, k)[2])
    counts, (dc, ac), seg = W.optimized_restart(pattern, n)
    job = _gray_job(_restart_coefs(pattern, n, W.WB_BITS))
    head, mid = jpeg_file.compose_parts(ONES, [1], [1], 1, job["image_size"], {0: dc, 1: dc}, {0: ac, 1: ac}, W.RI)
    t = W.Tiled(head + mid, seg.period, n, seg.cut, b"\xff\xd9")
    h = tq.encode_histogram_batch([job], restart_interval=W.RI)
    got = h["counts"][0].cpu().numpy()
    assert h["status"].cpu().tolist() == [0]
    assert np.array_equal(got[0, :256], counts[0, :256] * n) and np.array_equal(got[2, :256], counts[1, :256] * n)
    out = _guarded(len(t) + 4096)
    r = tq.encode_file_batch([job], optimize=True, outs=[out.view[:len(t) + 4096]], restart_interval=W.RI)
    torch.cuda.synchronize()
    assert (int(r["len"][0]), int(r["status"][0])) == (len(t), 0)
    tabs = tq.huffman_of_tables(r["tables"][0])
    assert (list(tabs["dc"][0][0]), list(tabs["dc"][0][1])) == (list(dc[0]), list(dc[1]))
    assert (list(tabs["ac"][0][0]), list(tabs["ac"][0][1])) == (list(ac[0]), list(ac[1]))
    assert _parts_mismatch(out.view, [t]) is None
    assert _all_equal(out.view[len(t):], SENT8) and _margins_hold(out)


def _progressive_parts(pattern, n):
    size = (8 * W.WB_BITS, 8 * n * W.PERIOD // W.WB_BITS)
    return W.progressive_restart(pattern, n, jpeg_file.compose_parts(ONES, [1], [1], 1, size, progressive=True)[0])


def _progressive_file_is(tq, job, parts, script, ri, **kw):
    total = sum(len(p) for p in parts)
    out = _guarded(total + 4096)
    r = tq.encode_file_batch([job], scans=script, outs=[out.view[:total + 4096]], restart_interval=ri, **kw)
    torch.cuda.synchronize()
    assert (int(r["len"][0]), int(r["status"][0])) == (total, 0)
    assert _parts_mismatch(out.view, parts) is None
    assert _all_equal(out.view[total:], SENT8) and _margins_hold(out)


def test_progressive_file_with_an_ac_scan_of_more_than_2_32_bits(tq, tools):
    """encode_file_batch(scans=[DC; AC 1..63]), restart interval 32: each scan tiled under its own tables"""
    pattern = W.restart_pattern()
    n = _bits_size_n(lambda k: W.progressive_restart(pattern, k, b"")[1])
    job = _gray_job(_restart_coefs(pattern, n, W.WB_BITS))
    _progressive_file_is(tq, job, _progressive_parts(pattern, n), W.DC_AC_SCRIPT, W.RI)


def test_refinement_scan_whose_running_weight_passes_2_32(tq, tools):
    """DC, AC 1..63 at Al = 1 and its refinement with restart interval 1 on 4.3 M blocks that all end in zeros with
    correction bits buffered: every block is a head and weighs its tail + QR_CORR_MAX + 1, so the 32-bit sum qr_wscan
    carries across workgroups wraps inside the scan, and qr_next takes its differences across the wrap.  The first block
    whose running sum has passed 2^32 is block 4 323 612 of 4 345 856: 22 244 blocks, 86 workgroups, lie behind it"""
    pattern = W.refine_pattern()
    n = W.refine_periods(pattern)
    assert P32 <= W.refine_weight(pattern, n) < 1.01 * P32
    wrap = W.wrap_block(W.refine_block_weights(1), n)
    assert wrap == 4323612 and n * len(pattern) - wrap == 22244
    hb = n * len(pattern) // W.REFINE_WB
    coefs = torch.from_numpy(pattern).cuda().repeat(n, 1).view(hb, W.REFINE_WB, 64)
    job = _gray_job(coefs)
    head = jpeg_file.compose_parts(ONES, [1], [1], 1, job["image_size"], progressive=True)[0]
    _progressive_file_is(tq, job, W.progressive_tiled(pattern, n, head, W.GRAY_REFINE, 1), W.GRAY_REFINE, 1, refinement=True)


def test_refinement_scan_without_restarts_whose_running_weight_passes_2_32(tq, tools):
    """the mirror: no restart markers, the heads are the writing blocks, and every run piece spans the three blocks of
    correction bits between two of them: qr_next's binary search takes its differences across the wrap of the sum.  The
    first block whose running sum has passed 2^32 is block 15 243 896 of 15 321 088, the first of a group: the piece of the
    three blocks in front of it ends on the wrap, and 77 192 blocks (more than two of qr_next's search ranges of 32 767)
    lie behind it"""
    pattern = W.refine_norestart_pattern()
    n = W.refine_periods(pattern, W.refine_weight_norestart)
    assert P32 <= W.refine_weight_norestart(pattern, n) < 1.01 * P32
    wrap = W.wrap_block(W.refine_block_weights(0), n)
    assert wrap == 15243896 and wrap % (1 + W.GROUP_TAILS) == 0 and n * len(pattern) - wrap == 77192
    hb = n * len(pattern) // W.REFINE_WB
    coefs = torch.from_numpy(pattern).cuda().repeat(n, 1).view(hb, W.REFINE_WB, 64)
    job = _gray_job(coefs)
    head = jpeg_file.compose_parts(ONES, [1], [1], 1, job["image_size"], progressive=True)[0]
    _progressive_file_is(tq, job, W.progressive_tiled(pattern, n, head, W.GRAY_REFINE, 0), W.GRAY_REFINE, None, refinement=True)


def _read_and_compare(tq, data, arr, unit, what, **kw):
    arr.fill_(SENT16)
    r = tq.read_batch([data], outs=[[arr]], **kw)
    torch.cuda.synchronize()
    status = r["status"].cpu().tolist()
    if status == [0]:
        assert _tiling_mismatch(arr.view(-1), unit, arr.numel()) == -1, what
    return status


def test_read_a_scan_of_more_than_2_32_bytes_by_intervals(tq, tools):
    """read_batch on the tiled restart file (built on the device from libjpeg's file of one pattern): the pattern tiled,
    status 0; the same file without its last 1000 bytes: status 2, as the host build gives at n = 3"""
    pattern = W.restart_pattern()
    one = tools["enc"].write(W.restart_image(pattern, 1, W.WB_SMALL), W.RI, 0)
    n = W.periods_past(W.BYTES, len(parse_rst(one)["segment"]) + 2, unit=W.WB_BYTES // W.PERIOD)
    hb = n * W.PERIOD // W.WB_BYTES
    t = W.tile_file(one, n, (8 * W.WB_BYTES, 8 * hb))
    assert t.body_len() >= P32
    fg, data = _device_file([t])
    ag = _guarded(hb * W.WB_BYTES * 64, torch.int16)
    arr = ag.view[:hb * W.WB_BYTES * 64].view(hb, W.WB_BYTES, 64)
    unit = torch.from_numpy(pattern).cuda().view(-1)
    assert _read_and_compare(tq, data, arr, unit, "intervals") == [0]
    assert _margins_hold(ag) and _margins_hold(fg)
    assert _parts_mismatch(data, [t]) is None, "the reader changed its input"
    assert _read_and_compare(tq, data[:len(t) - W.TRUNCATE], arr, unit, "truncated") == [W.STATUS_TRUNCATED_INTERVALS]
    assert _margins_hold(ag)


def test_read_a_scan_of_more_than_2_32_bytes_by_the_split_route(tq, tools):
    row = W.norestart_row(W.SEED, W.WB_BYTES)
    one = tools["enc"].write(W.norestart_image(row, 1), 0, 0)
    n = W.periods_past(W.BYTES, len(parse_rst(one)["segment"]))
    t = W.tile_file(one, n, (8 * W.WB_BYTES, 64 * n), restart=False)
    assert t.body_len() >= P32
    fg, data = _device_file([t])
    ag = _guarded(8 * n * W.WB_BYTES * 64, torch.int16)
    arr = ag.view[:8 * n * W.WB_BYTES * 64].view(8 * n, W.WB_BYTES, 64)
    unit = torch.from_numpy(row).cuda().view(-1)
    assert _read_and_compare(tq, data, arr, unit, "split", split=True) == [0]
    assert _margins_hold(ag) and _margins_hold(fg)
    assert _read_and_compare(tq, data[:len(t) - W.TRUNCATE], arr, unit, "truncated", split=True) == [W.STATUS_TRUNCATED_SPLIT]
    assert _margins_hold(ag)


def _read_progressive_tiled(parts, pattern, wb, n, truncated=W.STATUS_TRUNCATED_PROGRESSIVE):
    """qs_hip_read_prog_device_batch on the file of W.Tiled parts, built on the device, and on the same file without its last
    1000 bytes.  The scans' tables come from jpeg_file.parse_progressive of the same file at n = 1, their offsets from the
    tiling -- torch_qs.read_progressive_batch would search the whole file for markers on the host, hundreds of megabytes
    in Python, so the wrapper itself is covered at small sizes only.  truncated: the status of
    the cut file, as the host build gives it at n = 3.  -> the offsets given"""
    total = sum(len(p) for p in parts)
    hb = n * W.PERIOD // wb
    p = jpeg_file.parse_progressive(b"".join(W.Tiled(q.head, q.period, 1, q.cut, q.tail).bytes() for q in parts))
    assert p["image_size"] == (8 * wb, 8 * hb) and len(p["scans"]) == len(parts)
    scans = [dict(s) for s in p["scans"]]
    for k, s in enumerate(scans):
        s["offset"] = sum(len(q) for q in parts[:k]) + len(parts[k].head)
    fg, data = _device_file(parts)
    ag = _guarded(hb * wb * 64, torch.int16)
    arr = ag.view[:hb * wb * 64].view(hb, wb, 64)
    arr.fill_(SENT16)
    hip = pkg.HipQS()
    jobs = [hip.device_job([arr.data_ptr()], [(hb, wb)], [None], hsamp=[1], vsamp=[1], colorspace=1, image_size=p["image_size"])]
    opts = [hip.read_prog_opts(scans)]
    _per, nbytes = hip.read_prog_batch_info(jobs, opts)
    ws, status = _guarded(nbytes), Guarded(2, torch.int32)
    stream = torch.cuda.current_stream().cuda_stream
    hip.read_prog_batch_prepare(jobs, opts, ws.view.data_ptr(), nbytes, stream)
    unit = torch.from_numpy(pattern).cuda().view(-1)
    for nbytes_file, want in ((total, 0), (total - W.TRUNCATE, truncated)):
        hip.read_prog_batch(jobs, [data.data_ptr()], [nbytes_file], status.view.data_ptr(), ws.view.data_ptr(), nbytes, stream)
        torch.cuda.synchronize()
        assert int(status.view[0]) == want
        if want == 0:
            assert _tiling_mismatch(arr.view(-1), unit, arr.numel()) == -1
        assert _margins_hold(ag) and _margins_hold(ws) and _margins_hold(fg)
    assert _parts_mismatch(data, parts) is None, "the reader changed its input"
    return [s["offset"] for s in scans]


def test_read_a_progressive_file_with_an_ac_scan_of_more_than_2_32_bits(tq, tools):
    pattern = W.restart_pattern()
    n = _bits_size_n(lambda k: W.progressive_restart(pattern, k, b"")[1])
    _read_progressive_tiled(_progressive_parts(pattern, n), pattern, W.WB_BITS, n)


def _offset_parts(pattern):
    """[DC; AC 1..62; AC 63..63] on so many patterns that the last SOS header ends a little more than 2^31 bytes into the
    file -> (n, the Tiled parts, that offset)"""
    unit = W.WB_OFFSET // W.PERIOD
    n = unit
    for _ in range(4):
        parts = W.progressive_tiled(pattern, n, b"", W.DC_AC_AC_SCRIPT, W.RI)
        n = W.periods_past(P31, len(parts[0].period) + len(parts[1].period), unit=unit)
    size = (8 * W.WB_OFFSET, 8 * n * W.PERIOD // W.WB_OFFSET)
    head = jpeg_file.compose_parts(ONES, [1], [1], 1, size, progressive=True)[0]
    parts = W.progressive_tiled(pattern, n, head, W.DC_AC_AC_SCRIPT, W.RI)
    offset = len(parts[0]) + len(parts[1]) + len(parts[2].head)
    assert P31 <= offset < 1.01 * P31 and size[1] <= 65500
    return n, parts, offset


def test_progressive_file_with_a_scan_behind_2_31_bytes(tq, tools):
    """encode_file_batch(scans=[DC; AC 1..62; AC 63..63]), restart interval 32, 25 M blocks: the coder places its third
    scan, and EOI, past 2^31 bytes of the file"""
    pattern = W.restart_pattern()
    n, parts, _offset = _offset_parts(pattern)
    job = _gray_job(_restart_coefs(pattern, n, W.WB_OFFSET))
    _progressive_file_is(tq, job, parts, W.DC_AC_AC_SCRIPT, W.RI)


def test_read_a_progressive_file_whose_last_scan_starts_past_2_31_bytes(tq, tools):
    """the scan `offset` of qs_hip_read_prog as a 64-bit value: the third scan's is past 2^31, and the reader's
    `offset - length` and limit arithmetic runs there; the truncated copy lacks the last 21 intervals of that scan: status 1"""
    pattern = W.restart_pattern()
    n, parts, offset = _offset_parts(pattern)
    offsets = _read_progressive_tiled(parts, pattern, W.WB_OFFSET, n, truncated=W.STATUS_TRUNCATED_SHORT_SCAN)
    assert offsets[-1] == offset >= P31 > offsets[1] and len(parts[2]) > W.TRUNCATE
