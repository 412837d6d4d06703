"""Whole JPEG files built on the device (torch_qs.encode_file_batch / encode_file, qs_hip_encode_device_batch_files):
histogram, optimal tables, DHT markers, framing and the segment in one run, against libjpeg 9 itself writing the same
arrays with optimize_coding (tests/libjpeg9_encode.c)."""
import numpy as np
import pytest

import jpegqs_pkg
from decode_oracle import GOLD, LibJpeg9
from encode_oracle import GOLDEN, LAYOUTS, SIZES, LibJpeg9Enc, parse_jpeg, synth_scan_image
from encode_rst_oracle import LibJpeg9EncRst, layout_cases
from helpers import Guarded

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
jpeg_file = pkg.jpeg_file


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    return LibJpeg9Enc(tmp_path_factory.mktemp("lj9enc"))


@pytest.fixture(scope="module")
def rst(tmp_path_factory):
    return LibJpeg9EncRst(tmp_path_factory.mktemp("lj9rst"))


@pytest.fixture(scope="module")
def lj9(tmp_path_factory):
    return LibJpeg9(tmp_path_factory.mktemp("lj9"))


@pytest.fixture(scope="module")
def tq():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible to torch")
    return pkg.torch_qs


def _dev(im):
    """the arrays on the device, each between margins"""
    out = []
    for c in im["coefs"]:
        g = Guarded(c.size, torch.int16)
        g.view.copy_(torch.from_numpy(np.ascontiguousarray(c).reshape(-1)))
        out.append((g, g.view.view(c.shape)))
    return out


def _kw(im):
    return dict(hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"], image_size=im["image_size"])


def _batch(ims):
    devs = [_dev(im) for im in ims]
    return devs, [dict(coefs=[t for _g, t in d], quants=im["quants"], **_kw(im)) for d, im in zip(devs, ims)]


def _check_inputs(devs, ims):
    for d, im in zip(devs, ims):
        for (g, t), c in zip(d, im["coefs"]):
            g.check()
            assert np.array_equal(t.cpu().numpy(), c), "the encoder changed an input array"


def _files(tq, ims, caps=None, **kw):
    """encode_file_batch with every output between margins and one byte off any alignment -> (files as bytes or None,
    len, status, guards, the call's result)"""
    devs, batch = _batch(ims)
    if caps is None:
        caps = [8192 + 72 * sum(c.shape[0] * c.shape[1] for c in im["coefs"]) for im in ims]
    outs = [Guarded(c + 1) for c in caps]
    r = tq.encode_file_batch(batch, outs=[o.view[1:] for o in outs], **kw)
    torch.cuda.synchronize()
    lens, status = r["len"].cpu().tolist(), r["status"].cpu().tolist()
    for o in outs:
        o.check()
        assert int(o.view[0]) == 0xA5, "the byte in front of the buffer changed"
    _check_inputs(devs, ims)
    files = [o.view[1:1 + l].cpu().numpy().tobytes() if s == 0 else None for o, l, s in zip(outs, lens, status)]
    return files, lens, status, outs, r


def _tiny_images():
    rng = np.random.default_rng(77)
    one_block = synth_scan_image(rng, (5, 3), [1], [1], 1)
    one_mcu = [synth_scan_image(rng, (16, 16), [2, 1, 1], [2, 1, 1], 3), synth_scan_image(rng, (9, 2), [2, 1, 1], [2, 1, 1], 3),
               synth_scan_image(rng, (32, 8), [4, 1, 1], [1, 1, 1], 3), synth_scan_image(rng, (3, 3), [1, 1, 1, 1], [1, 1, 1, 1], 4)]
    return [("one block", one_block)] + [(f"one MCU {k}", im) for k, im in enumerate(one_mcu)]


@pytest.fixture(scope="module")
def corpus(lj9):
    ims = [(n, lj9.read(GOLD / f"{n}.jpg")) for n in GOLDEN]
    for li, (hs, vs, cs) in enumerate(LAYOUTS):
        for size in SIZES:
            ims.append((f"layout {li} at {size}", synth_scan_image(np.random.default_rng(li * 1000 + size[0]), size, hs, vs, cs)))
    return ims + _tiny_images()


@pytest.fixture(scope="module")
def optimized(enc, corpus):
    """libjpeg's optimized file of every corpus image, written once"""
    return [enc.write(im, optimize=True) for _n, im in corpus]


def test_optimized_files_equal_libjpeg_in_one_mixed_batch(tq, corpus, optimized):
    """golden images, every layout x odd sizes, one-block and one-MCU images: more jobs than one launch chunk; the
    tables come back as well"""
    assert len(corpus) > 32
    files, lens, status, _outs, r = _files(tq, [im for _n, im in corpus])
    assert status == [0] * len(corpus)
    for k, ((name, im), f, w, l) in enumerate(zip(corpus, files, optimized, lens)):
        assert f == w and l == len(w), name
        p = parse_jpeg(w)
        h = tq.huffman_of_tables(r["tables"][k])
        assert {t: (list(b), list(v)) for t, (b, v) in p["dc"].items()} == h["dc"], name
        assert {t: (list(b), list(v)) for t, (b, v) in p["ac"].items()} == h["ac"], name


def test_standard_and_caller_tables(tq, enc, corpus, optimized):
    ims = [im for _n, im in corpus]
    files, _lens, status, _outs, r = _files(tq, ims, optimize=False)
    assert status == [0] * len(ims) and r["tables"] is None
    for (name, im), f in zip(corpus, files):
        assert f == enc.write(im), name
    huff = [dict(dc=parse_jpeg(w)["dc"], ac=parse_jpeg(w)["ac"]) for w in optimized]
    files, _lens, status, _outs, _r = _files(tq, ims, optimize=False, huffman=huff)
    assert status == [0] * len(ims)
    for (name, _im), f, w in zip(corpus, files, optimized):
        assert f == w, name
    with pytest.raises(ValueError, match="exclude"):
        tq.encode_file_batch(_batch(ims[:1])[1], optimize=True, huffman=huff[:1])


def test_restart_intervals_with_optimize(tq, rst):
    """restart_interval in {1, 2, 7} and restart_in_rows = 1 on every layout and size: the tables are counted from the
    restart scan and the DRI bytes sit in the mid"""
    cases = [c for c in layout_cases() if (c[3] == 0 and c[2] in (1, 2, 7)) or (c[2] == 0 and c[3] == 1)]
    assert len(cases) >= 4 * 5 * 7 and {(c[2], c[3]) for c in cases} == {(1, 0), (2, 0), (7, 0), (0, 1)}
    files, _lens, status, _outs, _r = _files(tq, [im for _n, im, _ri, _rows in cases],
                                             restart_interval=[c[2] for c in cases], restart_in_rows=[c[3] for c in cases])
    assert status == [0] * len(cases)
    dri = 0
    for (name, im, ri, rows), f in zip(cases, files):
        assert f == rst.write(im, ri, rows, optimize=True), name
        dri += b"\xff\xdd\x00\x04" in f[:f.index(b"\xff\xda")]
    assert dri == len(cases)


def _stop_images(lj9):
    """UPSAMPLE_UV inputs: 4:2:0 and 4:2:2 goldens as they are (stop 0) and with a planted range-check trip in the last
    component (stop 1), a grayscale and a 4:4:4 job between them"""
    ims = [lj9.read(GOLD / f"{s}.jpg") for s in ("gray64", "rgb141x93_420", "rgb128x96_420", "rgb141x93_444",
                                                 "rgb120x88_422_rst", "rgb141x93_420")]
    for k in (2, 4):
        im = ims[k]
        im["quants"][2] = im["quants"][2].copy()
        im["quants"][2][0] = max(int(im["quants"][2][0]), 3)
        im["coefs"][2] = im["coefs"][2].copy()
        im["coefs"][2][0, 0, 0] = 1000
    return ims


def _left_by_the_smoothing(im, coefs, res, stop):
    """the image dict of what the smoothing left: the replacement chroma at 1x1 when it stood, else the original"""
    host = [c.cpu().numpy() for c in coefs]
    if res["coef_up"] is not None and stop == 0:
        n = len(host)
        return dict(coefs=[host[0]] + [u.cpu().numpy() for u in res["coef_up"]], quants=res["quants"], hsamp=[1] * n,
                    vsamp=[1] * n, colorspace=im["colorspace"], image_size=im["image_size"])
    return dict(coefs=host, quants=res["quants"], hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"],
                image_size=im["image_size"])


def test_after_smoothing_both_stop_outcomes(tq, enc, rst, lj9):
    """UPSAMPLE_UV with both stop outcomes in one batch: the device picks variant 0 or 1 for the head, the mid and the
    scan alike; also with restart_in_rows, where the two variants have different DRI values"""
    ims = _stop_images(lj9)
    _devs, batch = _batch(ims)
    res = tq.quantsmooth_batch_(batch, pkg.flags_for_quality(6), 2)
    r = tq.encode_file_batch(batch, result=res)
    rr = tq.encode_file_batch(batch, result=res, restart_in_rows=1)
    torch.cuda.synchronize()
    stops = res["stop"].cpu().tolist()
    assert stops == [0, 0, 1, 0, 1, 0]
    assert res["images"][1]["coef_up"] is not None and res["images"][2]["coef_up"] is not None
    assert r["status"].cpu().tolist() == [0] * 6 == rr["status"].cpu().tolist()
    dri = {}
    for k, (im, b, ri) in enumerate(zip(ims, batch, res["images"])):
        left = _left_by_the_smoothing(im, b["coefs"], ri, stops[k])
        got = r["files"][k][:int(r["len"][k])].cpu().numpy().tobytes()
        assert got == enc.write(left, optimize=True), f"job {k} (stop {stops[k]})"
        got = rr["files"][k][:int(rr["len"][k])].cpu().numpy().tobytes()
        assert got == rst.write(left, 0, 1, optimize=True), f"job {k} (stop {stops[k]}) with restart_in_rows"
        dri[k] = jpeg_file.parse(got)["restart_interval"]
    # one MCU row of the variant taken: 141 wide at 1x1 after the replacement, 128 wide at 2x2 where the original stood
    assert dri[1] == 18 and dri[2] == 8


def _dht_bytes(f):
    return sum(len(p) + 4 for code, p in parse_jpeg(f)["markers"] if code == 0xC4)


def test_smooth_and_encode_files_in_one_captured_graph(tq, enc, lj9):
    """quantsmooth_batch_ -> encode_file_batch(optimize=True) captured once and replayed on three contents whose optimal
    tables have different sizes: the tables and the segment's position follow the data"""
    ims = _stop_images(lj9)[1:4]
    for im in ims:
        im["coefs"] = [c.copy() for c in im["coefs"]]
    ims[1]["coefs"][2][0, 0, 0] = int(lj9.read(GOLD / "rgb128x96_420.jpg")["coefs"][2][0, 0, 0])      # no trip to begin with
    flags = pkg.flags_for_quality(6)
    src = [[torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in im["coefs"]] for im in ims]
    work = [[t.clone() for t in s] for s in src]
    batch = [dict(coefs=w, quants=im["quants"], **_kw(im)) for w, im in zip(work, ims)]
    outs = [Guarded(200000) for _ in ims]
    ws1, ws2 = None, tq.Workspace()

    def step():
        for w, s in zip(work, src):
            for a, b in zip(w, s):
                a.copy_(b)
        res = tq.quantsmooth_batch_(batch, flags, 2, workspace=ws1)
        return res, tq.encode_file_batch(batch, result=res, outs=[o.view for o in outs], workspace=ws2)

    res, out = step()                                          # eager: prepares both workspaces, uploads the frames
    ws1 = res["workspace"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gres, gout = step()
    rng = np.random.default_rng(3)
    seen, dht = set(), set()
    for rep in range(3):
        for s, im in zip(src, ims):                            # new content: all of it, or fewer of its coefficients
            for t, c in zip(s, im["coefs"]):                       # (6 or 20 of a block's 64), the rest perturbed by one
                c = c.copy()
                if rep:
                    c[..., (6 if rep == 1 else 20):] = 0
                    c += rng.integers(-1, 2, c.shape).astype(np.int16) * (c != 0)
                t.copy_(torch.from_numpy(c))
        src[rep % 3][2].view(-1)[0] = 1000 if rep == 1 else int(ims[rep % 3]["coefs"][2].reshape(-1)[0])
        g.replay()
        torch.cuda.synchronize()
        glen, gstatus, gstop = gout["len"].cpu().tolist(), gout["status"].cpu().tolist(), gres["stop"].cpu().tolist()
        assert gstatus == [0, 0, 0]
        sizes = []
        for k, (im, o, l) in enumerate(zip(ims, outs, glen)):
            got = o.view[:l].cpu().numpy().tobytes()
            want = enc.write(_left_by_the_smoothing(im, work[k], gres["images"][k], gstop[k]), optimize=True)
            assert got == want, f"replay {rep}, image {k} (stop {gstop[k]})"
            o.check()
            sizes.append(_dht_bytes(got))
        dht.add(tuple(sizes))
        seen.add(tuple(gstop))
    assert len(seen) > 1                                       # the stop outcome changed across replays
    assert len(dht) == 3                                       # ... and so did the size of the tables


def test_capacities(tq, enc):
    """capacity L, L - 1, inside the head, inside a DHT marker and 1, on misaligned guarded buffers"""
    ims = [synth_scan_image(np.random.default_rng(77), (5, 3), [1], [1], 1),
           synth_scan_image(np.random.default_rng(1), (141, 93), [2, 1, 1], [2, 1, 1], 3)]
    want = [enc.write(im, optimize=True) for im in ims]
    for pick in (lambda w: len(w), lambda w: len(w) - 1, lambda w: 10, lambda w: w.index(b"\xff\xc4") + 10, lambda w: 1):
        caps = [pick(w) for w in want]
        devs, batch = _batch(ims)
        big = [Guarded(len(w) + 1000) for w in want]
        r = tq.encode_file_batch(batch, outs=[g.view[1:1 + c] for g, c in zip(big, caps)])
        torch.cuda.synchronize()
        assert r["len"].cpu().tolist() == [len(w) for w in want]
        assert r["status"].cpu().tolist() == [0 if c == len(w) else 2 for c, w in zip(caps, want)]
        for g, c, w in zip(big, caps, want):
            g.check(untouched_from=1 + c)
            assert int(g.view[0]) == 0xA5
            assert g.view[1:1 + c].cpu().numpy().tobytes() == w[:c]       # the part that fits, and nothing beyond it


def test_a_coefficient_out_of_range_in_one_job(tq, enc):
    ims = [synth_scan_image(np.random.default_rng(k), (40, 24), [1], [1], 1) for k in range(3)]
    ims[1]["coefs"][0][1, 2, 9] = 1024
    files, lens, status, _outs, _r = _files(tq, ims)
    assert status == [0, 1, 0] and lens[1] == 0
    assert files[0] == enc.write(ims[0], optimize=True) and files[2] == enc.write(ims[2], optimize=True)


def test_the_workspace_is_left_alone(tq, enc, corpus):
    """encode_scan_batch, encode_file_batch(optimize=True) and encode_scan_batch again on one workspace: the plain run's
    tables are still prepare's"""
    ims = [im for _n, im in corpus[:40:3]]
    _devs, batch = _batch(ims)
    a = tq.encode_scan_batch(batch)
    torch.cuda.synchronize()
    first = [s[:l].cpu().numpy().tobytes() for s, l in zip(a["segments"], a["len"].cpu().tolist())]
    before = a["workspace"].buf.data_ptr()
    f = tq.encode_file_batch(batch, workspace=a["workspace"])
    b = tq.encode_scan_batch(batch, workspace=a["workspace"])
    torch.cuda.synchronize()
    assert f["workspace"] is a["workspace"] and a["workspace"].buf.data_ptr() == before
    assert f["status"].cpu().tolist() == [0] * len(ims) == b["status"].cpu().tolist()
    third = [s[:l].cpu().numpy().tobytes() for s, l in zip(b["segments"], b["len"].cpu().tolist())]
    assert first == third
    for im, s in zip(ims, first):
        assert s == parse_jpeg(enc.write(im))["segment"]


def test_frameless_run(tq, enc):
    """frames = NULL: the optimized DHT markers followed by the segment, and nothing else"""
    ims = [synth_scan_image(np.random.default_rng(4), (67, 131), [1], [1], 1),
           synth_scan_image(np.random.default_rng(5), (141, 93), [2, 1, 1], [2, 1, 1], 3)]
    _devs, batch = _batch(ims)
    hip = pkg.HipQS()
    jobs, dev, _stop = tq._encode_jobs(batch, None, "test", torch)
    _per, ws = tq._encode_workspace(jobs, dev, None, b"", None, "test", torch)
    scratch = Guarded(hip.encode_files_scratch_bytes(2))
    assert scratch.view.data_ptr() % 256 == 0
    outs = [Guarded(100000) for _ in ims]
    length, status = torch.empty(2, dtype=torch.int64, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    hip.encode_batch_files(jobs, None, True, None, [o.view.data_ptr() for o in outs], [100000, 100000], length.data_ptr(),
                           status.data_ptr(), None, scratch.view.data_ptr(), int(scratch.view.numel()), ws.buf.data_ptr(),
                           ws.nbytes, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    scratch.check()
    assert status.cpu().tolist() == [0, 0]
    for im, o, l in zip(ims, outs, length.cpu().tolist()):
        w = enc.write(im, optimize=True)
        want = w[w.index(b"\xff\xc4"):w.index(b"\xff\xda")] + parse_jpeg(w)["segment"]
        assert l == len(want) and o.view[:l].cpu().numpy().tobytes() == want
        o.check(untouched_from=l)


def test_read_takes_the_device_file(tq):
    """file out, file in: read(encode_file(..., restart_interval=4)) on the device tensor of the file"""
    im = synth_scan_image(np.random.default_rng(9), (141, 93), [2, 1, 1], [2, 1, 1], 3)
    coefs = [torch.from_numpy(c).cuda() for c in im["coefs"]]
    r = tq.encode_file(coefs, im["quants"], **_kw(im), restart_interval=4)
    assert int(r["status"].item()) == 0
    back = tq.read(r["file"][:int(r["len"].item())])
    torch.cuda.synchronize()
    assert int(back["status"].item()) == 0 and back["restart_interval"] == 4
    assert back["image_size"] == tuple(im["image_size"]) and back["hsamp"] == list(im["hsamp"])
    for a, b in zip(back["coefs"], im["coefs"]):
        hb, wb = min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])
        assert np.array_equal(a.cpu().numpy()[:hb, :wb], b[:hb, :wb])
    for q, w in zip(back["quants"], im["quants"]):
        assert np.array_equal(np.asarray(q).reshape(64), np.asarray(w).reshape(64))
