"""The whole-file coder (torch_qs.encode_file_batch, qs_hip_encode_device_batch_files) on scans whose optimal tables pass
16 and 32 bits: the arrays of tests/crafted_scans.py, whose AC histograms give Huffman trees of 17, 22 and 32 levels --
figure K.3 cuts those back inside the table kernel, and libjpeg 9 itself writes the expected files -- and of 33, where
libjpeg stops with JERR_HUFF_CLEN_OVERFLOW and the run reports status 5.  Every depth named here is asserted on the
realised histogram by huff_oracle.code_sizes (the `deep` fixture), never taken from the code under test."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import jpegqs_pkg
from crafted_scans import ac_histogram, dc_histogram, shared_deep_image
from encode_oracle import LAYOUTS, LibJpeg9Enc, LibjpegError, parse_jpeg, synth_scan_image
from encode_rst_oracle import LibJpeg9EncRst, parse_rst
from helpers import Guarded
from huff_oracle import code_sizes, libjpeg_optimal

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TABLE = 273                                                           # bytes of a qs_hip_huff_table: bits[17], huffval[256]


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    return LibJpeg9Enc(tmp_path_factory.mktemp("lj9enc"))


@pytest.fixture(scope="module")
def rst(tmp_path_factory):
    return LibJpeg9EncRst(tmp_path_factory.mktemp("lj9rst"))


@pytest.fixture(scope="module")
def tq():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible to torch")
    return pkg.torch_qs


@pytest.fixture(scope="module")
def deep():
    """{name: (im, hist: the realised histogram of the deep AC table, depth, table: its index)}: gray at 17, 22, 32, 33;
    the three-component form (AC 1 deep) at 20 and 33"""
    out = {}
    for name, depth, ycc in (("g17", 17, False), ("g22", 22, False), ("y20", 20, True), ("g32", 32, False),
                             ("g33", 33, False), ("y33", 33, True)):
        im = shared_deep_image(depth, ycc)
        h = ac_histogram(im, (1, 2) if ycc else (0,))
        assert max(code_sizes(h)) == depth, name
        out[name] = SimpleNamespace(im=im, hist=h, depth=depth, table=1 if ycc else 0)
    return out


def _tiny(k):
    """ordinary small images, every layout in turn"""
    hs, vs, cs = LAYOUTS[k % len(LAYOUTS)]
    return synth_scan_image(np.random.default_rng(900 + k), [(5, 3), (33, 9), (16, 16), (40, 24)][k % 4], hs, vs, cs)


@pytest.fixture(scope="module")
def written(enc, deep):
    """libjpeg's optimized file of the arrays it accepts, written once; it refuses the others"""
    for name in ("g33", "y33"):
        with pytest.raises(LibjpegError):
            enc.write(deep[name].im, optimize=True)
    return {name: enc.write(deep[name].im, optimize=True) for name in ("g17", "g22", "y20", "g32")}


def _tensor(a):
    """the host tensor over a numpy array, read-only ones included (the shared arrays are; they are only read here)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return torch.from_numpy(np.ascontiguousarray(a))


def _dev(im):
    """the arrays on the device, each between margins"""
    out = []
    for c in im["coefs"]:
        g = Guarded(c.size, torch.int16)
        g.view.copy_(_tensor(c).reshape(-1))
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


def _capacity(im):
    return 8192 + 72 * sum(c.shape[0] * c.shape[1] for c in im["coefs"])


def _files(tq, ims, caps=None, room=0, **kw):
    """encode_file_batch with every output between margins and one byte off any alignment; `room`: bytes behind the
    capacity, which must stay as they were -> (files as bytes or None, len, status, guards, the call's result)"""
    devs, batch = _batch(ims)
    if caps is None:
        caps = [_capacity(im) for im in ims]
    outs = [Guarded(1 + c + room) for c in caps]
    r = tq.encode_file_batch(batch, outs=[o.view[1:1 + c] for o, c in zip(outs, caps)], **kw)
    torch.cuda.synchronize()
    lens, status = r["len"].cpu().tolist(), r["status"].cpu().tolist()
    for o, c in zip(outs, caps):
        o.check(untouched_from=1 + c)
        assert int(o.view[0]) == 0xA5, "the byte in front of the buffer changed"
    _check_inputs(devs, ims)
    files = [o.view[1:1 + l].cpu().numpy().tobytes() if s == 0 else None for o, l, s in zip(outs, lens, status)]
    return files, lens, status, outs, r


def _same_tables(tq, record, f, name):
    h = tq.huffman_of_tables(record)
    assert {t: (list(b), list(v)) for t, (b, v) in f["dc"].items()} == h["dc"], name
    assert {t: (list(b), list(v)) for t, (b, v) in f["ac"].items()} == h["ac"], name


def test_cut_back_files_equal_libjpeg(tq, enc, deep, written):
    """depth 17, 22, a tiny image, depth 32 and the three-component form at 20 in one batch: the cut-back of figure K.3
    runs inside the table kernel, and the code words, the DHT markers and the segment's place follow its result"""
    names = ["g17", "g22", None, "g32", "y20"]
    ims = [_tiny(0) if n is None else deep[n].im for n in names]
    want = [enc.write(ims[2], optimize=True) if n is None else written[n] for n in names]
    files, lens, status, _outs, r = _files(tq, ims)
    assert status == [0] * 5
    for k, (n, f, w, l) in enumerate(zip(names, files, want, lens)):
        assert l == len(w) and f == w, n
        p = parse_jpeg(w)
        _same_tables(tq, r["tables"][k], p, n)
        if n is not None:
            d = deep[n]
            assert max(code_sizes(d.hist)) == d.depth > 16 and p["ac"][d.table][0][16] > 0, n
            assert (list(p["ac"][d.table][0]), list(p["ac"][d.table][1])) == libjpeg_optimal(d.hist), n


def test_cut_back_with_restart_intervals_and_read_back(tq, rst, deep):
    """depth 22 with restart_interval = 7 (the AC counts are those of the plain scan), then the device reader on the
    device file"""
    d = deep["g22"]
    w = rst.write(d.im, 7, 0, optimize=True)
    p = parse_rst(w)
    assert p["dri"] == 7 and p["ac"][0][0][16] > 0 and (list(p["ac"][0][0]), list(p["ac"][0][1])) == libjpeg_optimal(d.hist)
    files, lens, status, outs, r = _files(tq, [d.im], restart_interval=7)
    assert status == [0] and lens == [len(w)] and files[0] == w
    _same_tables(tq, r["tables"][0], p, "g22 with restarts")
    back = tq.read(outs[0].view[1:1 + lens[0]].clone())
    torch.cuda.synchronize()
    assert int(back["status"].item()) == 0 and back["restart_interval"] == 7
    assert back["image_size"] == tuple(d.im["image_size"])
    a, b = back["coefs"][0].cpu().numpy(), d.im["coefs"][0]
    assert a.shape[0] >= b.shape[0] and a.shape[1] >= b.shape[1]
    assert np.array_equal(a[:b.shape[0], :b.shape[1]], b)


def test_histogram_under_contention(tq, deep):
    """a few symbols with millions of counts each: the most contended case the counting kernel's atomics can meet"""
    ims = [deep["g32"].im, deep["g33"].im]
    devs, batch = _batch(ims)
    r = tq.encode_histogram_batch(batch)
    torch.cuda.synchronize()
    got = r["counts"].cpu().numpy().view(np.uint32).astype(np.int64)
    assert r["status"].cpu().tolist() == [0, 0]
    for n, h in zip(("g32", "g33"), got):
        assert np.array_equal(h[2, :256], deep[n].hist) and h[2, :256].max() > 3_000_000, n
        assert np.array_equal(h[0, :16], dc_histogram(deep[n].im)) and not h[0, 16:256].any(), n
        assert not h[1, :256].any() and not h[3, :256].any(), n
        assert (h[:, 256] == 1).all(), n
    _check_inputs(devs, ims)


def _zero_table(record, w):
    """table w (DC 0, DC 1, AC 0, AC 1) of a qs_hip_huff_tables record: in use, bits and huffval all zero"""
    rec = record.cpu().numpy()
    return rec[4 * TABLE + w] == 1 and not rec[w * TABLE:(w + 1) * TABLE].any()


def test_status_5_and_its_neighbours(tq, enc, deep):
    """34 jobs (the launch chunk of 32 is crossed): depth 33 at 0 and 33, its three-component form at 31, ordinary
    images around them.  The failed jobs report 5 and no length and write nothing outside their buffers (the header
    promises nothing about the inside); every other job gets libjpeg's file"""
    bad = {0: "g33", 31: "y33", 33: "g33"}
    ims = [deep[bad[k]].im if k in bad else _tiny(k) for k in range(34)]
    files, lens, status, _outs, r = _files(tq, ims)
    assert status == [5 if k in bad else 0 for k in range(34)]
    for k, im in enumerate(ims):
        if k in bad:
            d = deep[bad[k]]
            assert lens[k] == 0 and files[k] is None
            assert _zero_table(r["tables"][k], 2 + d.table), f"job {k}"
            # the job's other tables are libjpeg's procedure on their counts (libjpeg itself writes no file to compare)
            h = tq.huffman_of_tables(r["tables"][k])
            comps = [c for c in range(len(im["coefs"])) if (c > 0) == bool(d.table)]
            assert h["dc"][d.table] == libjpeg_optimal(np.pad(dc_histogram(im, comps), (0, 240))), f"job {k}"
            assert h["ac"][d.table] == ([0] * 17, [])
            if d.table:
                assert h["ac"][0] == libjpeg_optimal(ac_histogram(im, (0,))), f"job {k}"
                assert h["dc"][0] == libjpeg_optimal(np.pad(dc_histogram(im, (0,)), (0, 240))), f"job {k}"
        else:
            w = enc.write(im, optimize=True)
            assert lens[k] == len(w) and files[k] == w, f"job {k}"
            _same_tables(tq, r["tables"][k], parse_jpeg(w), f"job {k}")


def _planted(im):
    """the gray image with 1024, in its sign, over its first AC value of 10 bits -> (image, the array as the device
    counts it).  The coder refuses the value and goes on with it clamped to 10 bits (jchuff.c stops instead), so the
    symbol counted is the one the scan had: the realised histogram, and with it the depth, is the unplanted one"""
    c = im["coefs"][0].copy()
    flat = c.reshape(-1, 64)
    big = np.abs(flat[:, 1:].astype(np.int32)) >= 512
    b = int(np.flatnonzero(big.any(axis=1))[0])
    k = 1 + int(np.flatnonzero(big[b])[0])
    assert 512 <= abs(int(flat[b, k])) <= 1023
    flat[b, k] = 1024 if flat[b, k] > 0 else -1024
    counted = c.copy()
    counted[..., 1:] = np.clip(counted[..., 1:], -1023, 1023)
    assert (counted != c).sum() == 1
    return dict(im, coefs=[c]), counted


def test_precedence_1_5_2(tq, deep, written):
    """a refused coefficient wins over the table's overflow: the planted depth-33 job's histogram, as the device counts
    it, still has depth 33, so its table status is set and status 1 has to win over it; the same plant at depth 32 is
    plain status 1.  The overflow wins over a short buffer (len 0, nothing behind the capacity); a short buffer on a
    cut-back table gives 2 with the exact length and the file's first bytes"""
    p33, counted33 = _planted(deep["g33"].im)
    p32, counted32 = _planted(deep["g32"].im)
    for counted, d in ((counted33, deep["g33"]), (counted32, deep["g32"])):
        h = ac_histogram(dict(coefs=[counted]))
        assert np.array_equal(h, d.hist) and max(code_sizes(h)) == d.depth
    w = written["g32"]
    ims = [p33, deep["g33"].im, deep["g32"].im, p32]
    files, lens, status, outs, r = _files(tq, ims, caps=[_capacity(p33), 10, len(w) - 1, _capacity(p32)], room=1000)
    assert status == [1, 5, 2, 1] and lens == [0, 0, len(w), 0]
    assert outs[2].view[1:len(w)].cpu().numpy().tobytes() == w[:-1]
    # the table kernel did meet the overflow on the planted job: its AC table is the zeroed one of status 5
    assert _zero_table(r["tables"][0], 2) and _zero_table(r["tables"][1], 2)
    assert tq.huffman_of_tables(r["tables"][3])["ac"][0] == libjpeg_optimal(deep["g32"].hist)


def test_status_4_on_a_workspace_the_run_does_not_know(tq, deep):
    """the status-5 image as a restart job: 5 on the workspace prepare saw, 4 (and no length) on a copy of it elsewhere.
    The library knows workspaces by address and the allocator hands freed blocks out again, so the copy sits 256 bytes
    into a block of its own: torch's blocks start at multiples of 512, and no workspace was ever prepared there"""
    im = deep["g33"].im
    devs, batch = _batch([im])
    first = tq.encode_file_batch(batch, restart_interval=7)
    torch.cuda.synchronize()
    assert first["status"].cpu().tolist() == [5] and first["len"].cpu().tolist() == [0]
    ws = first["workspace"]
    out = Guarded(_capacity(im))
    block = torch.empty(ws.nbytes + 512, dtype=torch.uint8, device=ws.buf.device)
    copy = block[256:256 + ws.nbytes]
    copy.copy_(ws.buf)
    assert copy.data_ptr() % 512 == 256
    moved = tq.encode_file_batch(batch, outs=[out.view], workspace=tq.Workspace(buf=copy, key=ws.key), restart_interval=7)
    torch.cuda.synchronize()
    assert moved["status"].cpu().tolist() == [4] and moved["len"].cpu().tolist() == [0]
    out.check()
    _check_inputs(devs, [im])


def test_graph_replay_across_the_limit(tq, enc, deep):
    """encode_file_batch(optimize=True) captured once on arrays of the depth-33 geometry and a small neighbour, replayed
    on depth 33 (5), the depth-32 blocks with the rest of the array zero (0: libjpeg's file of exactly those arrays; the
    extra blocks' EOBs move the depth, which is asserted to stay in 17 .. 32), depth 33 again (5), ordinary content (0):
    no table status, prefix or length survives a replay"""
    im33 = deep["g33"].im
    shape = im33["coefs"][0].shape
    nblk = shape[0] * shape[1]

    def spread(blocks):
        a = np.zeros((nblk, 64), np.int16)
        a[:blocks.size // 64] = blocks.reshape(-1, 64)
        return a.reshape(shape)

    rng = np.random.default_rng(5)
    contents = [im33["coefs"][0], spread(deep["g32"].im["coefs"][0]), im33["coefs"][0],
                spread(synth_scan_image(rng, (8 * 61, 8 * 37), [1], [1], 1)["coefs"][0])]
    depths = [max(code_sizes(ac_histogram(dict(coefs=[c])))) for c in contents]
    assert depths[0] == depths[2] == 33 and 17 <= depths[1] <= 32 and depths[3] <= 32
    near = [synth_scan_image(rng, (67, 35), [2, 1, 1], [2, 1, 1], 3) for _ in contents]
    near = [dict(near[0], coefs=n["coefs"]) for n in near]            # one geometry and one set of quants
    want = [None if d > 32 else enc.write(dict(im33, coefs=[c]), optimize=True) for c, d in zip(contents, depths)]
    want_near = [enc.write(n, optimize=True) for n in near]
    assert want[1] != want[3] and len(set(want_near)) == len(near)

    ims = [dict(im33, coefs=[contents[3]]), near[3]]                 # the eager run: ordinary content
    devs, batch = _batch(ims)
    outs = [Guarded(_capacity(im)) for im in ims]
    first = tq.encode_file_batch(batch, outs=[o.view for o in outs])
    torch.cuda.synchronize()
    assert first["status"].cpu().tolist() == [0, 0]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = tq.encode_file_batch(batch, outs=[o.view for o in outs], workspace=first["workspace"])
    for rep, (c, n) in enumerate(zip(contents, near)):
        devs[0][0][1].copy_(_tensor(c))
        for (_g, t), a in zip(devs[1], n["coefs"]):
            t.copy_(_tensor(a))
        g.replay()
        torch.cuda.synchronize()
        lens, status = out["len"].cpu().tolist(), out["status"].cpu().tolist()
        for o in outs:
            o.check()
        assert status == [5 if want[rep] is None else 0, 0], f"replay {rep}"
        assert lens == [0 if want[rep] is None else len(want[rep]), len(want_near[rep])], f"replay {rep}"
        if want[rep] is not None:
            assert outs[0].view[:lens[0]].cpu().numpy().tobytes() == want[rep], f"replay {rep}"
            _same_tables(tq, out["tables"][0], parse_jpeg(want[rep]), f"replay {rep}")
        else:
            assert _zero_table(out["tables"][0], 2), f"replay {rep}"
        assert outs[1].view[:lens[1]].cpu().numpy().tobytes() == want_near[rep], f"replay {rep}: the neighbour"
        _check_inputs(devs, [dict(coefs=[c]), n])


def test_host_route(tq, deep, written):
    """encode_batch(optimize=True): the histogram on the device, qs_hip_huff_optimal on the host.  Depth 32 is libjpeg's
    file; at depth 33 the call raises what HipQS.huff_optimal raises -- hipqs.QsHipError with code -2 (QS_HIP_EINVAL), a
    RuntimeError: torch_qs.encode_batch calls it per table and lets the error pass, where the device route reports
    status 5"""
    devs, batch = _batch([deep["g32"].im, deep["g33"].im])
    assert tq.encode_batch(batch[:1], optimize=True) == [written["g32"]]
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        tq.encode_batch(batch[1:], optimize=True)
    assert e.value.code == -2 and isinstance(e.value, RuntimeError) and not isinstance(e.value, ValueError)
    with pytest.raises(pkg.hipqs.QsHipError):
        tq.encode_batch(batch, optimize=True)                         # one such image stops the batch
    _check_inputs(devs, [deep["g32"].im, deep["g33"].im])
