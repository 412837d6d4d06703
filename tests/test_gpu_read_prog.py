"""The progressive route of the device scan reader on the GPU (qs_hip_read_prog_device_batch, torch_qs.read_progressive /
read_progressive_batch / read_batch): files written by libjpeg 9 (tests/libjpeg9_encode.c) against libjpeg 9's own
read of them (tests/libjpeg9_decode.c), the round trip through the device progressive coder, a captured graph, the
dispatch of read_batch, and the corrupt corpus of tests/test_read_prog_host.py against the host build of the same
csrc/qs_read_prog.h.  Every array, file, status buffer and workspace lies between sentinel margins."""
import numpy as np
import pytest

import jpegqs_pkg
from encode_oracle import synth_scan_image
from encode_prog_oracle import LibJpeg9EncProg
from encode_rst_oracle import LibJpeg9EncRst
from helpers import Guarded
from read_oracle import LibjpegReader
from read_prog_oracle import ReadProgHost, build_grid, corpus_sources, corrupt_corpus

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
jpeg_file = pkg.jpeg_file


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpureadprog")
    return LibJpeg9EncProg(d), LibjpegReader(d), d


@pytest.fixture(scope="module")
def grid(tools):
    enc, lj, _d = tools
    return build_grid(enc, lj)


@pytest.fixture(scope="module")
def tq():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible to torch")
    return pkg.torch_qs


def _kw(im):
    return dict(hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"], image_size=im["image_size"])


class Batch:
    """the cases' files, arrays, status and workspace on the device, each between margins; the C ABI called directly"""

    def __init__(self, cases):
        self.hip = pkg.HipQS()
        self.cases = cases
        self.files, self.arrs, self.jobs, self.opts = [], [], [], []
        for c in cases:
            p = c["header"]
            f = Guarded(max(1, len(c["data"])))
            f.view[:len(c["data"])].copy_(torch.frombuffer(bytearray(c["data"]), dtype=torch.uint8))
            self.files.append(f)
            a = [Guarded(rows * stride * 64, torch.int16) for rows, stride in c["shapes"]]
            self.arrs.append(a)
            self.jobs.append(self.hip.device_job([g.view.data_ptr() for g in a], c["shapes"], [None] * len(a), hsamp=p["hsamp"],
                                                 vsamp=p["vsamp"], colorspace=p["colorspace"] or 1, image_size=p["image_size"]))
            self.opts.append(self.hip.read_prog_opts(p["scans"]))
        self.per, total = self.hip.read_prog_batch_info(self.jobs, self.opts)
        self.ws = Guarded(total)
        self.status = Guarded(len(cases), torch.int32)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.hip.read_prog_batch_prepare(self.jobs, self.opts, self.ws.view.data_ptr(), total, self.stream)

    def fill(self, value):
        for a in self.arrs:
            for g in a:
                g.view.fill_(value)

    def run(self):
        """-> (status list, [[arrays (rows, stride, 64)] per case]); the margins and the files checked"""
        self.hip.read_prog_batch(self.jobs, [f.view.data_ptr() for f in self.files], [len(c["data"]) for c in self.cases],
                                 self.status.view.data_ptr(), self.ws.view.data_ptr(), self.ws.view.numel(), self.stream)
        torch.cuda.synchronize()
        self.ws.check()
        self.status.check()
        out = []
        for c, f, a in zip(self.cases, self.files, self.arrs):
            f.check()
            assert f.view[:len(c["data"])].cpu().numpy().tobytes() == c["data"], "the reader changed its input"
            for g in a:
                g.check()
            out.append([g.view.cpu().numpy().reshape(rows, stride, 64) for g, (rows, stride) in zip(a, c["shapes"])])
        return self.status.view.cpu().tolist(), out


def _assert_exact(cases, status, arrs):
    for c, s, a in zip(cases, status, arrs):
        assert s == 0, (c["name"], s)
        for ci, (got, want) in enumerate(zip(a, c["want"])):
            if not np.array_equal(got, want):
                bad = np.argwhere((got != want).any(axis=2))
                raise AssertionError(f"{c['name']}: component {ci}: {len(bad)} blocks differ, first at {tuple(bad[0])}")


def test_grid_in_one_batch_and_again_over_stale_arrays(grid):
    """the whole grid of tests/test_read_prog_host.py in one batch of many launch chunks -- scans of all four kinds, the
    crafted refinement images, pairs of more than 64 intervals -- against libjpeg's arrays, the dummy blocks' rule and the
    zeros outside included; the inputs unchanged; then once more into the same arrays filled with 0x5a5a"""
    assert len(grid) > 3 * 32
    b = Batch(grid)
    assert max(max(p["intervals"]) for p in b.per) > 64                 # more than one decode workgroup in a pair
    assert {p["levels"] for p in b.per} >= {1, 3}
    _assert_exact(grid, *b.run())
    b.fill(0x5a5a)
    _assert_exact(grid, *b.run())


def test_corrupt_corpus_reports_what_the_host_build_reports(tools, grid):
    """the corrupt corpus of tests/test_read_prog_host.py (green there, for the same qs_read_prog.h, before this runs
    anywhere), with valid jobs between the corrupt ones: the statuses of the host build file by file and its arrays where
    the status is 0, every margin intact, the valid jobs still exact"""
    enc, lj, d = tools
    corpus = corrupt_corpus(corpus_sources(enc, lj))
    host = ReadProgHost(d).run(corpus)
    assert all(0 <= s <= 3 for s, _l, _a in host) and {0, 1, 2, 3} <= {s for s, _l, _a in host}
    valid = grid[5::9]
    for lo in range(0, len(corpus), 1200):
        cases, ref = [], []
        for k in range(lo, min(len(corpus), lo + 1200)):
            if k % 40 == 0:
                cases.append(valid[(k // 40) % len(valid)])
                ref.append(None)
            cases.append(corpus[k])
            ref.append(host[k])
        status, arrs = Batch(cases).run()
        for c, s, a, r in zip(cases, status, arrs, ref):
            if r is None:
                _assert_exact([c], [s], [a])
                continue
            assert s == r[0], (c["name"], s, r[0])
            if s == 0:
                for got, want in zip(a, r[2]):
                    assert np.array_equal(got, want), c["name"]


def _upload(im):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in im["coefs"]]


def test_round_trip_with_the_device_progressive_coder(tq, tools):
    """encode_file(scans=simple_progression, refinement=True, restart_interval=7) then read_progressive gives the original
    arrays; read of libjpeg's file with that script and interval, then encode_file with the returned script, gives the
    bytes of libjpeg's file"""
    enc, _lj, _d = tools
    rng = np.random.default_rng(78)
    for size, hs, vs in (((33, 18), [2, 1, 1], [2, 1, 1]), ((141, 93), [1, 1, 1], [1, 1, 1])):
        im = synth_scan_image(rng, size, hs, vs, 3)
        script = jpeg_file.simple_progression(3, 3)
        r = tq.encode_file(_upload(im), im["quants"], **_kw(im), scans=script, refinement=True, restart_interval=7)
        torch.cuda.synchronize()
        assert int(r["status"][0]) == 0
        data = r["file"][:int(r["len"][0])]
        for src in (data, data.cpu().numpy().tobytes()):
            got = tq.read_progressive(src)
            assert int(got["status"]) == 0 and got["scans"] == script and got["restart_interval"] == 7 and got["huffman"] is None
            assert got["image_size"] == tuple(size) and got["hsamp"] == hs and got["colorspace"] == 3
            for a, b, q, qw in zip(got["coefs"], im["coefs"], got["quants"], im["quants"]):
                assert np.array_equal(a.cpu().numpy(), b), size
                assert np.array_equal(q, qw)
        f = enc.write(im, script, 7, 0)
        got = tq.read(f)
        assert int(got["status"]) == 0
        again = tq.encode_file(got["coefs"], got["quants"], **_kw(got), scans=got["scans"], refinement=True, restart_interval=7)
        torch.cuda.synchronize()
        assert int(again["status"][0]) == 0 and again["file"][:int(again["len"][0])].cpu().numpy().tobytes() == f


def test_captured_graph_replays_on_other_files_and_notices_moved_scans(tq, tools):
    """read_progressive_batch on two device-resident files captured in a graph: replayed over scrambled arrays, with
    other files of the same header layout in the same tensors, and with a file whose second scan is one byte longer"""
    enc, lj, _d = tools
    script = jpeg_file.simple_progression(3, 3)
    sizes = [((33, 18), [2, 1, 1], [2, 1, 1]), ((64, 48), [1, 1, 1], [1, 1, 1])]

    def layout(f):
        p = jpeg_file.parse_progressive(f)
        return [(s["offset"], s["length"]) for s in p["scans"]]
    # a variant of each image with the same header layout -- the same scan offsets and lengths: the signs of one block's AC
    # coefficients flipped change neither a symbol nor a code length, only (rarely) the number of stuffed FF bytes
    files = [[], []]
    for k, (size, hs, vs) in enumerate(sizes):
        im = synth_scan_image(np.random.default_rng(300 + k), size, hs, vs, 3)
        a = enc.write(im, script, 1, 0)
        for t in range(im["coefs"][0].shape[1]):
            other = dict(im, coefs=[c.copy() for c in im["coefs"]])
            other["coefs"][0][0, t, 1:] = -other["coefs"][0][0, t, 1:]
            b = enc.write(other, script, 1, 0)
            if a != b and layout(a) == layout(b):
                break
        assert a != b and layout(a) == layout(b) and len(a) == len(b)
        files[0].append(a)
        files[1].append(b)
    want = []
    for row in files:
        got = []
        for f in row:
            ref, clean = lj.read_bytes(f)
            assert clean
            got.append(ref["coefs"])
        want.append(got)
    bufs = [Guarded(len(f) + 64) for f in files[0]]

    def load(row):
        for b, f in zip(bufs, row):
            b.view.zero_()
            b.view[:len(f)].copy_(torch.frombuffer(bytearray(f), dtype=torch.uint8))

    load(files[0])
    r = tq.read_progressive_batch([b.view for b in bufs])               # eager: prepares the workspace
    torch.cuda.synchronize()
    assert r["status"].cpu().tolist() == [0, 0]
    shapes = [[tuple(t.shape) for t in im["coefs"]] for im in r["images"]]
    outs = [[Guarded(int(np.prod(s)), torch.int16) for s in sh] for sh in shapes]
    views = [[g.view.view(s) for g, s in zip(gs, sh)] for gs, sh in zip(outs, shapes)]
    r = tq.read_progressive_batch([b.view for b in bufs], outs=views, workspace=r["workspace"])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gr = tq.read_progressive_batch([b.view for b in bufs], outs=views, workspace=r["workspace"])

    def check(status, arrays):
        torch.cuda.synchronize()
        for b in bufs:
            b.check()
        for gs in outs:
            for x in gs:
                x.check()
        assert gr["status"].cpu().tolist() == status
        for k, w in enumerate(arrays or []):
            for t, a in zip(views[k], w):
                assert np.array_equal(t.cpu().numpy(), a), k

    for v in (0, 1):
        load(files[v])
        for vs in views:
            for t in vs:
                t.fill_(0x5a5a)
        g.replay()
        check([0, 0], want[v])
    # the second scan one byte longer: every later scan starts a byte behind its prepared offset
    f = files[0][0]
    s1 = jpeg_file.parse_progressive(f)["scans"][1]
    end = s1["offset"] + s1["length"]
    longer = f[:end] + b"\x00" + f[end:]
    load([longer, files[0][1]])
    g.replay()
    torch.cuda.synchronize()
    st = gr["status"].cpu().tolist()
    assert st[0] != 0 and st[1] == 0, st
    check(st, None)


def test_read_batch_hands_progressive_batches_over(tq, tools):
    enc, lj, d = tools
    rng = np.random.default_rng(79)
    im = synth_scan_image(rng, (33, 18), [2, 1, 1], [2, 1, 1], 3)
    gray = synth_scan_image(rng, (24, 16), [1], [1], 1)
    progs = [enc.write(im, jpeg_file.simple_progression(3, 3), 7, 0), enc.write(gray, jpeg_file.simple_progression(1, 1), 0, 1)]
    base = LibJpeg9EncRst(d).write(im, 7, 0, False)
    a, b = tq.read_batch(progs), tq.read_progressive_batch(progs)
    torch.cuda.synchronize()
    assert a["status"].cpu().tolist() == b["status"].cpu().tolist() == [0, 0]
    for x, y, f in zip(a["images"], b["images"], progs):
        ref, _clean = lj.read_bytes(f)
        assert x["scans"] == y["scans"] and x["restart_interval"] == y["restart_interval"]
        for t, u, w in zip(x["coefs"], y["coefs"], ref["coefs"]):
            assert np.array_equal(t.cpu().numpy(), w) and np.array_equal(u.cpu().numpy(), w)
    dev = torch.frombuffer(bytearray(progs[0]), dtype=torch.uint8).cuda()
    assert int(tq.read(dev)["status"]) == 0
    with pytest.raises(ValueError, match="file 1 is sequential"):
        tq.read_batch([progs[0], base])
    with pytest.raises(ValueError, match="file 1 is progressive"):
        tq.read_batch([base, progs[0]])
    with pytest.raises(ValueError, match="split=True"):
        tq.read_batch(progs, split=True)
    with pytest.raises(ValueError, match="SOF0"):
        tq.read_progressive(base)
    # a baseline file through read_batch: the arrays it gave before this route existed -- libjpeg's
    got = tq.read_batch([base])["images"][0]
    ref, _clean = lj.read_bytes(base)
    assert int(got["status"]) == 0 and "scans" not in got and got["huffman"] is not None
    for t, w in zip(got["coefs"], ref["coefs"]):
        assert np.array_equal(t.cpu().numpy(), w)
