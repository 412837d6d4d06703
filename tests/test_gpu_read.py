"""The device scan reader on the GPU (qs_hip_read_device_batch, torch_qs.read / read_batch): files written by libjpeg 9
(tests/libjpeg9_encode.c) against libjpeg 9's own read of them (tests/libjpeg9_decode.c), the round trip through the
device entropy coder, a captured graph, and the corrupt corpus of tests/test_read_host.py against the host build of the
same csrc/qs_read.h.  Every array, file, status buffer and workspace lies between sentinel margins."""
import numpy as np
import pytest

import jpegqs_pkg
from encode_oracle import synth_scan_image
from encode_rst_oracle import LibJpeg9EncRst, parse_rst
from helpers import Guarded
from read_oracle import LibjpegReader, ReadHost, build_grid, corpus_sources, corrupt_corpus

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
jpeg_file = pkg.jpeg_file


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpuread")
    return LibJpeg9EncRst(d), LibjpegReader(d), d


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
            f = Guarded(len(c["data"]))
            f.view.copy_(torch.frombuffer(bytearray(c["data"]), dtype=torch.uint8))
            self.files.append(f)
            a = [Guarded(rows * stride * 64, torch.int16) for rows, stride in c["shapes"]]
            self.arrs.append(a)
            self.jobs.append(self.hip.device_job([g.view.data_ptr() for g in a], c["shapes"], [None] * len(a), hsamp=p["hsamp"],
                                                 vsamp=p["vsamp"], colorspace=p["colorspace"], image_size=p["image_size"]))
            self.opts.append(self.hip.read_opts(p["dc"], p["ac"], p["dc_tbl"], p["ac_tbl"], p["restart_interval"]))
        self.per, total = self.hip.read_batch_info(self.jobs, self.opts)
        self.ws = Guarded(total)
        self.status = Guarded(len(cases), torch.int32)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.hip.read_batch_prepare(self.jobs, self.opts, self.ws.view.data_ptr(), total, self.stream)

    def fill(self, value):
        for a in self.arrs:
            for g in a:
                g.view.fill_(value)

    def run(self):
        """-> (status list, [[arrays (rows, stride, 64)] per case]); the margins and the files checked"""
        offs = [c["header"]["scan_offset"] for c in self.cases]
        self.hip.read_batch(self.jobs, [f.view.data_ptr() + o for f, o in zip(self.files, offs)],
                            [len(c["data"]) - o for c, o in zip(self.cases, offs)], self.status.view.data_ptr(),
                            self.ws.view.data_ptr(), self.ws.view.numel(), self.stream)
        torch.cuda.synchronize()
        self.ws.check()
        self.status.check()
        out = []
        for c, f, a in zip(self.cases, self.files, self.arrs):
            f.check()
            assert f.view.cpu().numpy().tobytes() == c["data"], "the reader changed its input"
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
    """the whole grid of tests/test_read_host.py in one batch of many launch chunks against libjpeg's arrays, dummy
    blocks and the zeros outside included; the inputs unchanged; then once more into the same arrays filled with 0x5a5a"""
    assert len(grid) > 3 * 32
    b = Batch(grid)
    assert [p["intervals"] for p in b.per][:3] and max(p["intervals"] for p in b.per) > 64     # more than one decode workgroup
    _assert_exact(grid, *b.run())
    b.fill(0x5a5a)
    _assert_exact(grid, *b.run())


def test_interval_cap_is_refused_before_anything_runs(grid):
    hip = pkg.HipQS()
    sentinel = Guarded(200 * 200 * 64, torch.int16)
    p = grid[0]["header"]
    assert p["hsamp"] == [1]

    def job(w, h):
        return hip.device_job([sentinel.view.data_ptr()], [(h, w)], [None], hsamp=[1], vsamp=[1], colorspace=1,
                              image_size=(8 * w, 8 * h))
    opts = hip.read_opts(p["dc"], p["ac"], [0], [0], 0)
    per, _ = hip.read_batch_info([job(128, 256)], [opts])                      # exactly the cap: one lane, accepted
    assert per[0]["intervals"] == 1 and per[0]["blocks_per_interval"] == 32768
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.read_batch_info([job(200, 200)], [opts])
    assert e.value.code == -4
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.read_batch_prepare([job(200, 200)], [opts], sentinel.view.data_ptr(), sentinel.view.numel() * 2, None)
    assert e.value.code == -4
    per, _ = hip.read_batch_info([job(200, 200)], [hip.read_opts(p["dc"], p["ac"], [0], [0], 200)])
    assert per[0]["intervals"] == 200
    torch.cuda.synchronize()
    sentinel.check()
    assert (sentinel.view.cpu().numpy().view(np.uint16) == 0xA5A5).all()


def _upload(im):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in im["coefs"]]


def test_round_trip_with_the_device_coder(tq, tools):
    """encode(restart_interval=r) then read gives the original arrays; read then encode with the returned tables and
    interval gives the file's own scan bytes"""
    enc, lj, _d = tools
    rng = np.random.default_rng(77)
    ims = [synth_scan_image(rng, (141, 93), [2, 1, 1], [2, 1, 1], 3), synth_scan_image(rng, (67, 131), [1], [1], 1),
           synth_scan_image(rng, (33, 9), [1, 1, 1, 1], [1, 1, 1, 1], 4)]
    for im in ims:
        dev = _upload(im)
        for kw in (dict(restart_interval=1), dict(restart_interval=7), dict(restart_in_rows=1)):
            data = tq.encode(dev, im["quants"], **_kw(im), **kw)
            for src in (data, torch.frombuffer(bytearray(data), dtype=torch.uint8), torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()):
                got = tq.read(src)
                assert int(got["status"]) == 0, kw
                assert got["image_size"] == tuple(im["image_size"]) and got["hsamp"] == im["hsamp"] and got["colorspace"] == im["colorspace"]
                for a, b, q, qw in zip(got["coefs"], im["coefs"], got["quants"], im["quants"]):
                    assert np.array_equal(a.cpu().numpy(), b), kw
                    assert np.array_equal(q, qw)
        for ri, opt in ((3, False), (5, True)):
            data = enc.write(im, ri, 0, opt)                            # libjpeg's file, optimized tables in one
            got = tq.read(data)
            assert int(got["status"]) == 0 and got["restart_interval"] == ri and got["huffman"] is not None
            seg = tq.encode_scan(got["coefs"], **_kw(got), huffman=got["huffman"], restart_interval=got["restart_interval"])
            assert int(seg["status"]) == 0
            assert seg["segment"][:int(seg["len"])].cpu().numpy().tobytes() == parse_rst(data)["segment"]
            again = tq.encode(got["coefs"], got["quants"], **_kw(got), huffman=got["huffman"],
                              restart_interval=got["restart_interval"])
            assert again == data


def test_read_smooth_and_encode_in_one_captured_graph(tq, tools):
    """read_batch, quantsmooth_batch_ and encode_scan_batch captured in one graph and replayed with other file bytes of
    the same header in the same device buffers: the eager result of each file"""
    enc, _lj, _d = tools
    sizes = [(141, 93), (64, 48)]
    files = []                                                          # files[v][k]: variant v of image k
    for v in range(3):
        row = []
        for k, (w, h) in enumerate(sizes):
            y = pkg.synth.synth_ycc(w, h, 2, 2, quality=50, seed=100 + 10 * v + k)     # natural statistics: no range-check stop
            row.append(enc.write(dict(coefs=y["coefs"], quants=y["quants"], hsamp=y["hsamp"], vsamp=y["vsamp"], colorspace=3,
                                      image_size=(w, h)), 4, 0))
        files.append(row)
    heads = [[f[:jpeg_file.parse(f)["scan_offset"]] for f in row] for row in files]
    assert heads[0] == heads[1] == heads[2]
    flags = pkg.flags_for_quality(3)

    def eager(row):
        r = tq.read_batch(row)
        res = tq.quantsmooth_batch_(r["images"], flags, 1)
        out = tq.encode_scan_batch(r["images"], result=res, restart_interval=4)
        torch.cuda.synchronize()
        assert r["status"].cpu().tolist() == [0, 0] and out["status"].cpu().tolist() == [0, 0]
        return [s[:int(l)].cpu().numpy().tobytes() for s, l in zip(out["segments"], out["len"].cpu().tolist())]

    want = [eager(row) for row in files]
    assert want[1] != want[2]
    cap = max(len(f) for row in files for f in row) + 64
    bufs = [Guarded(cap) for _ in sizes]
    outs = [Guarded(100000) for _ in sizes]
    ws = [tq.Workspace(), None, tq.Workspace()]
    coefs = [None]

    def load(row):
        for b, f in zip(bufs, row):
            b.view.zero_()
            b.view[:len(f)].copy_(torch.frombuffer(bytearray(f), dtype=torch.uint8))

    def step():
        r = tq.read_batch([b.view for b in bufs], outs=coefs[0], workspace=ws[0])
        res = tq.quantsmooth_batch_(r["images"], flags, 1, workspace=ws[1])
        return r, res, tq.encode_scan_batch(r["images"], result=res, outs=[o.view for o in outs], workspace=ws[2],
                                            restart_interval=4)

    load(files[0])
    r, res, out = step()                                                # eager: prepares the three workspaces
    ws[1] = res["workspace"]
    coefs[0] = [im["coefs"] for im in r["images"]]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gr, gres, gout = step()
    for v in (1, 2):
        load(files[v])
        g.replay()
        torch.cuda.synchronize()
        assert gr["status"].cpu().tolist() == [0, 0] and gout["status"].cpu().tolist() == [0, 0]
        for k, (o, l) in enumerate(zip(outs, gout["len"].cpu().tolist())):
            assert o.view[:l].cpu().numpy().tobytes() == want[v][k], f"replay of variant {v}, image {k}"
            o.check()
        for b in bufs:
            b.check()


def test_corrupt_corpus_reports_what_the_host_build_reports(tools, grid):
    """the corrupt corpus of tests/test_read_host.py (green there, for the same qs_read.h, before this runs anywhere) in
    one batch with valid jobs between the corrupt ones: the statuses of the host build, every margin intact, the valid
    jobs still exact"""
    enc, lj, d = tools
    corpus = corrupt_corpus(corpus_sources(enc, lj))
    host = [s for s, _a in ReadHost(d).run(corpus)]
    assert all(0 <= s <= 3 for s in host) and {1, 2, 3} <= set(host)
    valid = grid[5::9]
    cases, is_valid = [], []
    for k, c in enumerate(corpus):
        if k % 40 == 0:
            cases.append(valid[(k // 40) % len(valid)])
            is_valid.append(True)
        cases.append(c)
        is_valid.append(False)
    status, arrs = Batch(cases).run()
    assert [s for s, v in zip(status, is_valid) if not v] == host
    good = [k for k, v in enumerate(is_valid) if v]
    _assert_exact([cases[k] for k in good], [status[k] for k in good], [arrs[k] for k in good])
