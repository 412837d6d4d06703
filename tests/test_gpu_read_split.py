"""The split route of the device scan reader on the GPU (qs_hip_read_split_device_batch, torch_qs.read /
read_batch(split=True)): the valid corpus of tests/read_oracle.py plus files of hundreds of segments against libjpeg 9's
own read, both routes on the same restart files, the round trip through the device entropy coder, a captured graph, and
the corrupt corpus against the host build of the same csrc/qs_read_split.h.  Every array, file, status buffer and
workspace lies between sentinel margins."""
import numpy as np
import pytest

import jpegqs_pkg
from encode_oracle import synth_scan_image
from encode_rst_oracle import LibJpeg9EncRst, parse_rst
from helpers import Guarded
from read_oracle import LibjpegReader, build_grid, corpus_sources, corrupt_corpus, make_case
from read_split_oracle import SPLIT_BYTES, SplitHost, dc_wrap_cases, long_symbol_case, natural_image, without_markers

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
jpeg_file = pkg.jpeg_file


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpureadsplit")
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
    """the cases' scans, arrays, status and workspace on the device, each between margins; the C ABI called directly.
    A case holds its scan (the bytes behind the SOS header) and the parsed header."""

    def __init__(self, cases, split=True):
        self.hip = pkg.HipQS()
        self.cases, self.split = cases, split
        self.scans, self.arrs, self.jobs, self.opts = [], [], [], []
        for c in cases:
            p = c["header"]
            f = Guarded(max(1, len(c["scan"])))                          # (a scan truncated to nothing still has an address)
            if c["scan"]:
                f.view.copy_(torch.frombuffer(bytearray(c["scan"]), dtype=torch.uint8))
            self.scans.append(f)
            a = [Guarded(rows * stride * 64, torch.int16) for rows, stride in c["shapes"]]
            self.arrs.append(a)
            self.jobs.append(self.hip.device_job([g.view.data_ptr() for g in a], c["shapes"], [None] * len(a), hsamp=p["hsamp"],
                                                 vsamp=p["vsamp"], colorspace=p["colorspace"], image_size=p["image_size"]))
            self.opts.append(self.hip.read_opts(p["dc"], p["ac"], p["dc_tbl"], p["ac_tbl"], p["restart_interval"]))
        self.per, total = self.hip.read_batch_info(self.jobs, self.opts, split=split)
        self.ws = Guarded(total)
        self.status = Guarded(len(cases), torch.int32)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.hip.read_batch_prepare(self.jobs, self.opts, self.ws.view.data_ptr(), total, self.stream, split=split)

    def fill(self, value):
        for a in self.arrs:
            for g in a:
                g.view.fill_(value)

    def run(self):
        """-> (status list, [[arrays (rows, stride, 64)] per case]); the margins and the scans checked"""
        self.hip.read_batch(self.jobs, [f.view.data_ptr() for f in self.scans], [len(c["scan"]) for c in self.cases],
                            self.status.view.data_ptr(), self.ws.view.data_ptr(), self.ws.view.numel(), self.stream,
                            split=self.split)
        torch.cuda.synchronize()
        self.ws.check()
        self.status.check()
        out = []
        for c, f, a in zip(self.cases, self.scans, self.arrs):
            f.check()
            assert f.view[:len(c["scan"])].cpu().numpy().tobytes() == bytes(c["scan"]), "the reader changed its input"
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


def test_grid_and_long_intervals_in_one_batch_and_again_over_stale_arrays(tools, grid):
    """the grid of tests/read_oracle.py, the crafted scans of tests/test_read_split_host.py, a 768 x 640 4:2:0 file
    at quality 90 without DRI (its segments span three workgroups of the segment launches) and the 200 x 200-block gray
    scan of one interval that the interval route refuses, in one batch of many launch chunks against libjpeg's arrays;
    the inputs unchanged; then once more into the same arrays filled with 0x5a5a"""
    enc, lj, _d = tools
    big = make_case(enc, lj, "768 x 640 4:2:0 at quality 90, no DRI", natural_image(768, 640, 2, 2, 90, 3), 0, 0, 0)
    assert len(big["scan"]) > 2 * 256 * SPLIT_BYTES and big["header"]["restart_interval"] == 0
    gray = make_case(enc, lj, "200 x 200 blocks of gray, one interval",
                     synth_scan_image(np.random.default_rng(5), (1600, 1600), [1], [1], 1, amp=20, density=0.1), 0, 0, 0)
    assert gray["shapes"] == [(200, 200)] and gray["header"]["restart_interval"] == 0
    hip = pkg.HipQS()
    p = gray["header"]
    job = hip.device_job([0x1000], [(200, 200)], [None], hsamp=[1], vsamp=[1], colorspace=1, image_size=(1600, 1600))
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.read_batch_info([job], [hip.read_opts(p["dc"], p["ac"], [0], [0], 0)])
    assert e.value.code == -4
    cases = grid[:100] + [big] + grid[100:200] + [gray, long_symbol_case()] + dc_wrap_cases() + grid[200:]
    assert len(cases) > 3 * 32
    b = Batch(cases)
    assert b.per[100]["intervals"] == 1 and b.per[100]["max_segments"] > 2 * 256
    _assert_exact(cases, *b.run())
    b.fill(0x5a5a)
    _assert_exact(cases, *b.run())


def test_both_routes_agree_on_restart_files(grid):
    """files with restart markers -- intervals of one MCU up to the whole scan -- through both routes: the same status
    and the same arrays"""
    some = [c for c in grid if c["header"]["restart_interval"]][::2]
    assert len(some) > 50
    s_old, a_old = Batch(some, split=False).run()
    s_new, a_new = Batch(some, split=True).run()
    assert s_old == s_new == [0] * len(some)
    for c, x, y in zip(some, a_old, a_new):
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), c["name"]


def _upload(im):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in im["coefs"]]


def test_round_trip_with_the_device_coder(tq, tools):
    """encode without restart markers, then read(split=True), gives the original arrays; encode_scan of what was read,
    with the returned tables, gives the file's own scan bytes -- host bytes, a host tensor and a device tensor"""
    enc, _lj, _d = tools
    rng = np.random.default_rng(78)
    ims = [synth_scan_image(rng, (141, 93), [2, 1, 1], [2, 1, 1], 3), synth_scan_image(rng, (67, 131), [1], [1], 1),
           synth_scan_image(rng, (33, 9), [1, 1, 1, 1], [1, 1, 1, 1], 4)]
    for im in ims:
        data = tq.encode(_upload(im), im["quants"], **_kw(im))
        assert jpeg_file.parse(data)["restart_interval"] == 0
        for src in (data, torch.frombuffer(bytearray(data), dtype=torch.uint8), torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()):
            got = tq.read(src, split=True)
            assert int(got["status"]) == 0
            assert got["image_size"] == tuple(im["image_size"]) and got["hsamp"] == im["hsamp"] and got["colorspace"] == im["colorspace"]
            for a, b, q, qw in zip(got["coefs"], im["coefs"], got["quants"], im["quants"]):
                assert np.array_equal(a.cpu().numpy(), b)
                assert np.array_equal(q, qw)
        for opt in (False, True):
            data = enc.write(im, 0, 0, opt)                             # libjpeg's file, optimized tables in one
            got = tq.read(data, split=True)
            assert int(got["status"]) == 0 and got["restart_interval"] == 0 and got["huffman"] is not None
            seg = tq.encode_scan(got["coefs"], **_kw(got), huffman=got["huffman"])
            assert int(seg["status"]) == 0
            assert seg["segment"][:int(seg["len"])].cpu().numpy().tobytes() == parse_rst(data)["segment"]


def test_read_smooth_and_encode_in_one_captured_graph(tq, tools):
    """read_batch(split=True), quantsmooth_batch_ and encode_scan_batch captured in one graph and replayed with other
    file bytes of the same header in the same device buffers -- other bytes synchronise in another pattern: the eager
    result of each file"""
    enc, _lj, _d = tools
    sizes = [(259, 203), (64, 48)]
    files = []                                                          # files[v][k]: variant v of image k
    for v in range(3):
        row = []
        for k, (w, h) in enumerate(sizes):
            y = pkg.synth.synth_ycc(w, h, 2, 2, quality=50, seed=200 + 10 * v + k)     # natural statistics: no range-check stop
            row.append(enc.write(dict(coefs=y["coefs"], quants=y["quants"], hsamp=y["hsamp"], vsamp=y["vsamp"], colorspace=3,
                                      image_size=(w, h)), 0, 0))
        files.append(row)
    heads = [[f[:jpeg_file.parse(f)["scan_offset"]] for f in row] for row in files]
    assert heads[0] == heads[1] == heads[2]
    assert all(len(row[0]) - len(heads[0][0]) > 8 * SPLIT_BYTES for row in files)       # several segments
    flags = pkg.flags_for_quality(3)

    def eager(row):
        r = tq.read_batch(row, split=True)
        res = tq.quantsmooth_batch_(r["images"], flags, 1)
        out = tq.encode_scan_batch(r["images"], result=res)
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
        r = tq.read_batch([b.view for b in bufs], outs=coefs[0], workspace=ws[0], split=True)
        res = tq.quantsmooth_batch_(r["images"], flags, 1, workspace=ws[1])
        return r, res, tq.encode_scan_batch(r["images"], result=res, outs=[o.view for o in outs], workspace=ws[2])

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
    """the corrupt corpus of tests/test_read_split_host.py (green there, for the same qs_read_split.h, before this runs
    anywhere), with and without its markers, in one batch with valid jobs between the corrupt ones: the statuses of
    the host build, every margin intact, the valid jobs still exact"""
    enc, lj, d = tools
    corpus = corrupt_corpus(corpus_sources(enc, lj))
    corpus = corpus + [without_markers(c) for c in corpus[::3]]
    host = [s for s, _r, _n, _a in SplitHost(d).run(corpus)]
    assert all(0 <= s <= 4 for s in host) and {1, 2, 3} <= set(host)
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
