"""The three scan readers on the GPU on files libjpeg 9 does not write (the corpus of tests/foreign_files.py, green on the
host builds in tests/test_foreign_files_host.py before this runs anywhere): what only runs here -- the drivers' descriptor
building, the staging of tables by id in LDS, the per-job table slots across launch chunks of 32 jobs, and the
torch_qs.read* layer -- against libjpeg 9's own read of every file.  Every array, file, status buffer and workspace lies
between sentinel margins (the Batch helpers of the three reader test modules)."""
import numpy as np
import pytest

import jpegqs_pkg
from encode_prog_oracle import LibJpeg9EncProg
from encode_rst_oracle import LibJpeg9EncRst
from foreign_files import foreign_cases, read_cases, refused_case
from read_oracle import LibjpegReader
from read_split_oracle import SplitHost
from test_gpu_read import Batch as IntervalBatch
from test_gpu_read_prog import Batch as ProgBatch
from test_gpu_read_split import Batch as SplitBatch

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
jpeg_file = pkg.jpeg_file
CHUNK = 32                         # QS_RD_CHUNK: jobs per launch chunk


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpuforeign")
    return LibJpeg9EncProg(d), LibJpeg9EncRst(d), LibjpegReader(d), d


@pytest.fixture(scope="module")
def specs(tools):
    return foreign_cases(tools[0], tools[1])


@pytest.fixture(scope="module")
def prog(tools, specs):
    return read_cases(tools[2], specs["prog"])


@pytest.fixture(scope="module")
def base(tools, specs):
    return read_cases(tools[2], specs["base"], 1)


@pytest.fixture(scope="module")
def tq():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible to torch")
    return pkg.torch_qs


def _mixed(cases):
    """the cases with the writer's files (tables by id, in one DHT) and libjpeg's (tables per scan) in turns, so that
    neighbours in a launch chunk differ in their table slots, repeated up to more than one chunk"""
    ours, theirs = [c for c in cases if c["fixed"]], [c for c in cases if not c["fixed"]]
    out = []
    for k in range(max(len(ours), len(theirs))):
        out += ours[k:k + 1] + theirs[k:k + 1]
    assert len(out) == len(cases)
    return out + out[:max(0, 40 - len(out))]


def _check(cases, status, arrs, want_status=None):
    for k, (c, s, a) in enumerate(zip(cases, status, arrs)):
        assert s == (0 if want_status is None else want_status[k]), (c["name"], s)
        if s:
            continue
        for ci, (got, want) in enumerate(zip(a, c["want"])):
            if not np.array_equal(got, want):
                bad = np.argwhere((got != want).any(axis=2))
                raise AssertionError(f"{c['name']}: component {ci}: {len(bad)} blocks differ, first at {tuple(bad[0])}")


def test_progressive_corpus_in_one_batch_and_again_over_stale_arrays(prog):
    """the whole progressive corpus through the C ABI in one batch longer than a launch chunk, jobs with different table
    assignments next to each other: status 0 and libjpeg's arrays, then once more into arrays filled with 0x5a5a"""
    cases = _mixed(prog)
    assert len(cases) >= 40 > CHUNK
    b = ProgBatch(cases)
    assert max(max(p["intervals"]) for p in b.per) > 64                 # more than one decode workgroup in a pair
    _check(cases, *b.run())
    b.fill(0x5a5a)
    _check(cases, *b.run())


def test_baseline_corpus_through_both_sequential_routes(tools, base):
    """the baseline corpus through the interval route and through the split route in the same way; the split route
    reports what its host build reports for the file (0, or 4 where the segments do not synchronise in its rounds), and
    the two routes agree wherever both report 0"""
    cases = _mixed(base)
    assert len(cases) >= 40 > CHUNK
    host = [s for s, _r, _n, _a in SplitHost(tools[3]).run(cases)]
    assert set(host) <= {0, 4} and host.count(0) > CHUNK
    ib, sb = IntervalBatch(cases), SplitBatch(cases)
    for fill in (None, 0x5a5a):
        if fill is not None:
            ib.fill(fill)
            sb.fill(fill)
        s_int, a_int = ib.run()
        _check(cases, s_int, a_int)
        s_spl, a_spl = sb.run()
        _check(cases, s_spl, a_spl, host)
        for c, s, x, y in zip(cases, s_spl, a_int, a_spl):
            if s == 0:
                assert all(np.array_equal(p, q) for p, q in zip(x, y)), c["name"]


def _foreign_ids(p):
    return any(td != ta or td > 1 for td, ta in zip(p["dc_tbl"], p["ac_tbl"]))


def _assert_image(got, c, lj=None):
    assert int(got["status"]) == 0, c["name"]
    p, ref = c["header"], c["ref"]
    assert got["image_size"] == tuple(p["image_size"]) and got["hsamp"] == p["hsamp"] and got["vsamp"] == p["vsamp"], c["name"]
    for t, w, q, qw in zip(got["coefs"], ref["coefs"], got["quants"], p["quants"]):
        assert np.array_equal(t.cpu().numpy(), w), c["name"]
        assert np.array_equal(q, qw), c["name"]


def test_torch_layer_reads_the_corpus_from_bytes_and_from_device_tensors(tq, prog, base):
    """torch_qs.read on every file as bytes and on every third as a device tensor, read_batch on each corpus whole, and
    read(split=True) where the split route reads the file: libjpeg's arrays, the file's quantisers and geometry; huffman is
    None exactly when a component's Td != Ta or a table id above 1 is used (always for a progressive file)"""
    for k, c in enumerate(prog + base):
        srcs = [c["data"]] + ([torch.frombuffer(bytearray(c["data"]), dtype=torch.uint8).cuda()] if k % 3 == 0 else [])
        for src in srcs:
            got = tq.read(src)
            _assert_image(got, c)
            if c["kind"] == "prog":
                assert got["huffman"] is None and got["scans"] == c["header"]["script"], c["name"]
                assert got["restart_interval"] == c["header"]["scans"][0]["restart_interval"], c["name"]
            else:
                assert (got["huffman"] is None) == _foreign_ids(c["header"]), c["name"]
                assert got["restart_interval"] == c["header"]["restart_interval"], c["name"]
    assert any(_foreign_ids(c["header"]) for c in base) and not all(_foreign_ids(c["header"]) for c in base)
    for cases in (prog, base):
        r = tq.read_batch([c["data"] for c in cases])
        torch.cuda.synchronize()
        assert r["status"].cpu().tolist() == [0] * len(cases)
        for im, c in zip(r["images"], cases):
            _assert_image(im, c)
    r = tq.read_batch([torch.frombuffer(bytearray(c["data"]), dtype=torch.uint8).cuda() for c in base], split=True)
    torch.cuda.synchronize()
    status = r["status"].cpu().tolist()
    assert set(status) <= {0, 4} and status.count(0) > CHUNK
    for im, c, s in zip(r["images"], base, status):
        if s == 0:
            _assert_image(im, c)


def _libjpeg_of(lj, r):
    torch.cuda.synchronize()
    assert int(r["status"][0]) == 0
    ref, clean = lj.read_bytes(r["file"][:int(r["len"][0])].cpu().numpy().tobytes())
    assert clean
    return ref


def test_what_was_read_writes_files_libjpeg_reads_to_the_same_arrays(tq, tools, prog, base):
    """read -> encode_file(optimize=True) -> libjpeg's read for baseline files with foreign tables (huffman is None: the
    coder makes its own), and read -> encode_file(scans=the script read, refinement=True, restart_interval=the file's) ->
    libjpeg's read for progressive ones: the arrays libjpeg read from the foreign file"""
    lj = tools[2]
    some = [c for c in base if c["fixed"] and c["header"]["colorspace"] == 3][:4] + [c for c in base if c["fixed"] and len(c["header"]["hsamp"]) == 1][:1]
    assert len(some) == 5 and all(_foreign_ids(c["header"]) for c in some)
    for c in some:
        got = tq.read(c["data"])
        assert int(got["status"]) == 0 and got["huffman"] is None
        ref = _libjpeg_of(lj, tq.encode_file(got["coefs"], got["quants"], hsamp=got["hsamp"], vsamp=got["vsamp"],
                                             colorspace=got["colorspace"], image_size=got["image_size"], optimize=True,
                                             restart_interval=got["restart_interval"] or None))
        assert all(np.array_equal(a, w) for a, w in zip(ref["coefs"], c["ref"]["coefs"])), c["name"]
    names = ("simple progression, Td (3,2,1) Ta (1,2,3)", "script 'ac two steps', Td (2,0,3) Ta (3,1,0), Ri 1",
             "a refinement that spans two first-scan bands", "a first-scan band refined in two",
             "gray refine, ids 2/3, no DRI, zero pad bits")
    some = [c for c in prog if c["name"] in names]
    assert len(some) == len(names)
    for c in some:
        got = tq.read(c["data"])
        assert int(got["status"]) == 0
        ri = got["restart_interval"]
        assert all(s["restart_interval"] == ri for s in c["header"]["scans"])
        ref = _libjpeg_of(lj, tq.encode_file(got["coefs"], got["quants"], hsamp=got["hsamp"], vsamp=got["vsamp"],
                                             colorspace=got["colorspace"], image_size=got["image_size"], scans=got["scans"],
                                             refinement=True, restart_interval=ri or None))
        assert all(np.array_equal(a, w) for a, w in zip(ref["coefs"], c["ref"]["coefs"])), c["name"]


def test_fill_bytes_in_front_of_rstn_are_refused_by_status(tools, specs, prog, base):
    """the stated limit (DESIGN.md sections 14 and 18): files with FF FF Dn, read with what a prepare on the intact file
    holds, end with a non-zero status on every route, every margin intact (Batch.run checks them), and the valid jobs
    on both sides of them still exact"""
    lj = tools[2]
    bad = [refused_case(lj, s) for s in specs["refused"] if s["intact"] is not None]
    bad_base, bad_prog = [c for c in bad if c["kind"] == "base"], [c for c in bad if c["kind"] == "prog"]
    assert bad_base and bad_prog
    for make, valid, refused in ((IntervalBatch, base, bad_base), (SplitBatch, base, bad_base), (ProgBatch, prog, bad_prog)):
        cases, is_bad = [valid[0]], [False]
        for k, c in enumerate(refused):
            cases += [c, valid[1 + k]]
            is_bad += [True, False]
        status, arrs = make(cases).run()
        for c, s, a, refuse in zip(cases, status, arrs, is_bad):
            if refuse:
                assert 1 <= s <= 3, (make.__module__, c["name"], s)
            else:
                _check([c], [s], [a])
