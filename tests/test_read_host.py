"""The device scan reader without a GPU: csrc/qs_read.h compiled for the host (tests/read_host.cpp) against libjpeg 9 at
both ends -- files written by libjpeg (tests/libjpeg9_encode.c), expected arrays read by libjpeg
(tests/libjpeg9_decode.c) -- and the same program under -fsanitize=address,undefined on a seeded corrupt corpus."""
import re

import numpy as np
import pytest

from encode_rst_oracle import LibJpeg9EncRst
from read_oracle import (LibjpegReader, ReadHost, build_grid, corpus_sources, corrupt_corpus, expected_arrays,
                         true_shapes)


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("read")
    return LibJpeg9EncRst(d), LibjpegReader(d), d


@pytest.fixture(scope="module")
def grid(tools):
    enc, lj, _d = tools
    return build_grid(enc, lj)


def _compare(cases, results):
    for c, (status, arrs) in zip(cases, results):
        assert status == 0, (c["name"], status)
        for ci, (a, w) in enumerate(zip(arrs, c["want"])):
            if not np.array_equal(a, w):
                bad = np.argwhere((a != w).any(axis=2))
                raise AssertionError(f"{c['name']}: component {ci} of shape {a.shape[:2]}: {len(bad)} blocks differ, "
                                     f"first at (by, bx) = {tuple(bad[0])}")


def test_grid_equals_libjpeg(tools, grid):
    """every layout x restart interval, the DC extremes, a stuffed FF 00 in front of a marker, optimized tables and a
    table with 16-bit codes: the arrays are libjpeg's for every block inside the array, the dummy blocks of edge MCUs
    included, and 0 outside (every third case has arrays wider and taller than needed)"""
    _enc, _lj, d = tools
    assert any(max(c["header"]["ac"][t][0][16] for t in c["header"]["ac"]) > 0 for c in grid), "no 16-bit code in the grid"
    assert any(c["shapes"] != true_shapes(c["header"]) for c in grid), "no array larger than libjpeg's geometry"
    assert any(re.search(rb"\xff\x00\xff[\xd0-\xd7]", c["scan"]) for c in grid), "no stuffed FF 00 in front of a marker"
    _compare(grid, ReadHost(d).run(grid))


def test_scan_in_a_larger_buffer(tools, grid):
    """EOI and anything behind it are ignored: the same arrays with the rest of the file, and junk that holds markers,
    behind the segment"""
    _enc, _lj, d = tools
    some = [dict(c, scan=c["scan"] + b"\xff\xd0junk\xff\xd9\xff\x00" * 3) for c in grid[::17]]
    _compare(some, ReadHost(d).run(some))


def test_interval_cap_and_bad_tables_are_refused(tools, grid):
    _enc, _lj, d = tools
    c = grid[0]
    big = dict(c, header=dict(c["header"], image_size=(8 * 200, 8 * 200), restart_interval=0), shapes=[(200, 200)])
    assert big["header"]["hsamp"] == [1]
    bits = [0] * 17
    bits[1] = 3                                                         # three codes of one bit
    bad = dict(c, header=dict(c["header"], dc={0: (bits, [0, 1, 2])}))
    (s1, _), (s2, _) = ReadHost(d).run([big, bad])
    assert (s1, s2) == (-3, -1)


def test_corrupt_corpus_under_sanitizers(tools):
    """the host build with -fsanitize=address,undefined, as its own process: no report, every status in 0..3, non-zero
    wherever libjpeg's own read of the file warns or stops; where both read it clean the arrays are equal; at most 5 % of
    the corpus is damage that happens to decode"""
    enc, lj, d = tools
    corpus = corrupt_corpus(corpus_sources(enc, lj))
    assert len(corpus) > 500
    results = ReadHost(d, sanitize=True).run(corpus)
    plain = ReadHost(d).run(corpus)
    assert [s for s, _ in results] == [s for s, _ in plain]
    both_clean = 0
    for c, (status, arrs) in zip(corpus, results):
        assert status in (0, 1, 2, 3), (c["name"], status)
        ref, clean = lj.read_bytes(c["data"])
        if not clean:
            assert status != 0, f"{c['name']}: libjpeg warns or stops, the reader reports 0"
        elif status == 0:
            both_clean += 1
            for a, w in zip(arrs, expected_arrays(ref, c["shapes"])):
                assert np.array_equal(a, w), c["name"]
    print(f"corpus: {len(corpus)} cases, {both_clean} decode clean here and in libjpeg")
    assert both_clean <= 0.05 * len(corpus), (both_clean, len(corpus))


def test_info_call_needs_no_device_and_refuses_what_the_reader_does_not_cover():
    import jpegqs_pkg
    pkg = jpegqs_pkg.load()
    hip = pkg.HipQS()

    def job(shapes, hs, vs, size):
        return hip.device_job([0x1000 * (i + 1) for i in range(len(shapes))], shapes, [None] * len(shapes), hsamp=hs, vsamp=vs,
                              colorspace=3 if len(shapes) == 3 else 1, image_size=size)

    def code(j, o):
        with pytest.raises(pkg.hipqs.QsHipError) as e:
            hip.read_batch_info([j], [o])
        return e.value.code

    ycc = job([(12, 18), (6, 9), (6, 9)], [2, 1, 1], [2, 1, 1], (141, 93))
    o = hip.read_opts(dc_tbl=[0, 1, 1], ac_tbl=[0, 1, 1], restart_interval=7)
    per, nbytes = hip.read_batch_info([ycc, ycc], [o, o])
    assert per[0] == dict(blocks_in_mcu=6, mcus=54, intervals=8, blocks_per_interval=42) and nbytes > 2 * 7000
    assert hip.read_batch_info([ycc], [hip.read_opts(dc_tbl=[0, 1, 1], ac_tbl=[0, 1, 1], restart_interval=60)])[0][0]["intervals"] == 1
    assert code(job([(12, 17), (6, 9), (6, 9)], [2, 1, 1], [2, 1, 1], (141, 93)), o) == -2        # an array too narrow
    assert code(ycc, hip.read_opts(dc_tbl=[0, 2, 1], ac_tbl=[0, 1, 1])) == -2                      # table 2 is not there
    assert code(ycc, hip.read_opts(dc_tbl=[0, 1, 1], ac_tbl=[0, 1, 1], restart_interval=70000)) == -2
    assert code(job([(8, 8), (8, 8), (8, 8)], [4, 2, 2], [2, 2, 1], (64, 64)), o) == -4             # 14 blocks in an MCU
    gray = job([(200, 200)], [1], [1], (1600, 1600))
    assert code(gray, hip.read_opts(dc_tbl=[0], ac_tbl=[0])) == -4                                  # 40 000 blocks, one interval
    assert hip.read_batch_info([gray], [hip.read_opts(dc_tbl=[0], ac_tbl=[0], restart_interval=200)])[0][0]["intervals"] == 200
