"""The split route of the device scan reader without a GPU: csrc/qs_read_split.h compiled for the host
(tests/read_split_host.cpp: qr_split_serial runs the kernels' stages one after the other on the functions a lane runs)
against libjpeg 9's arrays and against the one-lane-per-interval reader of the same inputs (tests/read_host.cpp); the
same program with no synchronisation rounds, with segments of 16 bytes, and under -fsanitize=address,undefined on the
corrupt corpus."""
import collections

import numpy as np
import pytest

from encode_rst_oracle import LibJpeg9EncRst
from read_oracle import LibjpegReader, ReadHost, corpus_sources, corrupt_corpus
from read_split_oracle import (SPLIT_BYTES, SPLIT_ROUNDS, SplitHost, boundary_facts, dc_wrap_cases, intervals_of,
                               long_symbol_case, split_corpus, table_period, without_markers)

SMALL = 16                         # bytes per segment of the build that cuts small files into many segments ...
SMALL_ROUNDS = 300                 # ... and its rounds: twice the 118 the worst file of the corpus needs there, and more


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("readsplit")
    return LibJpeg9EncRst(d), LibjpegReader(d), d


@pytest.fixture(scope="module")
def corpus(tools):
    enc, lj, _d = tools
    return split_corpus(enc, lj)


@pytest.fixture(scope="module")
def crafted():
    return [long_symbol_case()] + dc_wrap_cases()


@pytest.fixture(scope="module")
def plain(tools, corpus, crafted):
    """the shipped constants on the valid corpus and the crafted scans"""
    return SplitHost(tools[2]).run(corpus + crafted)


def _exact(cases, results):
    for c, (status, _needed, _nseg, arrs) in zip(cases, results):
        assert status == 0, (c["name"], status)
        for ci, (a, w) in enumerate(zip(arrs, c["want"])):
            if not np.array_equal(a, w):
                bad = np.argwhere((a != w).any(axis=2))
                raise AssertionError(f"{c['name']}: component {ci}: {len(bad)} blocks differ, first at (by, bx) = {tuple(bad[0])}")


def test_header_and_kernel_constants_agree():
    import re
    from read_oracle import CSRC, HERE, pkg
    hdr = (HERE.parent / "include" / "jpegqs_hip.h").read_text()
    src = (CSRC / "qs_read_split.h").read_text()
    for name, want in (("BYTES", SPLIT_BYTES), ("ROUNDS", SPLIT_ROUNDS)):
        assert int(re.search(rf"#define QS_HIP_READ_SPLIT_{name} (\d+)", hdr).group(1)) == want
        assert int(re.search(rf"#define QS_RD_SPLIT_{name} (\d+)", src).group(1)) == want
    assert (pkg.hipqs.READ_SPLIT_BYTES, pkg.hipqs.READ_SPLIT_ROUNDS) == (SPLIT_BYTES, SPLIT_ROUNDS)


def test_corpus_equals_libjpeg_and_the_interval_reader(tools, corpus, crafted, plain):
    """every file of the valid corpus and every crafted scan: status 0 -- never 4 -- and libjpeg's arrays, dummy blocks
    and zeros outside included; the arrays of qr_read_serial wherever that reads the file; every file synchronises in
    at most (R - 1) / 2 rounds, the margin R was chosen with"""
    cases = corpus + crafted
    _exact(cases, plain)
    hist = collections.Counter(needed for _s, needed, _n, _a in plain)
    print("rounds needed -> files:", sorted(hist.items()))
    assert 0 <= min(hist) and max(hist) <= (SPLIT_ROUNDS - 1) // 2, sorted(hist.items())
    assert max(nseg for _s, _r, nseg, _a in plain) > 100
    for c, (status, arrs), (_s, _r, _n, got) in zip(cases, ReadHost(tools[2]).run(cases), plain):
        assert status == 0, c["name"]
        assert all(np.array_equal(a, b) for a, b in zip(arrs, got)), c["name"]


def test_corpus_holds_the_situations_that_matter(corpus, crafted):
    """by the bytes: a segment boundary on an FF, one on the 00 behind it, an interval shorter than a segment beside
    intervals of several, a last interval of one MCU, symbols across boundaries -- among them a 16-bit code with 15
    value bits -- and every table period"""
    facts = collections.Counter(f for c in corpus for f in boundary_facts(c))
    for f in ("boundary on FF", "boundary on the 00 behind FF", "short interval beside long ones", "last interval of one MCU"):
        assert facts[f] > 0, f
    assert {table_period(c["header"]) for c in corpus} >= {1, 3, 4, 6}
    long = crafted[0]
    (start, nbits), = [(p, n) for p, n in long["symbols"] if n == 31]
    assert start < 8 * SPLIT_BYTES < start + nbits and max(long["header"]["ac"][0][0][16:]) == 1
    # any other symbol across a boundary: the bit in front of a boundary and the one behind it belong to one symbol
    wrap = crafted[1]
    (a, z), = intervals_of(wrap["scan"])
    assert any(p < 8 * b < p + n for p, n in wrap["symbols"] for b in range(a + SPLIT_BYTES, z, SPLIT_BYTES))


def test_dc_sums_pass_the_short_range_across_segments_and_intervals(crafted, plain, corpus):
    """the running DC sum, carried as libjpeg's int and stored as a short, passes +-32768 inside a segment, from one
    segment to the next, and stands far from 0 where an interval ends and the next starts at 0 again"""
    for c, res in list(zip(corpus + crafted, plain))[-2:]:
        diffs_wrap = 0
        dc = c["want"][0].reshape(-1, 64)[:, 0].astype(np.int64)
        ri = c["header"]["restart_interval"] or len(dc)
        for first in range(0, len(dc), ri):
            d = np.diff(dc[first:first + ri], prepend=0)
            diffs_wrap += int((np.abs(d) > 32767).sum())               # a step no 15-bit difference makes: the sum wrapped
        assert diffs_wrap > 20, c["name"]
        assert res[2] >= 4 and res[0] == 0                             # several segments
        if c["header"]["restart_interval"]:
            assert abs(int(dc[ri - 1])) > 1000 and len(intervals_of(c["scan"])) == 3
    _exact((corpus + crafted)[-2:], plain[-2:])


def test_table_periods(tools, corpus, plain):
    """p = 1 (gray, RGB, CMYK), 3 (4:4:4), 4 (2x1, 1x2, YCCK) and 6 (4:2:0) each read exactly, each with files of many
    segments.  The state the segments compare and hand on is (bit position, k, u mod p).  A build that compared u
    itself would fail the p = 1 files by status 4: with one table pair two decoders that differ only in u decode the
    same symbols for ever, so a guessed u = 0 would be put right by one segment per round only.  Such a build is not
    shipped; the p = 1 files here need the same few rounds as the others."""
    by_p = collections.defaultdict(list)
    for c, (status, needed, nseg, _a) in zip(corpus, plain):
        by_p[table_period(c["header"])].append((status, needed, nseg, len(c["header"]["hsamp"])))
    for p in (1, 3, 4, 6):
        assert by_p[p] and all(s == 0 for s, _r, _n, _c in by_p[p]), p
        assert max(n for _s, _r, n, _c in by_p[p]) >= 20, p
    many = [(needed, nseg) for _s, needed, nseg, ncomp in by_p[1] if ncomp > 1 and nseg >= 20]
    assert many and all(needed <= (SPLIT_ROUNDS - 1) // 2 < nseg - 1 for needed, nseg in many)


def test_without_rounds_the_verify_step_refuses_what_did_not_synchronise(tools, corpus, crafted, plain):
    """-DQS_RD_SPLIT_ROUNDS=0: only the speculative pass runs.  Status 4 for exactly the files whose guesses were not
    all true already, status 0 and libjpeg's arrays for the others: never wrong arrays with status 0"""
    cases = corpus + crafted
    res = SplitHost(tools[2], rounds=0).run(cases)
    refused = 0
    for c, (status, needed, nseg, arrs), (_s, needed_r, nseg_r, _a) in zip(cases, res, plain):
        assert nseg == nseg_r
        if needed_r == 0:
            assert status == 0 and needed == 0, c["name"]
            assert all(np.array_equal(a, w) for a, w in zip(arrs, c["want"])), c["name"]
        else:
            assert status == 4 and needed == -1, (c["name"], status)
            refused += 1
    assert refused > len(cases) // 2 and refused < len(cases)


def test_small_segments(tools, corpus, crafted):
    """-DQS_RD_SPLIT_BYTES=16: up to two thousand segments in the files of the corpus, segments shorter than a symbol,
    boundaries inside almost every symbol"""
    cases = corpus + crafted
    res = SplitHost(tools[2], rounds=SMALL_ROUNDS, nbytes=SMALL).run(cases)
    _exact(cases, res)
    assert max(n for _s, _r, n, _a in res) > 1000 and max(r for _s, r, _n, _a in res) < SMALL_ROUNDS // 2
    some = crafted + corpus[::7]                                         # and valid files under the sanitizers, both sizes
    _exact(some, SplitHost(tools[2], sanitize=True, rounds=SMALL_ROUNDS, nbytes=SMALL).run(some))
    _exact(some, SplitHost(tools[2], sanitize=True).run(some))


def test_corrupt_corpus_under_sanitizers(tools):
    """the corrupt corpus of tests/test_read_host.py, and each of its files once more with the markers taken out and
    DRI 0 (one interval of many segments), under -fsanitize=address,undefined with segments of 256 and of 16 bytes: no
    report -- every array and every scan is a heap block of exactly its size -- and, against qr_read_serial on the same
    input: status 0 for exactly the same inputs, with equal arrays; status 1 for exactly the same inputs; non-zero
    everywhere else"""
    enc, lj, d = tools
    corpus = corrupt_corpus(corpus_sources(enc, lj))
    corpus = corpus + [without_markers(c) for c in corpus]
    assert len(corpus) > 1000
    serial = ReadHost(d).run(corpus)
    assert {0, 1, 2, 3} <= {s for s, _a in serial}
    for host in (SplitHost(d, sanitize=True), SplitHost(d, sanitize=True, rounds=SMALL_ROUNDS, nbytes=SMALL)):
        res = host.run(corpus)
        clean = 0
        for c, (s0, a0), (s1, _r, _n, a1) in zip(corpus, serial, res):
            assert 0 <= s1 <= 4, (c["name"], s1)
            assert (s1 == 0) == (s0 == 0) and (s1 == 1) == (s0 == 1), (host.exe.name, c["name"], s0, s1)
            if s0 == 0:
                clean += 1
                assert all(np.array_equal(x, y) for x, y in zip(a0, a1)), c["name"]
        assert clean > 10
        print(f"{host.exe.name}: {len(corpus)} cases, {clean} read clean by both, statuses "
              f"{sorted(collections.Counter(s for s, _r, _n, _a in res).items())}")
    assert max(n for _s, _r, n, _a in res) > 10


def test_info_call_has_no_interval_cap():
    """qs_hip_read_split_device_batch_info needs no device: the 200 x 200-block gray scan of one interval that the
    interval route refuses is accepted, with the segments its workspace is sized for; the other refusals stay"""
    import jpegqs_pkg
    pkg = jpegqs_pkg.load()
    hip = pkg.HipQS()
    gray = hip.device_job([0x1000], [(200, 200)], [None], hsamp=[1], vsamp=[1], colorspace=1, image_size=(1600, 1600))
    o = hip.read_opts(dc_tbl=[0], ac_tbl=[0])
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.read_batch_info([gray], [o])
    assert e.value.code == -4
    per, nbytes = hip.read_batch_info([gray], [o], split=True)
    assert per[0]["intervals"] == 1 and per[0]["blocks_per_interval"] == 40000 and per[0]["mcus"] == 40000
    assert per[0]["max_segments"] > 40000 * 64 // SPLIT_BYTES and nbytes > 28 * per[0]["max_segments"]
    wide = hip.device_job([0x1000] * 3, [(8, 8)] * 3, [None] * 3, hsamp=[4, 2, 2], vsamp=[2, 2, 1], colorspace=3, image_size=(64, 64))
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.read_batch_info([wide], [hip.read_opts(dc_tbl=[0, 1, 1], ac_tbl=[0, 1, 1])], split=True)
    assert e.value.code == -4                                           # 14 blocks in an MCU
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.read_batch_info([gray], [hip.read_opts(dc_tbl=[2], ac_tbl=[0])], split=True)
    assert e.value.code == -2                                           # table 2 is not there
