"""The optimal-table procedure of the device's table kernel without a GPU: csrc/qs_huff.h compiled for the host
(tests/huff_host.cpp), plain and under -fsanitize=address,undefined as a process of its own, against a chain-walking
restatement of libjpeg's jpeg_gen_optimal_table and against libjpeg 9's own optimized files; jpeg_file.compose_parts
against compose; and the refusals of the whole-file run, which need no device."""
import ctypes as C

import numpy as np
import pytest

import jpegqs_pkg
from decode_oracle import GOLD, LibJpeg9
from encode_oracle import GOLDEN, LAYOUTS, SIZES, LibJpeg9Enc, histogram, parse_jpeg, synth_scan_image
from encode_rst_oracle import LibJpeg9EncRst, histogram_rst, interval_of, optimize_cases, parse_rst
from huff_oracle import HuffHost, code_sizes, edge_histograms, libjpeg_optimal, seeded_histograms

pkg = jpegqs_pkg.load()
jpeg_file = pkg.jpeg_file


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("huff")
    return HuffHost(d), HuffHost(d, sanitize=True)


@pytest.fixture(scope="module")
def hip():
    return pkg.HipQS()


def _check(name, h, got):
    status, bits, vals, rest = got
    want = libjpeg_optimal(h)
    if want is None:
        assert status == 5 and bits == [0] * 17 and vals == [], name
    else:
        assert status == 0 and (bits, vals) == want, name
    assert not any(rest), f"{name}: huffval is not zero behind its symbols"


def test_edge_histograms_plain_and_under_sanitizers(hosts):
    """the lane procedure in its host form: both builds end clean (no report on stderr, exit 0) and agree"""
    plain, san = hosts
    edges = edge_histograms()
    hs = [h for _n, h in edges]
    a, b = plain.run(hs), san.run(hs)
    assert a == b
    for (name, h), got in zip(edges, b):
        _check(name, h, got)
    by = {name: got for (name, _h), got in zip(edges, b)}
    assert by["all zero"][:3] == (0, [0] * 17, [])
    assert by["one symbol"][:3] == (0, [0, 1] + [0] * 15, [37])
    assert by["two symbols"][:3] == (0, [0, 1, 1] + [0] * 14, [3, 200])
    # tests/test_encode_host.py derives it: 257 leaves, the 256 heavy ones equal -> 255 codes of 8 bits, one of 9
    assert by["256 equal"][:3] == (0, [0] * 8 + [255, 1] + [0] * 7, list(range(256)))
    assert by["all ones"][0] == 0 and by["all ones"][2] == list(range(256))
    assert by["all 2^32 - 1"][0] == 0 and sum(by["all 2^32 - 1"][1]) == 256
    sizes = {name: max(code_sizes(h)) for name, h in edges}
    assert 17 <= sizes["cut back"] <= 32 and by["cut back"][0] == 0 and by["cut back"][1][16] > 0
    assert sizes["above 32"] > 32 and by["above 32"][0] == 5


def test_two_thousand_seeded_histograms_equal_the_chain_walk(hosts):
    """the relabelling by tree representative gives the code sizes of libjpeg's others[] walk: small ties, sparse,
    exponential spreads, Fibonacci-like trees (code sizes up to 46), heavy-tailed counts"""
    plain, _san = hosts
    hs = seeded_histograms(2000, 20)
    deep = 0
    for k, (h, got) in enumerate(zip(hs, plain.run(hs))):
        _check(f"histogram {k}", h, got)
        deep += got[0] == 5
    assert deep > 20                                                  # the refusal is exercised too


def test_tables_equal_libjpegs_own_optimized_files(hosts, tmp_path_factory):
    plain, _san = hosts
    enc = LibJpeg9Enc(tmp_path_factory.mktemp("lj9enc"))
    rst = LibJpeg9EncRst(tmp_path_factory.mktemp("lj9rst"))
    lj9 = LibJpeg9(tmp_path_factory.mktemp("lj9"))
    cases = []
    for name in GOLDEN:
        im = lj9.read(GOLD / f"{name}.jpg")
        tbl = jpeg_file.table_assignment(im["colorspace"], len(im["coefs"]))
        cases.append((name, parse_jpeg(enc.write(im, optimize=True)), histogram(im, tbl), tbl))
    for k, (im, ri, rows) in enumerate(optimize_cases()):
        tbl = jpeg_file.table_assignment(im["colorspace"], len(im["coefs"]))
        cases.append((f"restart case {k}", parse_rst(rst.write(im, ri, rows, optimize=True)),
                      histogram_rst(im, tbl, interval_of(im, ri, rows)), tbl))
    hs, what = [], []
    for name, f, h, tbl in cases:
        for t in sorted(set(tbl)):
            for is_ac, tabs in ((0, f["dc"]), (1, f["ac"])):
                hs.append(h[2 * is_ac + t][:256])
                what.append((f"{name}: {'AC' if is_ac else 'DC'} table {t}", (list(tabs[t][0]), list(tabs[t][1]))))
    assert len(hs) >= 2 * (len(GOLDEN) + 4)
    for (name, want), (status, bits, vals, _rest) in zip(what, plain.run(hs)):
        assert status == 0 and (bits, vals) == want, name


def test_host_entry_point_on_nothing_counted(hip):
    """qs_hip_huff_optimal used to search for the longest length in use without a lower bound"""
    assert hip.huff_optimal(np.zeros(257, np.int64)) == ([0] * 17, [])
    one = np.zeros(257, np.int64)
    one[255] = 1
    assert hip.huff_optimal(one) == ([0, 1] + [0] * 15, [255])


def test_host_entry_point_equals_the_host_program(hosts, hip):
    plain, _san = hosts
    hs = seeded_histograms(100, 5) + [h for _n, h in edge_histograms()]
    for k, (h, (status, bits, vals, _rest)) in enumerate(zip(hs, plain.run(hs))):
        if status:
            with pytest.raises(pkg.hipqs.QsHipError) as e:
                hip.huff_optimal(h)
            assert e.value.code == -2, k
        else:
            assert hip.huff_optimal(h) == (bits, vals), k


def test_compose_parts_is_pinned_to_compose(hip):
    std = ({t: hip.huff_standard(0, t) for t in (0, 1)}, {t: hip.huff_standard(1, t) for t in (0, 1)})
    rng = np.random.default_rng(3)
    seg = bytes(rng.integers(0, 255, 57, dtype=np.uint8))
    sof1 = 0
    for li, (hs, vs, cs) in enumerate(LAYOUTS):
        for size in SIZES:
            n = len(hs)
            quants = [rng.integers(1, 256, 64).astype(np.uint16) for _ in range(n)]
            if (li + size[0]) % 3 == 0:
                quants[n - 1] = quants[n - 1] * 300                   # above 255: 16-bit DQT, SOF1
            for ri in (0, 1, 65535):
                whole = jpeg_file.compose(seg, quants, hs, vs, cs, size, std[0], std[1], restart_interval=ri)
                head, mid = jpeg_file.compose_parts(quants, hs, vs, cs, size, std[0], std[1], restart_interval=ri)
                assert head + mid + seg + b"\xff\xd9" == whole
                bare, mid2 = jpeg_file.compose_parts(quants, hs, vs, cs, size, restart_interval=ri)
                assert mid2 == mid and head.startswith(bare) and head[len(bare):len(bare) + 2] == b"\xff\xc4"
                assert b"\xff\xc4" not in bare
                assert bare + head[len(bare):] + mid + seg + b"\xff\xd9" == whole
                assert (b"\xff\xdd\x00\x04" + ri.to_bytes(2, "big") in mid) == (ri != 0) and mid.count(b"\xff\xda") == 1
                p = jpeg_file.parse(whole)
                assert p["restart_interval"] == ri and p["sof"] == (0xC1 if max(int(q.max()) for q in quants) > 255 else 0xC0)
                sof1 += p["sof"] == 0xC1
    assert sof1 > 0
    with pytest.raises(ValueError):
        jpeg_file.compose_parts([None], [1], [1], 1, (8, 8), dc_tables=std[0])
    with pytest.raises(ValueError):
        jpeg_file.compose_parts([None], [1], [1], 1, (8, 8), restart_interval=65536)


def test_refusals_of_the_new_calls_need_no_device(hip):
    """a null frame pointer with a non-zero length, variant 1 missing on a two-geometry job and a short scratch are
    QS_HIP_EINVAL before anything is enqueued"""
    def job(shapes, hs, vs, size, up=None):
        j = hip.device_job([0x1000 * (i + 1) for i in range(len(shapes))], shapes, [None] * len(shapes), hsamp=hs, vsamp=vs,
                           colorspace=3 if len(shapes) == 3 else 1, image_size=size)
        if up:
            j.up_wblk, j.up_hblk = up[1], up[0]
            j.coef_up[0], j.coef_up[1] = 0x10000, 0x20000
        return j

    gray = job([(12, 18)], [1], [1], (141, 93))
    ycc = job([(12, 18), (6, 9), (6, 9)], [2, 1, 1], [2, 1, 1], (141, 93), up=(12, 18))
    assert hip.encode_files_scratch_bytes(0) == 0
    need = hip.encode_files_scratch_bytes(2)
    assert need >= 2 * (4 * 257 * 4 + 544 * 4 + 1096 + 8 + 4) and need % 256 == 0
    assert hip.encode_files_scratch_bytes(33) > hip.encode_files_scratch_bytes(32)
    _per, wsbytes = hip.encode_batch_info([gray, ycc])
    ws, scratch, out, buf = 0x100000, 0x4000000, 0x8000000, 0xC000000
    full = hip.encode_frame(head=[(buf, 100), (buf, 100)], mid=[(buf, 14), (buf, 14)])

    def code(frames, d_stop=0x1000, scratch_bytes=need, d_scratch=scratch):
        with pytest.raises(pkg.hipqs.QsHipError) as e:
            hip.encode_batch_files([gray, ycc], frames, True, d_stop, [out, out + 0x100000], [1000, 1000], 0x2000, 0x3000,
                                   None, d_scratch, scratch_bytes, ws, wsbytes)
        return e.value.code

    nohead = hip.encode_frame(head=[None, None], mid=[(buf, 14), (buf, 14)])
    nohead.head_bytes[0] = 100                                        # a length, no bytes
    assert code([nohead, full]) == -2
    assert code([full, hip.encode_frame(head=[(buf, 100), None], mid=[(buf, 14), None])]) == -2     # variant 1 missing
    assert code([hip.encode_frame(head=[(buf, 100), None], mid=[None, None]), full]) == -2         # no SOS header at all
    assert code([full, full], scratch_bytes=need - 1) == -2
    assert code([full, full], d_scratch=scratch + 8) == -2
    assert code(None, d_scratch=None) == -2
    # what is left is in order: the call gets as far as looking for a device (or, with one, would run)
    if hip.device_count() <= 0:
        assert code([full, full]) == -1
        # one geometry only when d_stop is not given: variant 1 is not needed then
        assert code([full, hip.encode_frame(head=[(buf, 100), None], mid=[(buf, 14), None])], d_stop=None) == -1
        with pytest.raises(pkg.hipqs.QsHipError) as e:
            hip.huff_optimal_device(0x1000, 4, 0x2000, 0x3000)
        assert e.value.code == -1
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.huff_optimal_device(None, 4, 0x2000, 0x3000)
    assert e.value.code == -2
    assert C.sizeof(pkg.hipqs.EncodeFrame) == 48 and C.sizeof(pkg.hipqs.HuffTables) == 1096
