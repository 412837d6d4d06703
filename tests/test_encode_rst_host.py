"""Restart intervals of the device entropy coder, without a GPU: the plain restatement of libjpeg 9's restart rules
(tests/encode_rst_oracle.py) against libjpeg 9 itself (tests/libjpeg9_encode.c) on every case the GPU module runs,
the DRI marker of jpeg_file.compose, the optimal tables of a restart scan, what the cases are there for, and the
qs_hip_encode_device_batch_info_opts bounds and argument checks."""
import numpy as np
import pytest

import jpegqs_pkg
import encode_rst_oracle as R
from encode_oracle import LibjpegError, BadCoef, encode_scan, histogram, synth_scan_image
from encode_rst_oracle import (LibJpeg9EncRst, encode_scan_rst, histogram_rst, interval_of, layout_cases, mcu_geometry,
                               parse_rst, scan_layout_rst, unit_facts, dc_range_images, optimize_cases)

pkg = jpegqs_pkg.load()
jpeg_file = pkg.jpeg_file


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    return LibJpeg9EncRst(tmp_path_factory.mktemp("lj9rst"))


@pytest.fixture(scope="module")
def hip():
    return pkg.HipQS()


@pytest.fixture(scope="module")
def std(hip):
    dc, ac = {t: tuple(hip.huff_standard(0, t)) for t in (0, 1)}, {t: tuple(hip.huff_standard(1, t)) for t in (0, 1)}
    R.set_standard_tables(dc, ac)
    return dc, ac


def _tbl(im):
    return jpeg_file.table_assignment(im["colorspace"], len(im["coefs"]))


def _job(hip, im):
    n = len(im["coefs"])
    return hip.device_job([0] * n, [c.shape[:2] for c in im["coefs"]], [None] * n, hsamp=im["hsamp"], vsamp=im["vsamp"],
                          colorspace=im["colorspace"], image_size=im["image_size"])


def test_restatement_and_composer_reproduce_libjpegs_file(hip, enc, std):
    """every layout x size x interval: the restated segment inside jpeg_file.compose's markers is libjpeg's file, DRI
    included; and info_opts bounds the segment"""
    dc, ac = std
    cases = layout_cases()
    assert len(cases) > 300
    markers = 0
    for name, im, ri, rows in cases:
        want = enc.write(im, ri, rows)
        Ri = interval_of(im, ri, rows)
        seg = encode_scan_rst(im, _tbl(im), dc, ac, Ri)
        f = parse_rst(want)
        assert seg == f["segment"], name
        assert f["dri"] == (Ri or None), name                      # DRI whenever Ri != 0, also beyond the MCU count
        got = jpeg_file.compose(seg, im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"], dc, ac,
                                restart_interval=Ri)
        assert got == want, name
        m = mcu_geometry(im)[1]
        n = 0 if Ri == 0 else -(-m // Ri) - 1
        assert sum(seg.count(bytes([0xFF, 0xD0 + k])) for k in range(8)) == n, name
        if Ri >= m:                                                 # no marker: the segment without an interval
            assert seg == encode_scan(im, _tbl(im), dc, ac), name
        markers += n
        per, _total = hip.encode_batch_info([_job(hip, im)], [(ri, rows)])
        assert len(seg) <= per[0]["max_segment_bytes"], name
    assert markers > 1000


def test_rows_are_counted_per_geometry_and_limited_to_16_bits(enc, std):
    """restart_in_rows wins over restart_interval; a row of more than 65535 MCUs is cut to 65535"""
    dc, ac = std
    im = synth_scan_image(np.random.default_rng(3), (141, 93), [2, 1, 1], [2, 1, 1], 3)
    f = parse_rst(enc.write(im, 5, 2))
    assert f["dri"] == 2 * 9 and f["segment"] == encode_scan_rst(im, _tbl(im), dc, ac, 18)
    assert interval_of(dict(im, image_size=(65500, 8), coefs=im["coefs"][:1], hsamp=[1], vsamp=[1]), 0, 9) == 65535


def test_more_than_eight_intervals_wrap_the_marker_number(enc, std):
    dc, ac = std
    im = synth_scan_image(np.random.default_rng(4), (141, 93), [2, 1, 1], [2, 1, 1], 3)       # 9 x 6 MCUs
    seg = encode_scan_rst(im, _tbl(im), dc, ac, 2)
    assert seg == parse_rst(enc.write(im, 2, 0))["segment"]
    raws = scan_layout_rst(im, _tbl(im), dc, ac, 2)["raw"]
    assert len(raws) == 27
    codes, pos = [], 0
    for k, raw in enumerate(raws[:-1]):                             # the two bytes behind each stuffed interval
        pos += len(R.stuff(raw))
        assert seg[pos] == 0xFF
        codes.append(seg[pos + 1])
        pos += 2
    assert codes == [0xD0 + (k & 7) for k in range(26)] and codes[8] == 0xD0 and codes[7] == 0xD7


def test_padding_cases_have_their_properties(enc, std):
    dc, ac = std
    im, Ri = R.padding_case()
    lay = scan_layout_rst(im, (0,), dc, ac, Ri)
    raws, bits = lay["raw"], lay["bits"]
    assert bits[1] % 8 == 0 and raws[1][-1] != 0xFF                 # PAD0
    assert bits[3] % 8 and raws[3][-1] == 0xFF                      # PAD_FF
    assert bits[5] % 8 == 0 and raws[5][-1] == 0xFF                 # DATA_FF
    assert bits[0] == 6 and raws[0] == b"\x2b"
    seg = encode_scan_rst(im, (0,), dc, ac, Ri)
    assert seg == parse_rst(enc.write(im, Ri, 0))["segment"]
    assert seg.count(b"\xff\x00\xff\xd3") == 1 and seg.count(b"\xff\x00\xff\xd5") == 1   # stuffed, then the marker
    assert raws[1] + b"\xff\xd1" in seg


def test_unit_case_has_its_properties(enc, std):
    dc, ac = std
    im, Ri = R.unit_case()
    raws = scan_layout_rst(im, (0,), dc, ac, Ri)["raw"]
    facts = unit_facts(raws)
    assert len(facts["on_unit"]) == 3 and len(facts["ff_before_unit"]) == 2
    k1, k2, k3 = facts["on_unit"]
    assert [facts["starts"][k] for k in (k1, k2, k3)] == [4096, 8192, 12288]
    lay = scan_layout_rst(im, (0,), dc, ac, Ri)
    assert lay["bits"][k2 - 1] % 8 and lay["bits"][k3 - 1] % 8 == 0                      # a padded 0xFF, a data 0xFF
    assert encode_scan_rst(im, (0,), dc, ac, Ri) == parse_rst(enc.write(im, Ri, 0))["segment"]


def test_dc_range_follows_the_interval(enc, std):
    dc, ac = std
    a, b = dc_range_images()
    assert parse_rst(enc.write(a, 0, 0))["segment"] == encode_scan(a, (0,), dc, ac)
    with pytest.raises(LibjpegError):
        enc.write(a, 2, 0)
    with pytest.raises(BadCoef):
        encode_scan_rst(a, (0,), dc, ac, 2)
    with pytest.raises(LibjpegError):
        enc.write(b, 0, 0)
    with pytest.raises(BadCoef):
        encode_scan(b, (0,), dc, ac)
    assert parse_rst(enc.write(b, 2, 0))["segment"] == encode_scan_rst(b, (0,), dc, ac, 2)


def test_optimal_tables_of_a_restart_scan(hip, enc, std):
    """libjpeg's optimize_coding file of a restart scan: its DHT tables are qs_hip_huff_optimal of the restart-aware
    histogram, they differ from the tables of the same arrays without restarts, and the whole file composes"""
    differ = 0
    for k, (im, ri, rows) in enumerate(optimize_cases()):
        want = enc.write(im, ri, rows, optimize=True)
        f = parse_rst(want)
        Ri = interval_of(im, ri, rows)
        tbl = _tbl(im)
        h = histogram_rst(im, tbl, Ri)
        dct = {t: tuple(hip.huff_optimal(h[t])) for t in sorted(set(tbl))}
        act = {t: tuple(hip.huff_optimal(h[2 + t])) for t in sorted(set(tbl))}
        for t in sorted(set(tbl)):
            assert (list(f["dc"][t][0]), list(f["dc"][t][1])) == (dct[t][0], dct[t][1]), f"case {k} DC {t}"
            assert (list(f["ac"][t][0]), list(f["ac"][t][1])) == (act[t][0], act[t][1]), f"case {k} AC {t}"
        seg = encode_scan_rst(im, tbl, dct, act, Ri)
        assert jpeg_file.compose(seg, im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"], dct, act,
                                 restart_interval=Ri) == want, f"case {k}"
        plain = histogram(im, tbl)
        assert not np.array_equal(plain[:2], h[:2]) and np.array_equal(plain[2:], h[2:])   # the DC counts move
        differ += any(tuple(hip.huff_optimal(plain[t])) != dct[t] for t in sorted(set(tbl)))
    assert differ == len(optimize_cases())


def test_info_opts_null_is_the_old_info(hip):
    ims = [im for _n, im, _ri, _rows in layout_cases()[::37]]
    jobs = [_job(hip, im) for im in ims]
    old = hip.encode_batch_info(jobs)
    assert hip.encode_batch_info(jobs, [None] * len(jobs)) == old
    assert hip.encode_batch_info(jobs, [(0, 0)] * len(jobs)) == old
    lib = hip.lib                                                    # opts == NULL itself
    import ctypes as C
    from jpeg_quantsmooth_amd import hipqs
    per = (hipqs.EncodeInfo * len(jobs))()
    total = C.c_size_t(0)
    assert lib.qs_hip_encode_device_batch_info_opts(hip._job_ptrs(jobs), len(jobs), None, per, C.byref(total)) == 0
    assert int(total.value) == old[1] and [int(p.max_segment_bytes) for p in per] == [o["max_segment_bytes"] for o in old[0]]
    big = hip.encode_batch_info(jobs, [(1, 0)] * len(jobs))
    for o, b, im in zip(old[0], big[0], ims):                       # at most 4 bytes per interval end
        assert b["max_segment_bytes"] == o["max_segment_bytes"] + 4 * (mcu_geometry(im)[1] - 1)
    assert big[1] >= old[1]


@pytest.mark.parametrize("opt", [(-1, 0), (65536, 0), (0, -1), (1 << 20, 1)])
def test_bad_options_are_einval(hip, opt):
    im = synth_scan_image(np.random.default_rng(1), (33, 9), [1], [1], 1)
    with pytest.raises(pkg.QsHipError) as e:
        hip.encode_batch_info([_job(hip, im)], [opt])
    assert e.value.code == -2
    with pytest.raises(pkg.QsHipError) as e:                        # prepare checks its arguments before it needs a device
        hip.encode_batch_prepare([_job(hip, im)], None, 256, 1 << 30, None, [opt])
    assert e.value.code == -2


def test_a_workspace_sized_for_other_options_is_einval(hip):
    """prepare_opts wants the size info_opts gives for the same options (checked before any device is touched)"""
    job = hip.device_job([0], [(1024, 1024)], [None], hsamp=[1], vsamp=[1], colorspace=1, image_size=(8192, 8192))
    _p0, plain = hip.encode_batch_info([job])
    _p1, rst = hip.encode_batch_info([job], [(1, 0)])
    assert rst > plain
    with pytest.raises(pkg.QsHipError) as e:
        hip.encode_batch_prepare([job], None, 256, plain, None, [(1, 0)])
    assert e.value.code == -2 and "workspace" in str(e.value)


def test_both_helpers_share_a_directory(enc, tmp_path):
    """the plain and the restart helper in one directory keep their staged inputs apart (both name them by process and
    count), which tools/bench_device_batch.py --encode --restart relies on: its host side stages once and writes often"""
    import sys
    from encode_oracle import LibJpeg9Enc, parse_jpeg
    im = synth_scan_image(np.random.default_rng(2), (40, 24), [2, 1, 1], [2, 1, 1], 3)
    plain, rst = LibJpeg9Enc(tmp_path), LibJpeg9EncRst(tmp_path)
    staged = plain.stage(im)
    want = rst.write(im, 2, 0)
    assert staged.exists() and parse_jpeg(plain.run(staged))["segment"] == parse_rst(enc.write(im, 0, 0))["segment"]
    sys.path.insert(0, str(R.HERE.parent / "tools"))
    import bench_device_batch as tool
    for restart, rows in ((None, None), (2, None), (None, 1)):
        helper, write = tool.host_writer(tmp_path, restart, rows)
        s = helper.stage(im)
        first = write(s)
        assert write(s) == first == enc.write(im, restart or 0, rows or 0)      # the staged input outlives a write
        assert parse_rst(first)["dri"] == (R.interval_of(im, restart or 0, rows or 0) or None)
    assert want == tool.host_writer(tmp_path, 2, None)[1](rst.stage(im))
