"""The three scan readers on files libjpeg 9 does not write, without a GPU: the writer of tests/foreign_files.py pinned
to libjpeg's own bytes, then its corpus -- table ids up to 3, Td != Ta, tables defined once, complete tables with 16-bit
codes, a DRI that changes between scans, zero pad bits, segments and fill bytes between scans, odd component ids, the
layouts the reader grids leave out -- through libjpeg 9's reader (the oracle: every file asserted clean), both parsers of
jpeg_file and the host builds of csrc/qs_read.h, qs_read_split.h and qs_read_prog.h, plain and under
-fsanitize=address,undefined; the split route's synchronisation rounds per file; and the stated limits as refusals."""
import numpy as np
import pytest

from encode_prog_oracle import LibJpeg9EncProg
from encode_rst_oracle import LibJpeg9EncRst
from foreign_files import (LONG_AC, foreign_ac_table, foreign_cases, foreign_dc_table, jpeg_file, read_cases, refused_case,
                           write_baseline, write_progressive)
from encode_oracle import derive, synth_scan_image
from read_oracle import LibjpegReader, ReadHost, build_grid, true_shapes
from read_prog_oracle import ReadProgHost
from read_split_oracle import SPLIT_ROUNDS, SplitHost, table_period


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("foreign")
    return LibJpeg9EncProg(d), LibJpeg9EncRst(d), LibjpegReader(d), d


@pytest.fixture(scope="module")
def specs(tools):
    return foreign_cases(tools[0], tools[1])


@pytest.fixture(scope="module")
def prog(tools, specs):
    return read_cases(tools[2], specs["prog"])                        # libjpeg reads every file clean, or this fails


@pytest.fixture(scope="module")
def base(tools, specs):
    return read_cases(tools[2], specs["base"], 1)


@pytest.fixture(scope="module")
def split_results(tools, base):
    return SplitHost(tools[3]).run(base)


def _compare(cases, arrays_of):
    for c, arrs in zip(cases, arrays_of):
        for ci, (a, w) in enumerate(zip(arrs, c["want"])):
            if not np.array_equal(a, w):
                bad = np.argwhere((a != w).any(axis=2))
                raise AssertionError(f"{c['name']}: component {ci} of shape {a.shape[:2]}: {len(bad)} blocks differ, "
                                     f"first at (by, bx) = {tuple(bad[0])}")


def test_writer_with_every_knob_at_its_default_writes_libjpegs_bytes(tools):
    """the tie to libjpeg before anything is built on the writer: a 4:2:0 and a gray image, with and without a restart
    interval, as libjpeg's progressive file of jpeg_simple_progression and as its optimize_coding baseline file"""
    enc_prog, enc_rst, _lj, _d = tools
    rng = np.random.default_rng(41)
    for im in (synth_scan_image(rng, (33, 18), [2, 1, 1], [2, 1, 1], 3), synth_scan_image(rng, (24, 16), [1], [1], 1)):
        script = jpeg_file.simple_progression(len(im["coefs"]), im["colorspace"])
        for ri in (0, 2):
            assert write_progressive(im, script, restart=ri)["data"] == enc_prog.write(im, script, ri, 0), (im["hsamp"], ri)
            assert write_baseline(im, restart=ri)["data"] == enc_rst.write(im, ri, 0, True), (im["hsamp"], ri)


def test_table_families():
    """complete, with 16-bit codes on the symbols every scan uses, the all-ones code unused, and another assignment per id"""
    seen = set()
    for t in range(4):
        bits, vals = foreign_ac_table(t)
        assert sorted(vals) == list(range(256)) and bits[2:9] == [1] * 7 and bits[9] == 240 and bits[16] == 9
        codes = derive((bits, vals))
        assert {s for s, (_c, l) in codes.items() if l == 16} == set(LONG_AC)
        assert max(c for c, l in codes.values() if l == 16) < 0xFFFF
        dbits, dvals = foreign_dc_table(t)
        assert sorted(dvals) == list(range(12)) and dbits[2:13] == [1] * 11 and dbits[16] == 1 and sum(dbits) == 12
        seen.add((tuple(vals), tuple(dvals)))
        for u in range(t):                                              # no symbol keeps its code from one id to another
            other, dother = derive(foreign_ac_table(u)), derive(foreign_dc_table(u))
            assert sum(codes[s] == other[s] for s in range(256)) == 0
            assert sum(derive((dbits, dvals))[s] == dother[s] for s in range(12)) == 0
    assert len(seen) == 4


def test_corpus_carries_what_libjpeg_never_writes(prog, base):
    def pairs(c):
        if c["kind"] == "base":
            return list(zip(c["header"]["dc_tbl"], c["header"]["ac_tbl"]))
        w = c["written"]
        return list(zip(w["dc_ids"], w["ac_ids"])) if w["scans"] is not None else []
    for cases in (prog, base):
        assert any(max(max(p) for p in pairs(c)) > 1 for c in cases if pairs(c))
        assert any(any(td != ta for td, ta in pairs(c)) for c in cases if pairs(c))
        assert any(len(c["header"]["hsamp"]) == 4 and sum(h * v for h, v in zip(c["header"]["hsamp"], c["header"]["vsamp"])) == 10
                   for c in cases)
    assert any(len({td for s in c["header"]["scans"] if s["ss"] == 0 and s["ah"] == 0 for td in s["dc_tbl"]}) == 4 for c in prog)
    # a table defined once and used by later scans, a DRI that moves and returns to 0, a 16-bit code in use
    assert any(c["fixed"] and c["data"].count(b"\xff\xc4") == 1 and len(c["header"]["scans"]) >= 10 for c in prog)
    assert any([s["restart_interval"] for s in c["header"]["scans"]][:5] == [2, 0, 5, 1, 0] for c in prog)
    assert any(c["header"]["sof"] == 0xC1 for c in base) and any(c["header"]["sof"] == 0xC0 for c in base)
    assert any(int(max(q.max() for q in c["header"]["quants"])) > 255 for c in prog)
    assert any(c["header"]["component_ids"] == [200, 7, 90] for c in prog)
    assert any(c["shapes"] != true_shapes(c["header"]) for c in prog) and any(c["shapes"] != true_shapes(c["header"]) for c in base)
    assert {table_period(c["header"]) for c in base} >= {1, 3, 6, 10}


def test_parsers_return_what_was_written(prog, base):
    """ids, per-scan tables, per-scan DRI, offsets, lengths and quantisers as the writer recorded them"""
    n = 0
    for c in prog + base:
        w, p = c["written"], c["header"]
        if w["scans"] is None:                                          # libjpeg's files: test_read_*_host.py covers them
            continue
        n += 1
        assert p["component_ids"] == w["component_ids"], c["name"]
        for q, qw in zip(p["quants"], w["quants"]):
            assert np.array_equal(q, qw), c["name"]
        if c["kind"] == "base":
            s, = w["scans"]
            got = dict(comps=list(range(len(p["hsamp"]))), ss=0, se=63, ah=0, al=0, dc_tbl=p["dc_tbl"], ac_tbl=p["ac_tbl"],
                       dc=p["dc"], ac=p["ac"], restart_interval=p["restart_interval"], offset=p["scan_offset"], length=s["length"])
            assert got == s, c["name"]
        else:
            assert p["scans"] == w["scans"], c["name"]
            assert p["script"] == [jpeg_file.scan(*s) for s in c["script"]], c["name"]
    assert n > 30


def test_progressive_corpus_on_the_host_build(tools, prog):
    """status 0 and libjpeg's arrays -- the dummy blocks of edge MCUs included in every third case"""
    res = ReadProgHost(tools[3]).run(prog)
    for c, (status, _levels, _a) in zip(prog, res):
        assert status == 0, (c["name"], status)
    _compare(prog, [a for _s, _l, a in res])


def test_baseline_corpus_on_both_host_builds_and_the_rounds_it_needs(tools, base, split_results):
    """the interval route: status 0 and libjpeg's arrays.  The split route: at most SPLIT_ROUNDS rounds wherever it reports
    0, libjpeg's arrays there, and status 4 everywhere else; its foreign table assignments need more rounds than any file
    of the readers' own grid (measured here on both, not written down)"""
    enc_prog, enc_rst, lj, d = tools
    res = ReadHost(d).run(base)
    for c, (status, _a) in zip(base, res):
        assert status == 0, (c["name"], status)
    _compare(base, [a for _s, a in res])
    print("split route: rounds needed / segments / table period")
    for c, (status, needed, nseg, arrs) in zip(base, split_results):
        print(f"  {needed:3d} {nseg:4d} {table_period(c['header']):3d}  status {status}  {c['name']}")
        if status == 0:
            assert 0 <= needed <= SPLIT_ROUNDS, c["name"]
            _compare([c], [arrs])
        else:
            assert status == 4, (c["name"], status)
    grid = build_grid(enc_rst, lj)
    grid_rounds = max(needed for _s, needed, _n, _a in SplitHost(d).run(grid))
    ours = max(needed for s, needed, _n, _a in split_results if s == 0)
    print(f"split route: {ours} rounds at most here, {grid_rounds} on the grid of read_oracle.build_grid, cap {SPLIT_ROUNDS}")
    assert ours > grid_rounds


def test_a_reader_that_picks_another_table_slot_never_reads_right(tools, prog, base):
    """what the per-id code assignments are for: the same files read with the Td or the Ta of two components exchanged in
    the header give a non-zero status or other arrays, never libjpeg's"""
    d = tools[3]
    c = next(c for c in base if c["name"].startswith("SOF0 4:2:0"))
    assert (c["header"]["dc_tbl"], c["header"]["ac_tbl"]) == ([2, 3, 0], [3, 1, 2])
    wrong = [dict(c, header=dict(c["header"], dc_tbl=[3, 2, 0])), dict(c, header=dict(c["header"], ac_tbl=[3, 2, 1]))]
    for w, (status, arrs) in zip(wrong, ReadHost(d).run(wrong)):
        assert status or not all(np.array_equal(a, x) for a, x in zip(arrs, c["want"]))
    for w, (status, _r, _n, arrs) in zip(wrong, SplitHost(d).run(wrong)):
        assert status or not all(np.array_equal(a, x) for a, x in zip(arrs, c["want"]))
    c = next(c for c in prog if c["name"] == "simple progression, Td (3,2,1) Ta (1,2,3)")
    scans = c["header"]["scans"]
    assert scans[0]["dc_tbl"] == [3, 2, 1] and scans[1]["ac_tbl"] == [1]
    wrong = [dict(c, header=dict(c["header"], scans=[dict(scans[0], dc_tbl=[2, 3, 1])] + scans[1:])),
             dict(c, header=dict(c["header"], scans=scans[:1] + [dict(scans[1], ac_tbl=[2])] + scans[2:]))]
    for w, (status, _l, arrs) in zip(wrong, ReadProgHost(d).run(wrong)):
        assert status or not all(np.array_equal(a, x) for a, x in zip(arrs, c["want"]))


def _sanitizer_slice(cases):
    return [c for c in cases if c["fixed"] or sum(h * v for h, v in zip(c["header"]["hsamp"], c["header"]["vsamp"])) == 10]


def test_fixed_table_cases_under_sanitizers(tools, prog, base, split_results):
    """the cases with the foreign tables and the frames of 10 blocks to the MCU through the three host builds with
    -fsanitize=address,undefined (stand-alone programs): no report, the same statuses and arrays"""
    d = tools[3]
    some = _sanitizer_slice(prog)
    assert len(some) >= 20
    res = ReadProgHost(d, sanitize=True).run(some)
    assert [s for s, _l, _a in res] == [0] * len(some)
    _compare(some, [a for _s, _l, a in res])
    some = _sanitizer_slice(base)
    assert len(some) >= 14
    res = ReadHost(d, sanitize=True).run(some)
    assert [s for s, _a in res] == [0] * len(some)
    _compare(some, [a for _s, a in res])
    plain = {c["name"]: r[0] for c, r in zip(base, split_results)}
    res = SplitHost(d, sanitize=True).run(some)
    assert [s for s, _r, _n, _a in res] == [plain[c["name"]] for c in some]
    ok = [k for k, r in enumerate(res) if r[0] == 0]
    _compare([some[k] for k in ok], [res[k][3] for k in ok])


def test_fill_byte_in_front_of_eoi_reads_on_the_host_build(tools, base):
    """jpeg_file.parse takes FF FF D9 behind the scan, as the kernels' rules do"""
    c, = [c for c in base if c["name"] == "FF in front of EOI"]
    assert c["data"].endswith(b"\xff\xff\xd9") and not c["data"].endswith(b"\x00\xff\xff\xd9")
    whole, head = jpeg_file.parse(c["data"]), jpeg_file.parse(c["data"], header_only=True)
    assert all(whole[k] == head[k] for k in ("scan_offset", "dc_tbl", "ac_tbl", "dc", "ac", "restart_interval", "image_size"))
    (status, arrs), = ReadHost(tools[3]).run([c])
    assert status == 0
    _compare([c], [arrs])


def test_stated_limits_are_refusals(tools, specs):
    """fill bytes in front of an RSTn: libjpeg reads the file clean, each parser says what it does not support, and a
    reader prepared on the intact file reports a status in 1 .. 3 -- never arrays.  An AC scan in front of its
    component's DC scan: libjpeg's decoder reads the file, the parser names the script rule and the scan"""
    _ep, _er, lj, d = tools
    builds = {san: (ReadHost(d, sanitize=san), SplitHost(d, sanitize=san), ReadProgHost(d, sanitize=san)) for san in (False, True)}
    for spec in specs["refused"]:
        parse = jpeg_file.parse_progressive if spec["kind"] == "prog" else jpeg_file.parse
        with pytest.raises(ValueError, match=spec["match"]) as e:
            parse(spec["data"])
        assert "more than one scan" not in str(e.value) and "marker expected" not in str(e.value), spec["name"]
        if spec["intact"] is None:
            ref, _clean = lj.read_bytes(spec["data"])
            assert ref is not None, spec["name"]
            continue
        c = refused_case(lj, spec)
        for san in (False, True):                                       # (the sanitizer builds: no report on these bytes)
            if spec["kind"] == "prog":
                (status, _l, _a), = builds[san][2].run([c])
                assert 1 <= status <= 3, (spec["name"], status)
            else:
                (s1, _a), = builds[san][0].run([c])
                (s2, _r, _n, _a), = builds[san][1].run([c])
                assert 1 <= s1 <= 3 and 1 <= s2 <= 3, (spec["name"], s1, s2)
    kinds = [(s["kind"], s["intact"] is None) for s in specs["refused"]]
    assert ("base", False) in kinds and ("prog", False) in kinds and ("prog", True) in kinds
