"""Every refusal rule of the three scan readers on a crafted stream of its own, without a GPU: the assembler of
tests/crafted_streams.py pinned to the bytes tests/foreign_files.py writes, then its cases -- per rule line of
csrc/qs_read.h, qs_read_split.h and qs_read_prog.h one file that trips that rule and nothing else, and an accepted twin
exactly on the boundary -- through libjpeg 9's reader (tests/golden/reader_rules.json records its verdicts) and the host
builds of the three headers, plain and under -fsanitize=address,undefined: the exact status of every case, libjpeg's
arrays for every twin.  That nothing else can produce the status is asserted on every file: a lenient decoder without
any of the rules reads every interval to its end and uses exactly its bits."""
import json
import re
import subprocess

import numpy as np
import pytest

from crafted_streams import (CODE, FIXTURE, LENGTH, OK, all_cases, baseline_blocks, digest, documented_limit, lenient_slack,
                             progressive_blocks, read_case, record, routes, rule_lines, write_baseline_items,
                             write_progressive_items)
from encode_oracle import synth_scan_image
from encode_refine_oracle import GRAY_REFINE, refine_scripts
from foreign_files import foreign_tables, jpeg_file, write_baseline, write_progressive
from read_oracle import CSRC, LibjpegReader, ReadHost
from read_prog_oracle import ReadProgHost
from read_split_oracle import SPLIT_BYTES, SplitHost

RULE = re.compile(r"return QS_RD_(CODE|LENGTH)|status = QS_RD_(CODE|LENGTH)")
HEADERS = ("qs_read.h", "qs_read_split.h", "qs_read_prog.h")


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("rules")
    return LibjpegReader(d), d


@pytest.fixture(scope="module")
def cases(tools):
    return [read_case(tools[0], c) for c in all_cases()]


def test_assembler_writes_the_bytes_of_foreign_files():
    """the tie before anything is built on the assembler: the items of a 4:2:0 and a gray image, block by block, give the
    files foreign_files writes for the same arrays and tables (which test_foreign_files_host.py ties to libjpeg's own
    bytes) -- baseline with and without a restart interval, progressive with first and refinement scans of both kinds"""
    rng = np.random.default_rng(43)
    simple = jpeg_file.simple_progression
    for im, scripts in ((synth_scan_image(rng, (33, 18), [2, 1, 1], [2, 1, 1], 3), list(refine_scripts(3, 3, simple).values())),
                        (synth_scan_image(rng, (24, 16), [1], [1], 1), [simple(1, 1), GRAY_REFINE])):
        n = len(im["coefs"])
        ids = jpeg_file.table_assignment(im["colorspace"], n)
        tables = foreign_tables(ids, ids)
        for ri in (0, 1, 2):
            assert write_baseline_items(im, baseline_blocks(im, ri), tables=tables, restart=ri)["data"] == \
                write_baseline(im, tables=tables, restart=ri)["data"], (n, ri)
            for script in scripts:
                scans = [progressive_blocks(im, s, ri) for s in script]
                assert write_progressive_items(im, script, scans, tables=tables, restart=ri)["data"] == \
                    write_progressive(im, script, tables=tables, restart=ri)["data"], (n, ri, script)


def test_every_rule_line_has_a_refused_case_and_every_refused_case_a_twin(cases):
    """the rule lines are read from the headers; a case names the lines it trips"""
    cited = set().union(*(rule_lines(c["rule"]) for c in cases))
    for h in HEADERS:
        for i, line in enumerate((CSRC / h).read_text().splitlines(), 1):
            if RULE.search(line):
                assert (h, i) in cited, f"{h}:{i} has no crafted case: {line.strip()}"
    by_name = {c["name"]: c for c in cases}
    assert len(by_name) == len(cases)
    for c in cases:
        assert (c["want_status"] != OK) == (c["rule"] is not None), c["name"]
        if c["want_status"] != OK:
            twin = by_name[c["twin"]]
            assert twin["want_status"] == OK and twin["kind"] == c["kind"], c["name"]
    for kind in ("base", "prog"):
        for place in ("first", "last") + (("dummy",) if kind == "base" else ()):
            assert any(c["name"].startswith(kind) and c["name"].endswith(place) and c["want_status"] == CODE for c in cases)
    assert any(c["name"].startswith("prog DC first: no code, dummy") for c in cases)


def test_no_other_rule_can_produce_the_status(cases):
    """isolation, without exceptions: the lenient decoder -- libjpeg's reading, none of the rules -- decodes every interval
    of every file to its end and has 0 .. 7 pad bits left; the two LENGTH forms have what they are about (8 bits left, one
    bit short) in the one interval they edit and nowhere else, their twins exactly 7 and 0"""
    for c in cases:
        slack = lenient_slack(c["data"], c["kind"])
        flat = [x for s in slack for x in s]
        if c["want_status"] == LENGTH:
            *where, bits = c["slack"]
            got = slack[where[0]][where[1]] if c["kind"] == "prog" else slack[0][where[0]]
            assert got == bits and sum(1 for x in flat if not 0 <= x <= 7) == 1, (c["name"], slack)
        else:
            assert all(0 <= x <= 7 for x in flat), (c["name"], slack)
        if "seven spare pad bits" in c["name"]:
            assert 7 in flat, c["name"]
        if "end on the byte boundary" in c["name"]:
            assert 0 in flat, c["name"]


def test_libjpegs_verdicts_are_the_recorded_ones(tools, cases):
    """tests/golden/reader_rules.json against libjpeg 9 read now: verdict and array digest of every file; every twin reads
    clean; a refused file libjpeg reads clean carries the paragraph of DESIGN.md that states the stricter status"""
    rows = json.loads(FIXTURE.read_text())
    assert rows == record(tools[0], documented_limit)
    design = " ".join((CSRC.parent.parent / "DESIGN.md").read_text().split())
    for row, c in zip(rows, cases):
        assert row["name"] == c["name"] and row["libjpeg"] == c["verdict"]
        if c["want_status"] == OK:
            assert c["verdict"] == "clean" and row["digest"] == digest(c["want"]), c["name"]
        elif c["verdict"] == "clean":
            assert row["documented"].startswith("DESIGN.md section"), c["name"]
            quoted = row["documented"].split("'", 1)[1].rsplit("'", 1)[0]
            assert " ".join(quoted.split()) in design, f"{c['name']}: DESIGN.md does not say: {quoted}"
    assert {r["libjpeg"] for r in rows} == {"clean", "warns"}
    assert any(r["libjpeg"] == "clean" and "EOB run" in r["name"] and r["status"]["progressive"] == CODE for r in rows)


def _same(c, arrs, what):
    for ci, (a, w) in enumerate(zip(arrs, c["want"])):
        assert np.array_equal(a, w), f"{c['name']}: {what}: component {ci} differs from libjpeg's"


@pytest.fixture(scope="module")
def sequential(tools, cases):
    """(the baseline cases, {sanitize: {route: results}}): each host build runs them once"""
    base, done = [c for c in cases if c["kind"] == "base"], {}

    def results(sanitize, route):
        if (sanitize, route) not in done:
            host = (ReadHost if route == "interval" else SplitHost)(tools[1], sanitize=sanitize)
            done[(sanitize, route)] = host.run(base)
        return done[(sanitize, route)]
    return base, results


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_interval_route_reports_the_exact_status(sequential, sanitize):
    """status 3, 2 or 0 as the fixture lists it -- not "non-zero"; libjpeg's arrays for every accepted file; under the
    sanitizers no report (the runner fails on one): every store inside exactly sized heap arrays"""
    rows = {r["name"]: r for r in json.loads(FIXTURE.read_text())}
    base, results = sequential
    for c, (s, a) in zip(base, results(sanitize, "interval")):
        assert s == rows[c["name"]]["status"]["interval"] == c["want_status"], (c["name"], s)
        if s == OK:
            _same(c, a, "interval route")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_split_route_reports_the_exact_status_and_agrees_with_the_interval_route(sequential, sanitize):
    """the same on the split route, and on every baseline case what the interval route reports: status and arrays; the
    cases made for it have their symbol on the boundary of two of several segments"""
    rows = {r["name"]: r for r in json.loads(FIXTURE.read_text())}
    base, results = sequential
    for c, (s, _needed, nseg, a), (s1, a1) in zip(base, results(sanitize, "split"), results(sanitize, "interval")):
        assert s == rows[c["name"]]["status"]["split"] == c["want_status"], (c["name"], s)
        assert s == s1, (c["name"], s, s1)
        if c["name"].startswith("split"):
            assert nseg >= 2 and len(c["scan"]) > SPLIT_BYTES, c["name"]
        if s == OK:
            _same(c, a, "split route")
            assert all(np.array_equal(x, y) for x, y in zip(a, a1)), c["name"]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_progressive_route_reports_the_exact_status(tools, cases, sanitize):
    """the same for the progressive route; the host program's guard margins around every array are intact (-6 otherwise)"""
    rows = {r["name"]: r for r in json.loads(FIXTURE.read_text())}
    prog = [c for c in cases if c["kind"] == "prog"]
    for c, (s, _levels, a) in zip(prog, ReadProgHost(tools[1], sanitize=sanitize).run(prog)):
        assert s == rows[c["name"]]["status"]["progressive"] == c["want_status"], (c["name"], s)
        if s == OK:
            _same(c, a, "progressive route")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_correction_bit_guard_at_block_level(tools, sanitize):
    """qrp_correct: a set bit moves a coefficient away from zero by p1 only where its bit Al is clear; one bit is taken
    either way.  No file validate_script accepts reaches the function with the bit set (a coefficient is refined only at
    Ah = its last Al, Al = Ah - 1: every non-zero value is then a multiple of 2 p1), so the guard is pinned here"""
    host = ReadProgHost(tools[1], sanitize=sanitize)
    triples = [(p1, c, byte) for p1 in (1, 2, 8) for c in (4 * p1, -4 * p1, 5 * p1, -5 * p1, 3 * p1, -p1, 32767, -32768 + p1)
               for byte in (0x80, 0x7F)]
    r = subprocess.run([str(host.exe), "correct"] + [str(x) for t in triples for x in t], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    want = [((c + (p1 if c >= 0 else -p1)) if byte & 0x80 and not c & p1 else c, 1) for p1, c, byte in triples]
    assert got == want
    assert any(c & p1 and byte & 0x80 for p1, c, byte in triples) and any(g[0] != c for g, (_p, c, _b) in zip(got, triples))


def test_fixture_names_the_routes_of_every_case():
    rows = json.loads(FIXTURE.read_text())
    for row in rows:
        assert set(row["status"]) in ({"interval", "split"}, {"progressive"}), row["name"]
        assert set(row["status"].values()) <= {OK, LENGTH, CODE}, row["name"]
    assert [routes(c) for c in all_cases()] == [tuple(r["status"]) for r in rows]
