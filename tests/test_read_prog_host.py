"""The progressive route of the device scan reader without a GPU: csrc/qs_read_prog.h compiled for the host
(tests/read_prog_host.cpp) against libjpeg 9 at both ends -- files written by libjpeg (tests/libjpeg9_encode.c),
expected arrays read by libjpeg (tests/libjpeg9_decode.c) -- jpeg_file.parse_progressive on the same files, and the same
program under -fsanitize=address,undefined on a seeded corrupt corpus."""
import struct

import numpy as np
import pytest

from encode_prog_oracle import LibJpeg9EncProg
from encode_rst_oracle import LibJpeg9EncRst
from read_oracle import LibjpegReader, true_shapes
from read_prog_oracle import (ReadProgHost, build_grid, corpus_sources, corrupt_corpus, expected_arrays, jpeg_file,
                              libjpeg_reads)

# Files of the corrupt corpus libjpeg warns on while the restated rules cannot notice (DESIGN.md section 18 names the
# libjpeg rule behind each kind): none
LIBJPEG_ONLY = []


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("read_prog")
    return LibJpeg9EncProg(d), LibjpegReader(d), d


@pytest.fixture(scope="module")
def grid(tools):
    enc, lj, _d = tools
    return build_grid(enc, lj)


def compare(cases, results):
    for c, (status, _levels, arrs) in zip(cases, results):
        assert status == 0, (c["name"], status)
        for ci, (a, w) in enumerate(zip(arrs, c["want"])):
            if not np.array_equal(a, w):
                bad = np.argwhere((a != w).any(axis=2))
                raise AssertionError(f"{c['name']}: component {ci} of shape {a.shape[:2]}: {len(bad)} blocks differ, "
                                     f"first at (by, bx) = {tuple(bad[0])}: {a[tuple(bad[0])]} for {w[tuple(bad[0])]}")


def test_grid_equals_libjpeg(tools, grid):
    """every layout x size x script x restart interval, the crafted refinement images, the 32 768-block EOB run, the DC
    extremes under a point transform and the committed progressive file: status 0 and libjpeg's arrays for every block
    inside the array, the dummy blocks of edge MCUs by the interleaved DC scans' rule, 0 outside"""
    _enc, _lj, d = tools
    assert any(c["shapes"] != true_shapes(c["header"]) for c in grid), "no array larger than libjpeg's geometry"
    assert any(s["ah"] and s["ss"] for c in grid for s in c["header"]["scans"])
    assert any(s["ah"] and not s["ss"] for c in grid for s in c["header"]["scans"])
    results = ReadProgHost(d).run(grid)
    compare(grid, results)
    for c, (_s, levels, _a) in zip(grid, results):
        n, cs = len(c["header"]["hsamp"]), c["header"]["colorspace"]
        if c["script"] == jpeg_file.simple_progression(3, 3) and n == 3 and cs == 3:
            assert levels == 3, c["name"]
        if c["script"] == jpeg_file.spectral_script(n):
            assert levels == 1, c["name"]
        if n == 1 and "dc twice" in c["name"]:
            assert levels == 3, c["name"]
    assert any("dc twice" in c["name"] and len(c["header"]["hsamp"]) == 1 for c in grid)


def test_grid_under_sanitizers(tools, grid):
    """a slice of the valid grid through the sanitizer build: no report, the same arrays"""
    _enc, _lj, d = tools
    some = grid[::9] + [c for c in grid if c["name"].startswith("crafted")]
    compare(some, ReadProgHost(d, sanitize=True).run(some))


def test_parser_on_the_grid(grid):
    for c in grid:
        p, data = c["header"], c["data"]
        if c["image"] is not None:
            assert p["script"] == [jpeg_file.scan(*s) for s in c["script"]], c["name"]
        dc, ac, dri, pos, k = {}, {}, 0, 2, 0
        while data[pos + 1] != 0xD9:                                    # an independent walk over the markers
            assert data[pos] == 0xFF
            code, n = data[pos + 1], struct.unpack_from(">H", data, pos + 2)[0]
            body = data[pos + 4:pos + 2 + n]
            if code == 0xC4:
                q = 0
                while q < len(body):
                    cnt = sum(body[q + 1:q + 17])
                    (ac if body[q] & 0x10 else dc)[body[q] & 15] = ([0] + list(body[q + 1:q + 17]), list(body[q + 17:q + 17 + cnt]))
                    q += 17 + cnt
            if code == 0xDD:
                dri = struct.unpack(">H", body)[0]
            pos += 2 + n
            if code == 0xDA:
                s = p["scans"][k]
                k += 1
                assert s["offset"] == pos and s["dc"] == dc and s["ac"] == ac and s["restart_interval"] == dri, c["name"]
                pos += s["length"]                                       # offsets and lengths tile the file
                assert data[pos] == 0xFF and data[pos + 1] not in (0, *range(0xD0, 0xD8)), c["name"]
                assert not any(data[j] == 0xFF and data[j + 1] != 0 and not 0xD0 <= data[j + 1] <= 0xD7
                               for j in range(s["offset"], pos - 1)), c["name"]
        assert k == len(p["scans"]) and pos + 2 == len(data), c["name"]


def test_parser_refuses(tools, grid):
    enc, _lj, d = tools
    c = next(c for c in grid if len(c["header"]["hsamp"]) == 3 and c["image"] is not None)
    data, p = c["data"], c["header"]
    base = LibJpeg9EncRst(d).write(c["image"], 0, 0, False)
    with pytest.raises(ValueError, match="SOF0"):
        jpeg_file.parse_progressive(base)
    with pytest.raises(ValueError, match="EOI"):
        jpeg_file.parse_progressive(data[:-2])
    with pytest.raises(ValueError, match="EOI"):
        jpeg_file.parse_progressive(data[:p["scans"][3]["offset"] + 1])
    # without its first scan (the DC scan: its SOS header and its bytes) an AC scan precedes its component's DC
    first = p["scans"][0]
    cut = data[:first["offset"] - 8 - 2 * len(first["comps"])] + data[first["offset"] + first["length"]:]
    with pytest.raises(ValueError, match="scan 0: an AC scan before"):
        jpeg_file.parse_progressive(cut)
    sof = data.index(b"\xff\xc2")
    with pytest.raises(ValueError, match="12-bit"):
        jpeg_file.parse_progressive(data[:sof + 4] + b"\x0c" + data[sof + 5:])
    with pytest.raises(ValueError):
        jpeg_file.parse(data)                                           # parse keeps refusing SOF2


def test_corrupt_corpus_under_sanitizers(tools):
    """the host build with -fsanitize=address,undefined, as its own process: no report, every store inside the arrays
    (the program's guard margins: status -6), every status in 0..3, non-zero wherever libjpeg's own read of the file
    warns or stops; where both read it clean the arrays are equal"""
    enc, lj, d = tools
    corpus = corrupt_corpus(corpus_sources(enc, lj))
    assert len(corpus) > 3000
    results = ReadProgHost(d, sanitize=True).run(corpus)
    plain = ReadProgHost(d).run(corpus)
    assert [r[0] for r in results] == [r[0] for r in plain]
    both_clean, missed = 0, []
    for c, (status, _levels, arrs), (ref, clean) in zip(corpus, results, libjpeg_reads(lj, corpus)):
        assert status in (0, 1, 2, 3), (c["name"], status)
        if not clean:
            if status == 0:
                missed.append(c["name"])
        elif status == 0:
            both_clean += 1
            for a, w in zip(arrs, expected_arrays(ref, c["shapes"], c["header"]["script"])):
                assert np.array_equal(a, w), c["name"]
    print(f"corpus: {len(corpus)} cases, {both_clean} decode clean here and in libjpeg, {len(missed)} only here")
    assert missed == LIBJPEG_ONLY, missed
    assert len(LIBJPEG_ONLY) <= 0.01 * len(corpus)
