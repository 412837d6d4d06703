"""The builders of tests/wide_cases.py against libjpeg 9, without a GPU: every tiling that tests/test_gpu_wide_offsets.py
expects at n of many thousands is libjpeg's whole file at n = 2, 3 and 5 (and at the GPU module's widths), the pattern
keeps the split route's synchronisation rounds far below its cap, and the host builds of the readers give the statuses
the GPU module expects of a truncated file."""
import re

import numpy as np
import pytest

import jpegqs_pkg
import wide_cases as W
from encode_prog_oracle import LibJpeg9EncProg
from encode_rst_oracle import LibJpeg9EncRst, parse_rst
from read_oracle import CSRC, LibjpegReader, ReadHost, expected_arrays, true_shapes
from read_prog_oracle import ReadProgHost
from read_split_oracle import SPLIT_ROUNDS, SplitHost

pkg = jpegqs_pkg.load()
jpeg_file = pkg.jpeg_file
NS = (2, 3, 5)
ONES = [np.ones(64, np.uint16)]


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("wide")
    return LibJpeg9EncRst(d), LibjpegReader(d), d


@pytest.fixture(scope="module")
def enc(tools):
    return tools[0]


@pytest.fixture(scope="module")
def pattern():
    return W.restart_pattern()


def _same(got: bytes, want: bytes, what):
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{what}: {len(got)} bytes, libjpeg {len(want)}; first difference at byte {at}")


def test_the_pattern_is_dense(enc, pattern):
    """about 230 bytes a block and every tenth byte stuffed: what the sizes of the GPU module are worked out from"""
    seg = parse_rst(enc.write(W.restart_image(pattern, 1, W.WB_SMALL), W.RI, 0))["segment"]
    assert 225 < len(seg) / W.PERIOD < 235
    assert 0.08 < seg.count(b"\xff\x00") / len(seg) < 0.12
    assert (np.abs(pattern[:, 1:]) >= 512).all() and (np.abs(pattern[:, 1:]) <= 1023).all()
    for k in range(7):
        assert seg.count(bytes([0xFF, 0xD0 + k])) == 1
    assert seg.count(b"\xff\xd7") == 0


@pytest.mark.parametrize("n", NS)
def test_restart_form_tiles_to_libjpegs_file(enc, pattern, n):
    one = enc.write(W.restart_image(pattern, 1, W.WB_SMALL), W.RI, 0)
    im = W.restart_image(pattern, n, W.WB_SMALL)
    t = W.tile_file(one, n, im["image_size"], restart=True)
    want = enc.write(im, W.RI, 0)
    _same(t.bytes(), want, f"restart form, n = {n}")
    assert len(t) == len(want)


def test_restart_form_at_the_gpu_modules_width(enc, pattern):
    """gray scan order does not depend on the width: the same unit at 1024 and 2560 block columns, where n is a multiple of
    4 and of 10"""
    one = enc.write(W.restart_image(pattern, 1, W.WB_SMALL), W.RI, 0)
    for wb, n in ((W.WB_BITS, 4), (W.WB_BITS, 12), (W.WB_BYTES, 10), (W.WB_BYTES, 30)):
        im = W.restart_image(pattern, n, wb)
        assert im["image_size"][0] == 8 * wb
        _same(W.tile_file(one, n, im["image_size"], restart=True).bytes(), enc.write(im, W.RI, 0), f"{wb} columns, n = {n}")


@pytest.mark.parametrize("wb", [W.WB_SMALL, W.WB_BYTES])
def test_no_restart_form_tiles_to_libjpegs_file(enc, wb):
    row = W.norestart_row(W.SEED, wb)
    one = enc.write(W.norestart_image(row, 1), 0, 0)
    for n in NS if wb == W.WB_SMALL else (2, 3):
        im = W.norestart_image(row, n)
        t = W.tile_file(one, n, im["image_size"], restart=False)
        _same(t.bytes(), enc.write(im, 0, 0), f"no-restart form, {wb} columns, n = {n}")


@pytest.mark.parametrize("n", NS)
def test_optimized_restart_form(enc, pattern, n):
    """counts of n patterns = n x counts of one; libjpeg's tables of them; one pattern coded under them and tiled"""
    counts, (dc, ac), seg = W.optimized_restart(pattern, n)
    im = W.restart_image(pattern, n, W.WB_SMALL)
    head, mid = jpeg_file.compose_parts(ONES, [1], [1], 1, im["image_size"], {0: dc, 1: dc}, {0: ac, 1: ac}, W.RI)
    t = W.Tiled(head + mid, seg.period, n, seg.cut, b"\xff\xd9")
    _same(t.bytes(), enc.write(im, W.RI, 0, optimize=True), f"optimized restart form, n = {n}")
    assert counts[0].sum() == W.PERIOD and counts[1].sum() == 63 * W.PERIOD


@pytest.mark.parametrize("wb", [W.WB_SMALL, 512])
def test_optimized_no_restart_form(enc, wb):
    row = W.norestart_row(W.SEED, wb)
    for n in NS:
        _counts, (dc, ac), seg = W.optimized_norestart(row, n)
        im = W.norestart_image(row, n)
        head, mid = jpeg_file.compose_parts(ONES, [1], [1], 1, im["image_size"], {0: dc, 1: dc}, {0: ac, 1: ac}, 0)
        t = W.Tiled(head + mid, seg.period, n, 0, b"\xff\xd9")
        _same(t.bytes(), enc.write(im, 0, 0, optimize=True), f"optimized no-restart form, {wb} columns, n = {n}")


@pytest.mark.parametrize("n", NS)
def test_progressive_dc_then_ac_tiles_scan_by_scan(tools, pattern, n):
    prog = LibJpeg9EncProg(tools[2])
    im = W.restart_image(pattern, n, W.WB_SMALL)
    head = jpeg_file.compose_parts(ONES, [1], [1], 1, im["image_size"], progressive=True)[0]
    parts = W.progressive_restart(pattern, n, head)
    _same(W.tiled_concat(parts), prog.write(im, W.DC_AC_SCRIPT, ri=W.RI), f"progressive, n = {n}")


@pytest.mark.parametrize("n", NS)
def test_progressive_with_a_short_scan_behind_the_long_one(tools, pattern, n):
    """[DC; AC 1..62; AC 63..63]: what the GPU module tiles until the last SOS lies past 2^31 bytes; the host build reads
    the tiled file, and the file cut inside its last scan has the status the GPU module expects"""
    prog = LibJpeg9EncProg(tools[2])
    im = W.restart_image(pattern, n, W.WB_SMALL)
    head = jpeg_file.compose_parts(ONES, [1], [1], 1, im["image_size"], progressive=True)[0]
    parts = W.progressive_tiled(pattern, n, head, W.DC_AC_AC_SCRIPT, W.RI)
    data = W.tiled_concat(parts)
    _same(data, prog.write(im, W.DC_AC_AC_SCRIPT, ri=W.RI), f"three scans, n = {n}")
    p = jpeg_file.parse_progressive(data)
    assert [s["offset"] for s in p["scans"]] == [sum(len(q) for q in parts[:k]) + len(parts[k].head) for k in range(3)]
    host = ReadProgHost(tools[2])
    (status, _levels, arrs), = host.run([dict(header=p, data=data, shapes=true_shapes(p))])
    assert status == 0 and np.array_equal(arrs[0], im["coefs"][0])
    if n >= 3:                                              # (at n = 2 the last scan is shorter than the cut)
        assert len(parts[2].period) // 8 < W.TRUNCATE // 8 and W.TRUNCATE < parts[2].body_len()    # whole intervals go
        (status, _levels, _arrs), = host.run([dict(header=p, data=data[:len(data) - W.TRUNCATE], shapes=true_shapes(p))])
        assert status == W.STATUS_TRUNCATED_SHORT_SCAN


@pytest.mark.parametrize("n", NS)
def test_simple_progression_tiles_scan_by_scan(tools, pattern, n):
    """libjpeg's own script for a gray frame (six scans, three of them refinements) on the dense pattern with restart
    interval 32: the refinement scans carry nothing but correction bits, cut into run pieces inside every interval"""
    prog = LibJpeg9EncProg(tools[2])
    script = jpeg_file.simple_progression(1, 1)
    assert sum(1 for s in script if s[3]) == 3
    im = W.restart_image(pattern, n, W.WB_SMALL)
    head = jpeg_file.compose_parts(ONES, [1], [1], 1, im["image_size"], progressive=True)[0]
    parts = W.progressive_tiled(pattern, n, head, script, W.RI)
    _same(W.tiled_concat(parts), prog.write(im, script, ri=W.RI), f"simple_progression, n = {n}")


@pytest.mark.parametrize("n", NS)
def test_refinement_script_with_restart_interval_1_tiles(tools, n):
    """DC, AC 1..63 at Al = 1 and its refinement, every block an interval: three tiled scans are libjpeg's file"""
    prog = LibJpeg9EncProg(tools[2])
    pattern = W.refine_pattern()
    im = W.gray_image(np.tile(pattern, (n, 1)), len(pattern))
    head = jpeg_file.compose_parts(ONES, [1], [1], 1, im["image_size"], progressive=True)[0]
    parts = W.progressive_tiled(pattern, n, head, W.GRAY_REFINE, 1)
    _same(W.tiled_concat(parts), prog.write(im, W.GRAY_REFINE, ri=1), f"refinement, n = {n}")


def test_the_refinement_patterns_weight():
    """every block of the pattern ends its band in zeros with its REFINE_TAILS bits buffered and writes nothing, so in a
    scan with restart interval 1 each block but the last adds tail + QR_CORR_MAX + 1 to the running sum, and the GPU
    module's n carries that sum past 2^32"""
    pattern = W.refine_pattern()
    assert (np.abs(pattern[:, 1:]) != 1).all()                     # no newly non-zero coefficient: no block writes
    pieces = W.run_pieces(W.gray_image(pattern, len(pattern)), W.GRAY_REFINE[2], 1)
    assert pieces == [(1, t) for t in W.REFINE_TAILS]
    assert int(re.search(r"#define QR_CORR_MAX (\d+)", (CSRC / "qs_encode_prog.h").read_text()).group(1)) + 1 == W.CORR_CUT
    assert W.refine_weight(pattern, 7) == 7 * sum(W.refine_block_weights(1)) - W.CORR_CUT
    n = W.refine_periods(pattern)
    assert n % (W.REFINE_WB // 8) == 0 and W.refine_weight(pattern, n) >= 1 << 32 > W.refine_weight(pattern, n // 2)
    assert W.refine_weight(pattern, 2) == 2 * (sum(W.REFINE_TAILS) + 8 * 938) - 938


@pytest.mark.parametrize("n", NS)
def test_refinement_script_without_restarts_tiles(tools, n):
    """the mirror: groups of a writing block and three blocks of 63 correction bits, no restart markers; the run pieces
    span the three blocks between two heads"""
    prog = LibJpeg9EncProg(tools[2])
    pattern = W.refine_norestart_pattern()
    im = W.gray_image(np.tile(pattern, (n, 1)), len(pattern))
    head = jpeg_file.compose_parts(ONES, [1], [1], 1, im["image_size"], progressive=True)[0]
    parts = W.progressive_tiled(pattern, n, head, W.GRAY_REFINE, 0)
    _same(W.tiled_concat(parts), prog.write(im, W.GRAY_REFINE, ri=0), f"refinement without restarts, n = {n}")
    assert W.run_pieces(im, W.GRAY_REFINE[2], 0) == [(3, 189)] * (8 * n)
    k = W.refine_periods(pattern, W.refine_weight_norestart)
    assert k % (W.REFINE_WB // 32) == 0 and W.refine_weight_norestart(pattern, k) >= 1 << 32
    assert W.refine_weight_norestart(pattern, 2) == 16 * (189 + 938) - 938 == 2 * sum(W.refine_block_weights(0)) - W.CORR_CUT
    w = W.refine_block_weights(0)
    assert W.wrap_block(w, k) % 4 == 0 and W.wrap_block(w, k) < 32 * k - 2 * 32767


# ---- the readers' side -------------------------------------------------------------------------------------------------------

def _case(lj, data, name):
    p = jpeg_file.parse(data)
    ref, clean = lj.read_bytes(data)
    shapes = true_shapes(p)
    return dict(name=name, data=data, header=p, scan=data[p["scan_offset"]:], shapes=shapes,
                want=None if ref is None else expected_arrays(ref, shapes), clean=clean)


def test_reading_a_tiled_file_gives_the_tiled_pattern(tools, pattern):
    """what the GPU module expects of the readers: the arrays of a tiled file are the pattern tiled (libjpeg's read,
    and the host builds of both routes)"""
    enc, lj, d = tools
    n = 3
    one = enc.write(W.restart_image(pattern, 1, W.WB_SMALL), W.RI, 0)
    im = W.restart_image(pattern, n, W.WB_SMALL)
    c = _case(lj, W.tile_file(one, n, im["image_size"]).bytes(), "restart form")
    assert c["clean"] and np.array_equal(c["want"][0], im["coefs"][0])
    (status, arrs), = ReadHost(d).run([c])
    assert status == 0 and np.array_equal(arrs[0], im["coefs"][0])
    row = W.norestart_row(W.SEED, W.WB_SMALL)
    one = enc.write(W.norestart_image(row, 1), 0, 0)
    im = W.norestart_image(row, n)
    c = _case(lj, W.tile_file(one, n, im["image_size"], restart=False).bytes(), "no-restart form")
    assert c["clean"] and np.array_equal(c["want"][0], im["coefs"][0])
    (status, _needed, _nseg, arrs), = SplitHost(d).run([c])
    assert status == 0 and np.array_equal(arrs[0], im["coefs"][0])


def split_rounds(tools, wb, n=4):
    enc, lj, d = tools
    row = W.norestart_row(W.SEED, wb)
    c = _case(lj, enc.write(W.norestart_image(row, n), 0, 0), f"no-restart form, {wb} columns")
    (status, needed, nseg, arrs), = SplitHost(d).run([c])
    assert status == 0 and np.array_equal(arrs[0], c["want"][0])
    return needed, nseg


@pytest.mark.parametrize("wb", [W.WB_SMALL, W.WB_BYTES])
def test_split_route_rounds_of_the_pattern(tools, wb):
    """a 4-period no-restart file of the chosen seed synchronises in at most W.SPLIT_ROUNDS_MEASURED rounds, against the
    cap of 17 (DESIGN.md sections 14.1 and 19.4): a status 4 in the GPU module would be a defect, not the pattern's doing"""
    needed, nseg = split_rounds(tools, wb)
    print(f"split route, {wb} columns: {nseg} segments, {needed} rounds")
    assert 0 <= needed <= W.SPLIT_ROUNDS_MEASURED <= (SPLIT_ROUNDS - 1) // 2
    assert nseg > 25 * wb                                  # 32 rows of 226-byte blocks in segments of 256 bytes


def test_truncated_files_on_the_host_builds(tools, pattern):
    """a file cut inside its last period: the statuses the GPU module expects of the same cut at its sizes"""
    enc, lj, d = tools
    n = 3
    one = enc.write(W.restart_image(pattern, 1, W.WB_SMALL), W.RI, 0)
    t = W.tile_file(one, n, W.restart_image(pattern, n, W.WB_SMALL)["image_size"])
    cut = t.bytes()[:len(t) - W.TRUNCATE]
    p = jpeg_file.parse(cut)
    c = dict(header=p, scan=cut[p["scan_offset"]:], shapes=true_shapes(p))
    (status, _arrs), = ReadHost(d).run([c])
    assert status == W.STATUS_TRUNCATED_INTERVALS
    row = W.norestart_row(W.SEED, W.WB_SMALL)
    one = enc.write(W.norestart_image(row, 1), 0, 0)
    t = W.tile_file(one, n, W.norestart_image(row, n)["image_size"], restart=False)
    cut = t.bytes()[:len(t) - W.TRUNCATE]
    p = jpeg_file.parse(cut)
    c = dict(header=p, scan=cut[p["scan_offset"]:], shapes=true_shapes(p))
    (status, _needed, _nseg, _arrs), = SplitHost(d).run([c])
    assert status == W.STATUS_TRUNCATED_SPLIT
    im = W.restart_image(pattern, n, W.WB_SMALL)
    head = jpeg_file.compose_parts(ONES, [1], [1], 1, im["image_size"], progressive=True)[0]
    data = W.tiled_concat(W.progressive_restart(pattern, n, head))
    p = jpeg_file.parse_progressive(data)
    host = ReadProgHost(d)
    (status, _levels, arrs), = host.run([dict(header=p, data=data, shapes=true_shapes(p))])
    assert status == 0 and np.array_equal(arrs[0], im["coefs"][0])
    (status, _levels, _arrs), = host.run([dict(header=p, data=data[:len(data) - W.TRUNCATE], shapes=true_shapes(p))])
    assert status == W.STATUS_TRUNCATED_PROGRESSIVE
