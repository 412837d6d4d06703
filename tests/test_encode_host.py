"""The device entropy coder's host side and its rules, without a GPU: a plain restatement of libjpeg 9's baseline scan
coder (tests/encode_oracle.py) against libjpeg 9 itself, the header composer, the optimal-table call and the range
limits."""
import numpy as np
import pytest

import jpegqs_pkg
from decode_oracle import GOLD, LibJpeg9
from encode_oracle import (GOLDEN, LAYOUTS, SIZES, BadCoef, LibJpeg9Enc, LibjpegError, encode_scan, histogram, parse_jpeg,
                           synth_scan_image)

pkg = jpegqs_pkg.load()
jpeg_file = pkg.jpeg_file


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    return LibJpeg9Enc(tmp_path_factory.mktemp("lj9enc"))


@pytest.fixture(scope="module")
def lj9(tmp_path_factory):
    return LibJpeg9(tmp_path_factory.mktemp("lj9"))


@pytest.fixture(scope="module")
def hip():
    return pkg.HipQS()


def std_tables(hip):
    return {t: tuple(hip.huff_standard(0, t)) for t in (0, 1)}, {t: tuple(hip.huff_standard(1, t)) for t in (0, 1)}


def layout_images():
    for li, (hs, vs, cs) in enumerate(LAYOUTS):
        for size in SIZES:
            yield f"{li}-{size[0]}x{size[1]}", synth_scan_image(np.random.default_rng(li * 1000 + size[0]), size, hs, vs, cs)


def all_images(lj9):
    yield from layout_images()
    for name in GOLDEN:
        yield name, lj9.read(GOLD / f"{name}.jpg")


def test_standard_tables_are_libjpegs(hip, enc):
    """the DHT markers libjpeg writes without optimize_coding hold the library's Annex K.3 tables"""
    im = synth_scan_image(np.random.default_rng(1), (16, 16), [2, 1, 1], [2, 1, 1], 3)
    f = parse_jpeg(enc.write(im))
    dc, ac = std_tables(hip)
    for t in (0, 1):
        assert (list(f["dc"][t][0]), list(f["dc"][t][1])) == (list(dc[t][0]), list(dc[t][1]))
        assert (list(f["ac"][t][0]), list(f["ac"][t][1])) == (list(ac[t][0]), list(ac[t][1]))


def test_restatement_reproduces_libjpegs_segment(hip, enc, lj9):
    """every layout x sizes that are not MCU multiples (dummy blocks), and the golden CLI images"""
    dc, ac = std_tables(hip)
    n = 0
    for name, im in all_images(lj9):
        f = parse_jpeg(enc.write(im))
        tbl = jpeg_file.table_assignment(im["colorspace"], len(im["coefs"]))
        assert encode_scan(im, tbl, dc, ac) == f["segment"], name
        n += 1
    assert n == len(LAYOUTS) * len(SIZES) + len(GOLDEN)


def test_composed_file_equals_libjpegs(hip, enc, lj9):
    """the header composer around libjpeg's own segment gives libjpeg's file, with standard and with optimized tables,
    8-bit and 16-bit quantisers"""
    dc, ac = std_tables(hip)
    for name, im in all_images(lj9):
        for optimize in (False, True):
            data = enc.write(im, optimize=optimize)
            f = parse_jpeg(data)
            dct, act = (f["dc"], f["ac"]) if optimize else (dc, ac)
            got = jpeg_file.compose(f["segment"], im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"],
                                    dct, act)
            assert got == data, f"{name} optimize={optimize}"
    im = synth_scan_image(np.random.default_rng(5), (24, 24), [1, 1, 1], [1, 1, 1], 3)
    im["quants"][1] = im["quants"][1].astype(np.uint16) * 300
    data = enc.write(im)
    f = parse_jpeg(data)
    assert jpeg_file.compose(f["segment"], im["quants"], im["hsamp"], im["vsamp"], 3, im["image_size"], dc, ac) == data


def _check_optimal(hip, f, h, tbl, name):
    for t in sorted(set(tbl)):
        for is_ac, tabs in ((0, f["dc"]), (1, f["ac"])):
            bits, vals = hip.huff_optimal(h[2 * is_ac + t])
            assert (bits, vals) == (list(tabs[t][0]), list(tabs[t][1])), f"{name}: {'AC' if is_ac else 'DC'} table {t}"


def test_optimal_tables_equal_libjpegs(hip, enc, lj9):
    """qs_hip_huff_optimal on the restatement's histograms against the DHT tables of optimize_coding"""
    for name, im in all_images(lj9):
        f = parse_jpeg(enc.write(im, optimize=True))
        tbl = jpeg_file.table_assignment(im["colorspace"], len(im["coefs"]))
        _check_optimal(hip, f, histogram(im, tbl), tbl, name)


def _gray_with_ac_symbols(symbols_and_counts):
    """a grayscale image whose AC histogram is exactly the given {run/size symbol: count} (plus EOB), DC all zero: one
    block per occurrence, the value at zigzag position run + 1"""
    from encode_oracle import ZIGZAG
    blocks = []
    for sym, cnt in symbols_and_counts.items():
        run, size = sym >> 4, sym & 15
        b = np.zeros(64, np.int16)
        b[ZIGZAG[run + 1]] = 1 << (size - 1)
        blocks += [b] * cnt
    n = len(blocks)
    w = min(n, 64)
    rows = -(-n // w)
    blocks += [blocks[-1]] * (rows * w - n)
    return dict(coefs=[np.array(blocks, np.int16).reshape(rows, w, 64)], quants=[np.ones(64, np.uint16)], hsamp=[1], vsamp=[1],
                colorspace=1, image_size=(8 * w, 8 * rows))


def _gray_packed(symbols_and_counts):
    """a grayscale image carrying about the given AC symbol counts, many symbols to a block (so EOB stays rare)"""
    from encode_oracle import ZIGZAG
    seq = [sym for sym, cnt in symbols_and_counts.items() for _ in range(cnt)]
    np.random.default_rng(7).shuffle(seq)
    blocks, b, k = [], np.zeros(64, np.int16), 1
    for sym in seq:
        run, size = sym >> 4, sym & 15
        if k + run > 63:
            blocks.append(b)
            b, k = np.zeros(64, np.int16), 1
        b[ZIGZAG[k + run]] = 1 << (size - 1)
        k += run + 1
    blocks.append(b)
    w = 64
    rows = -(-len(blocks) // w)
    blocks += [blocks[-1]] * (rows * w - len(blocks))
    return dict(coefs=[np.array(blocks, np.int16).reshape(rows, w, 64)], quants=[np.ones(64, np.uint16)], hsamp=[1], vsamp=[1],
                colorspace=1, image_size=(8 * w, 8 * rows))


# AC histograms libjpeg can be made to see (it never produces a symbol of more than 10 bits, so 160 run/size symbols
# plus EOB is the largest equiprobable alphabet; the full 256 are checked for their properties below)
DEGENERATE = {
    "one symbol": {0x01: 64},                       # (with EOB: two AC symbols)
    "two symbols": {0x01: 40, 0x12: 24},
    "equiprobable": {(r << 4) | s: 2 for r in range(16) for s in range(1, 11)},
    "skew": {((k // 10) << 4) | (k % 10 + 1): 1 << k for k in range(19)},                   # unlimited lengths pass 16
}


@pytest.mark.parametrize("case", sorted(DEGENERATE))
def test_optimal_tables_on_degenerate_histograms(hip, enc, case):
    im = (_gray_packed if case == "skew" else _gray_with_ac_symbols)(DEGENERATE[case])
    f = parse_jpeg(enc.write(im, optimize=True))
    h = histogram(im, (0,))
    if case == "skew":                              # Huffman's procedure alone would go past 16 bits here
        import heapq
        heap = [(int(c), 0) for c in h[2] if c] + [(1, 0)]
        heapq.heapify(heap)
        while len(heap) > 1:
            (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
            heapq.heappush(heap, (a + b, max(da, db) + 1))
        assert heap[0][1] > 16 and max(l for l in range(17) if f["ac"][0][0][l]) <= 16
    _check_optimal(hip, f, h, (0,), case)


def test_optimal_table_of_256_equiprobable_symbols(hip):
    """libjpeg cannot be fed this histogram (it refuses the values behind 96 of the symbols), so the expectation is
    derived here: with the reserved symbol there are 257 leaves of equal weight up to the reserved one's 1; a Huffman
    tree over 257 leaves whose 256 heavy ones are equal has depth 8 for 255 of them and depth 9 for two (2^9 - 257 = 255
    leaves fit one level up), the lighter reserved leaf among the two deepest; it then gives up its code, which leaves
    255 codes of 8 bits and one of 9.  Equal counts are listed by rising value."""
    import heapq
    heap = [(7, 0, s) for s in range(256)] + [(1, 0, 256)]          # an independent Huffman: (weight, depth, tie)
    depth = {}
    nodes = {s: [s] for s in range(257)}
    heapq.heapify(heap)
    nxt = 257
    while len(heap) > 1:
        (wa, _da, a), (wb, _db, b) = heapq.heappop(heap), heapq.heappop(heap)
        nodes[nxt] = nodes.pop(a) + nodes.pop(b)
        for s in nodes[nxt]:
            depth[s] = depth.get(s, 0) + 1
        heapq.heappush(heap, (wa + wb, 0, nxt))
        nxt += 1
    lengths = sorted(depth[s] for s in range(256))
    assert depth[256] == 9 and lengths == [8] * 255 + [9]
    bits, vals = hip.huff_optimal([7] * 256)
    assert [bits[l] for l in range(1, 17)] == [lengths.count(l) for l in range(1, 17)]
    assert vals == list(range(256))
    assert sum(b * 2 ** (16 - l) for l, b in enumerate(bits) if l) < 2 ** 16     # the all-ones code stays free


def test_a_dc_table_of_one_symbol(hip, enc):
    """every DC difference zero: the DC histogram has one symbol"""
    im = _gray_with_ac_symbols({0x01: 8})
    f = parse_jpeg(enc.write(im, optimize=True))
    assert hip.huff_optimal(histogram(im, (0,))[0]) == (list(f["dc"][0][0]), list(f["dc"][0][1]))


@pytest.mark.parametrize("ac,dcdiff,ok", [(1023, 0, True), (-1023, 0, True), (1024, 0, False), (-1024, 0, False),
                                          (0, 2047, True), (0, -2047, True), (0, 2048, False), (0, -2048, False)])
def test_range_limits(hip, enc, ac, dcdiff, ok):
    """libjpeg and the restatement accept and refuse the same values (JERR_BAD_DCT_COEF)"""
    dc, act = std_tables(hip)
    c = np.zeros((1, 3, 64), np.int16)
    c[0, 1, 5] = ac
    lo = -(abs(dcdiff) // 2) if dcdiff >= 0 else abs(dcdiff) // 2
    c[0, 1, 0], c[0, 2, 0] = lo, lo + dcdiff
    im = dict(coefs=[c], quants=[np.ones(64, np.uint16)], hsamp=[1], vsamp=[1], colorspace=1, image_size=(24, 8))
    if ok:
        assert encode_scan(im, (0,), dc, act) == parse_jpeg(enc.write(im))["segment"]
    else:
        with pytest.raises(LibjpegError):
            enc.write(im)
        with pytest.raises(BadCoef):
            encode_scan(im, (0,), dc, act)


def test_info_reports_tables_and_mcu_blocks(hip):
    job = hip.device_job([0, 0, 0], [(12, 18), (6, 9), (6, 9)], [None] * 3, hsamp=[2, 1, 1], vsamp=[2, 1, 1], colorspace=3,
                         image_size=(141, 93))
    per, total = hip.encode_batch_info([job])
    assert per[0]["dc_tbl"] == [0, 1, 1] and per[0]["ac_tbl"] == [0, 1, 1] and per[0]["blocks_in_mcu"] == [6, 6]
    assert per[0]["max_segment_bytes"] >= 9 * 6 * 6 * 208 and total > per[0]["max_segment_bytes"] // 2
    big = hip.device_job([0, 0, 0], [(8, 8)] * 3, [None] * 3, hsamp=[4, 2, 2], vsamp=[2, 1, 1], colorspace=3, image_size=(16, 16))
    with pytest.raises(pkg.QsHipError) as e:
        hip.encode_batch_info([big])                # 8 + 2 + 2 blocks in an MCU
    assert e.value.code == -4
