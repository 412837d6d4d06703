"""The arrays of tests/crafted_scans.py before any GPU is involved: their realised AC histograms give Huffman trees of
exactly the depths asked for (huff_oracle.code_sizes), libjpeg 9 itself writes the files up to depth 32 -- with the tables
of huff_oracle.libjpeg_optimal, cut back to 16 bits -- and refuses depth 33, and the host forms of the table procedure
(qs_hip_huff_optimal, tests/huff_host.cpp plain and under sanitizers as a process of its own) agree with it."""
import numpy as np
import pytest

import jpegqs_pkg
from crafted_scans import ac_histogram, dc_histogram, shared_deep_image
from encode_oracle import LibJpeg9Enc, LibjpegError, encode_scan, histogram, parse_jpeg
from huff_oracle import HuffHost, code_sizes, libjpeg_optimal

pkg = jpegqs_pkg.load()
jpeg_file = pkg.jpeg_file

SMALL = [(17, False), (22, False), (20, True)]                        # (depth, the three-component form with AC 1 deep)
LARGE = [(32, False), (33, False)]


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    return LibJpeg9Enc(tmp_path_factory.mktemp("lj9enc"))


@pytest.fixture(scope="module")
def hip():
    return pkg.HipQS()


def _deep_comps(ycc):
    return (1, 2) if ycc else (0,)


@pytest.mark.parametrize("depth,ycc", SMALL)
def test_small_arrays_against_the_restatement_and_libjpeg(enc, depth, ycc):
    im = shared_deep_image(depth, ycc)
    tbl = jpeg_file.table_assignment(im["colorspace"], len(im["coefs"]))
    assert tbl == ((0, 1, 1) if ycc else (0,))
    deep = 1 if ycc else 0
    assert im["image_size"][0] % 8 and im["image_size"][1] % 8
    assert all(np.array_equal(q, np.ones(64)) for q in im["quants"])
    want = histogram(im, tbl)
    h = ac_histogram(im, _deep_comps(ycc))
    assert np.array_equal(h, want[2 + deep][:256])
    assert np.array_equal(dc_histogram(im, _deep_comps(ycc)), want[deep][:16])
    if ycc:
        assert np.array_equal(ac_histogram(im, (0,)), want[2][:256])
        assert max(code_sizes(want[2][:256])) <= 16                 # AC 0 and both DC tables are ordinary
    assert max(code_sizes(h)) == depth
    assert h[0] > 0 and h[0xF0] == 0 and sum(h[s] > 0 for s in range(1, 11)) == 10 and sum(h[16:] > 0) == depth - 11
    f = parse_jpeg(enc.write(im, optimize=True))
    for t in sorted(set(tbl)):
        assert (list(f["dc"][t][0]), list(f["dc"][t][1])) == libjpeg_optimal(want[t][:256]), f"DC {t}"
        assert (list(f["ac"][t][0]), list(f["ac"][t][1])) == libjpeg_optimal(want[2 + t][:256]), f"AC {t}"
    assert f["ac"][deep][0][16] > 0 and sum(f["ac"][deep][0]) == depth
    assert encode_scan(im, tbl, f["dc"], f["ac"]) == f["segment"]


@pytest.fixture(scope="module")
def large():
    """{depth: (image, its realised AC histogram)}"""
    return {d: (shared_deep_image(d), ac_histogram(shared_deep_image(d))) for d, _ycc in LARGE}


def test_depth_32_is_written_and_33_refused_by_libjpeg_itself(enc, hip, large):
    (im32, h32), (im33, h33) = large[32], large[33]
    assert max(code_sizes(h32)) == 32 and max(code_sizes(h33)) == 33
    assert h32.max() > 3_000_000 and h33.max() > 3_000_000
    f = parse_jpeg(enc.write(im32, optimize=True))
    want = libjpeg_optimal(h32)
    assert (list(f["ac"][0][0]), list(f["ac"][0][1])) == want and want[0][16] > 0
    assert hip.huff_optimal(h32) == want
    with pytest.raises(LibjpegError, match="Huffman code size table out of bounds|overflow"):
        enc.write(im33, optimize=True)
    assert libjpeg_optimal(h33) is None
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.huff_optimal(h33)
    assert e.value.code == -2


def test_realised_histograms_through_the_host_program_plain_and_under_sanitizers(tmp_path_factory, large):
    """DC tables included; tests/huff_host.cpp as a process, and its -fsanitize=address,undefined build as another"""
    d = tmp_path_factory.mktemp("huff")
    plain, san = HuffHost(d), HuffHost(d, sanitize=True)
    hs, what = [], []
    for depth, ycc in SMALL + LARGE:
        im = shared_deep_image(depth, ycc)
        tables = [("AC 0", ac_histogram(im, (0,)) if ycc or depth not in large else large[depth][1], False),
                  ("DC 0", np.pad(dc_histogram(im, (0,)), (0, 240)), False)]
        if ycc:
            tables += [("AC 1", ac_histogram(im, (1, 2)), True), ("DC 1", np.pad(dc_histogram(im, (1, 2)), (0, 240)), False)]
        else:
            tables[0] = tables[0][:2] + (True,)
        for name, h, deep in tables:
            hs.append(h)
            what.append((f"depth {depth}{' ycc' if ycc else ''} {name}", depth if deep else None))
    a, b = plain.run(hs), san.run(hs)
    assert a == b
    for (name, depth), h, (status, bits, vals, rest) in zip(what, hs, a):
        assert not any(rest), name
        if depth is not None:
            assert max(code_sizes(h)) == depth, name
        if depth == 33:
            assert status == 5 and bits == [0] * 17 and vals == [], name
        else:
            assert status == 0 and (bits, vals) == libjpeg_optimal(h), name
            assert (bits[16] > 0) == (max(code_sizes(h)) > 16) == (depth is not None), name
