"""jpeg_file.parse, the inverse of jpeg_file.compose, on files libjpeg 9 wrote (tests/libjpeg9_encode.c): geometry,
tables, restart interval and quantisers equal what went in, compose(parse(...)) reproduces the header bytes, and every
form the device scan reader does not cover raises ValueError.  No device."""
import struct

import numpy as np
import pytest

import jpegqs_pkg
from decode_oracle import GOLD
from encode_oracle import LAYOUTS, SIZES, parse_jpeg, synth_scan_image
from encode_rst_oracle import RST_LAYOUTS, LibJpeg9EncRst, interval_of, parse_rst

pkg = jpegqs_pkg.load()
from jpeg_quantsmooth_amd import jpeg_file  # noqa: E402


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    return LibJpeg9EncRst(tmp_path_factory.mktemp("parse"))


@pytest.fixture(scope="module")
def std():
    hip = pkg.HipQS()
    return dict(dc={t: hip.huff_standard(0, t) for t in (0, 1)}, ac={t: hip.huff_standard(1, t) for t in (0, 1)})


def _valid(enc, li=4, size=(141, 93), ri=7):
    hs, vs, cs = LAYOUTS[li]
    im = synth_scan_image(np.random.default_rng(5), size, hs, vs, cs)
    return im, enc.write(im, ri, 0)


@pytest.mark.parametrize("li", RST_LAYOUTS)
def test_parse_inverts_compose_on_libjpeg_files(enc, std, li):
    hs, vs, cs = LAYOUTS[li]
    for size in SIZES:
        im = synth_scan_image(np.random.default_rng(li * 1000 + size[0]), size, hs, vs, cs)
        for optimize in (False, True):
            for ri, rows in ((0, 0), (1, 0), (7, 0), (65535, 0), (0, 1)):
                data = enc.write(im, ri, rows, optimize)
                p = jpeg_file.parse(data)
                what = (li, size, optimize, ri, rows)
                assert p["image_size"] == tuple(size) and p["colorspace"] == cs, what
                assert p["hsamp"] == list(hs) and p["vsamp"] == list(vs), what
                assert p["restart_interval"] == interval_of(im, ri, rows), what
                for q, want in zip(p["quants"], im["quants"]):
                    assert np.array_equal(q, want), what
                tbl = jpeg_file.table_assignment(cs, len(hs))
                assert p["dc_tbl"] == list(tbl) and p["ac_tbl"] == list(tbl), what
                other = parse_rst(data)                                  # the test suite's own marker walk
                assert p["scan_offset"] == len(other["head"]), what
                for kind in ("dc", "ac"):
                    assert sorted(p[kind]) == sorted(set(tbl)), what
                    for t in p[kind]:
                        bits, vals = p[kind][t]
                        assert (list(bits), list(vals)) == (list(other[kind][t][0]), list(other[kind][t][1])), what
                        if not optimize:
                            assert (list(bits), list(vals)) == (list(std[kind][t][0]), list(std[kind][t][1])), what
                again = jpeg_file.compose(b"", p["quants"], p["hsamp"], p["vsamp"], p["colorspace"], p["image_size"],
                                          p["dc"], p["ac"], p["restart_interval"])
                assert again[:p["scan_offset"]] == data[:p["scan_offset"]], what
                hp = jpeg_file.parse(data[:p["scan_offset"] + 3], header_only=True)
                assert hp["scan_offset"] == p["scan_offset"] and hp["dc"] == p["dc"], what


def test_sixteen_bit_quantisers(enc):
    hs, vs, cs = LAYOUTS[4]
    im = synth_scan_image(np.random.default_rng(9), (33, 9), hs, vs, cs)
    quants = [q.copy() for q in im["quants"]]
    quants[1][5] = 1000
    data = enc.write(im, 2, 0, quants=quants)
    p = jpeg_file.parse(data)
    assert p["sof"] == 0xC1 and int(p["quants"][1][5]) == 1000
    for q, want in zip(p["quants"], quants):
        assert np.array_equal(q, want)
    again = jpeg_file.compose(b"", p["quants"], p["hsamp"], p["vsamp"], p["colorspace"], p["image_size"], p["dc"], p["ac"], 2)
    assert again[:p["scan_offset"]] == data[:p["scan_offset"]]


def _raises(data, word, **kw):
    with pytest.raises(ValueError) as e:
        jpeg_file.parse(data, **kw)
    assert word in str(e.value), str(e.value)


def test_progressive_is_refused():
    data = (GOLD / "rgb120x88_prog.jpg").read_bytes()                 # written by libjpeg with a progressive scan script
    _raises(data, "progressive")
    _raises(data, "progressive", header_only=True)


def test_more_than_one_scan_is_refused(enc):
    _im, data = _valid(enc)
    p = jpeg_file.parse(data)
    off = p["scan_offset"]
    end = data.rindex(b"\xff\xd9")
    sos = data[data.rindex(b"\xff\xda", 0, off):off]
    dht = data[data.index(b"\xff\xc4"):]
    dht = dht[:2 + struct.unpack_from(">H", dht, 2)[0]]
    dqt = data[data.index(b"\xff\xdb"):]
    dqt = dqt[:2 + struct.unpack_from(">H", dqt, 2)[0]]
    _raises(data[:end] + sos + data[off:end] + data[end:], "second scan")
    _raises(data[:end] + dht + sos + data[off:end] + data[end:], "DHT")
    _raises(data[:end] + dqt + sos + data[off:end] + data[end:], "DQT")
    _raises(data[:end] + b"\xff\xdc\x00\x04\x00\x5d" + data[end:], "DNL")
    # a scan that carries one of the frame's three components: the others need scans of their own
    one = b"\xff\xda" + struct.pack(">H", 8) + bytes([1, 1, 0x00, 0, 63, 0])
    _raises(data[:off - len(sos)] + one + data[off:], "more than one scan")
    _raises(data[:off - len(sos)] + one + data[off:], "more than one scan", header_only=True)
    # a spectral selection or a successive approximation is not a sequential scan
    bad = bytearray(data)
    bad[off - 2] = 5
    _raises(bytes(bad), "sequential")


def test_twelve_bits_arithmetic_and_truncation_are_refused(enc):
    _im, data = _valid(enc)
    at = data.index(b"\xff\xc0")
    twelve = bytearray(data)
    twelve[at + 4] = 12
    _raises(bytes(twelve), "12-bit")
    arith = bytearray(data)
    arith[at + 1] = 0xC9
    _raises(bytes(arith), "arithmetic")
    p = jpeg_file.parse(data)
    _raises(data[:p["scan_offset"] - 5], "past the data", header_only=True)
    _raises(b"\x00" + data, "SOI")
