"""The markers of a baseline JPEG file around one entropy-coded segment, as libjpeg 9 writes them for a fresh compress
object after jpeg_write_coefficients (jcmarker.c): SOI, JFIF APP0 or Adobe APP14, one DQT per component, SOF0 (SOF1
when a quantiser exceeds 8 bits), one DHT per table the scan uses, DRI when the scan has a restart interval, SOS, the
segment, EOI.  Host only, no device.

Conventions of the library's encoder (include/jpegqs_hip.h): component ci uses quant table ci and the Huffman tables
jpeg_set_colorspace assigns.  Extra markers of a source file (jcopy_markers) are not written."""
from __future__ import annotations

import struct

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                   61, 54, 47, 55, 62, 63])

# jpeg_set_colorspace: (component ids, Huffman table per component, JFIF header, Adobe transform or None)
COLORSPACES = {
    1: ((1,), (0,), True, None),
    2: ((0x52, 0x47, 0x42), (0, 0, 0), False, 0),
    3: ((1, 2, 3), (0, 1, 1), True, None),
    4: ((0x43, 0x4D, 0x59, 0x4B), (0, 0, 0, 0), False, 0),
    5: ((1, 2, 3, 4), (0, 1, 1, 0), False, 2),
}


def table_assignment(colorspace: int, ncomp: int):
    """the Huffman table (0 / 1) of each component"""
    if colorspace not in COLORSPACES or len(COLORSPACES[colorspace][0]) != ncomp:
        raise ValueError(f"{ncomp} components in colour space {colorspace}: no JPEG file layout for it")
    return COLORSPACES[colorspace][1]


def _marker(code: int, payload: bytes) -> bytes:
    return bytes([0xFF, code]) + struct.pack(">H", len(payload) + 2) + payload


def _dht(index: int, table) -> bytes:
    bits, huffval = table
    bits = [int(b) for b in bits]
    n = sum(bits[1:17])
    return _marker(0xC4, bytes([index]) + bytes(bits[1:17]) + bytes(int(v) for v in huffval[:n]))


def compose(segment: bytes, quants, hsamp, vsamp, colorspace: int, image_size, dc_tables, ac_tables,
            restart_interval: int = 0) -> bytes:
    """-> the whole file.  quants[ci]: 64 quantisers in natural order (None: all ones); dc_tables / ac_tables: the two
    (bits[17], huffval) pairs each; only the tables the components use are written.  restart_interval: the scan's
    interval in MCUs; libjpeg writes DRI behind the last DHT whenever it is not 0, also when it exceeds the MCU count"""
    if not 0 <= int(restart_interval) <= 65535:
        raise ValueError(f"restart_interval {restart_interval}: 0 .. 65535")
    n = len(quants)
    ids, tbl, jfif, adobe = COLORSPACES[colorspace][0], table_assignment(colorspace, n), *COLORSPACES[colorspace][2:]
    w, h = image_size
    out = [b"\xff\xd8"]
    if jfif:
        out.append(_marker(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])))
    if adobe is not None:
        out.append(_marker(0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, adobe)))
    wide = False
    for ci, q in enumerate(quants):
        q = np.ones(64, np.int64) if q is None else np.asarray(q, np.int64).reshape(64)
        prec = int(q.max() > 255)
        wide |= bool(prec)
        z = q[ZIGZAG]
        body = b"".join(struct.pack(">H", int(v)) for v in z) if prec else bytes(int(v) for v in z)
        out.append(_marker(0xDB, bytes([(prec << 4) | ci]) + body))
    sof = struct.pack(">BHHB", 8, h, w, n) + b"".join(bytes([ids[ci], (hsamp[ci] << 4) | vsamp[ci], ci]) for ci in range(n))
    out.append(_marker(0xC1 if wide else 0xC0, sof))
    sent = set()
    for ci in range(n):
        for is_ac, tabs in ((0, dc_tables), (1, ac_tables)):
            if (is_ac, tbl[ci]) not in sent:
                sent.add((is_ac, tbl[ci]))
                out.append(_dht((is_ac << 4) | tbl[ci], tabs[tbl[ci]]))
    if restart_interval:
        out.append(_marker(0xDD, struct.pack(">H", int(restart_interval))))
    sos = bytes([n]) + b"".join(bytes([ids[ci], (tbl[ci] << 4) | tbl[ci]]) for ci in range(n)) + bytes([0, 63, 0])
    out.append(_marker(0xDA, sos))
    out.append(bytes(segment))
    out.append(b"\xff\xd9")
    return b"".join(out)
