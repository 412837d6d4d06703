"""The byte formats of the case files the suite's stand-alone programs read and write (tests/host_tools.py runs them):
one packer and one parser for each.  All little-endian."""
import struct

import numpy as np

MAGIC = 0x51534A43


def header(n, w, h, colorspace) -> bytes:
    return struct.pack("<5i", MAGIC, n, w, h, colorspace)


def pack_image(im, quants=None) -> bytes:
    """the coefficient-image record (tests/libjpeg9_decode.c): the header, per component int32 width and height in
    blocks, hsamp, vsamp, 1 and its table (64 uint16; ones where there is none), then the arrays (int16)"""
    quants = im["quants"] if quants is None else quants
    parts = [header(len(im["coefs"]), im["image_size"][0], im["image_size"][1], im["colorspace"])]
    for ci, c in enumerate(im["coefs"]):
        q = np.ones(64, np.uint16) if quants[ci] is None else np.asarray(quants[ci], np.uint16)
        parts.append(struct.pack("<5i", c.shape[1], c.shape[0], im["hsamp"][ci], im["vsamp"][ci], 1))
        parts.append(q.tobytes())
    parts += [np.ascontiguousarray(c, np.int16).tobytes() for c in im["coefs"]]
    return b"".join(parts)


def parse_image(b, with_quants=True) -> dict:
    """the record back -> dict(coefs, [quants: None where the record says the component has no table,] hsamp, vsamp,
    colorspace, image_size)"""
    _, n, w, h, cs = struct.unpack_from("<5i", b, 0)
    off, geo, quants = 20, [], []
    for _c in range(n):
        geo.append(struct.unpack_from("<5i", b, off))
        quants.append(np.frombuffer(b, np.uint16, 64, off + 20).copy() if geo[-1][4] else None)
        off += 20 + 128
    coefs = []
    for wb, hb, _hs, _vs, _hq in geo:
        coefs.append(np.frombuffer(b, np.int16, wb * hb * 64, off).reshape(hb, wb, 64).copy())
        off += wb * hb * 128
    im = dict(coefs=coefs, quants=quants, hsamp=[g[2] for g in geo], vsamp=[g[3] for g in geo], colorspace=cs,
              image_size=(w, h))
    if not with_quants:
        del im["quants"]
    return im


def pack_blocks(coefs, tables):
    """the block record: int32 n, then per block 64 coefficients (int16) and 64 table entries (uint16; one table may
    serve every block) -> (n, bytes)"""
    coefs = np.asarray(coefs, np.int16).reshape(-1, 64)
    tables = np.broadcast_to(np.asarray(tables, np.uint16).reshape(-1, 64), coefs.shape)
    return len(coefs), struct.pack("<i", len(coefs)) + np.concatenate([coefs.view(np.uint16), tables], axis=1).tobytes()


# ---- the cases of the scan readers (tests/read_case.h) -------------------------------------------------------------------

def pad4(v):
    return list(v) + [0] * (4 - len(v))


def frame_words(p, shapes):
    """the 19 int32 every reader case starts with: ncomp, width, height, hsamp[4], vsamp[4], stride[4], rows[4]"""
    return [len(p["hsamp"]), p["image_size"][0], p["image_size"][1], *pad4(p["hsamp"]), *pad4(p["vsamp"]),
            *pad4([s[1] for s in shapes]), *pad4([s[0] for s in shapes])]


def pack_tables(s) -> bytes:
    """the 8-table record (DC 0..3, AC 0..3) of s["dc"] / s["ac"] = {index: (bits[17], huffval)}: uint8 present, bits[17],
    huffval[256]"""
    tabs = []
    for kind in ("dc", "ac"):
        for t in range(4):
            if t in s[kind]:
                bits, vals = s[kind][t]
                tabs.append(bytes([1]) + bytes(bits) + bytes(vals) + bytes(256 - len(vals)))
            else:
                tabs.append(bytes(1 + 17 + 256))
    return b"".join(tabs)


def parse_results(b, cases, words=1):
    """what a reader host wrote: per case `words` int32, the status first, and -- status >= 0 -- the arrays of
    c["shapes"] = [(rows, stride)] -> [(the words..., [int16 (rows, stride, 64)] or None)]"""
    out, off = [], 0
    for c in cases:
        head = struct.unpack_from(f"<{words}i", b, off)
        off += 4 * words
        arrs = None
        if head[0] >= 0:
            arrs = []
            for rows, stride in c["shapes"]:
                arrs.append(np.frombuffer(b, np.int16, rows * stride * 64, off).reshape(rows, stride, 64).copy())
                off += rows * stride * 128
        out.append((*head, arrs))
    assert off == len(b)
    return out
