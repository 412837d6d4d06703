"""libjpeg 9 as the oracle of the device entropy coder (tests/libjpeg9_encode.c, compiled on demand like the decode
oracle's helper), a parser of the files it writes, and a plain Python restatement of the baseline scan coder (test only:
it pins the scan-order rules of DESIGN.md section 13 against libjpeg before any GPU is involved)."""
import struct

import numpy as np

from decode_oracle import blocks_needed
from host_tools import Tool, build
from wire import pack_image

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63]


class LibjpegError(Exception):
    """libjpeg stopped with an error (exit status 3 of the helper)"""


class LibJpeg9Enc(Tool):
    """tests/libjpeg9_encode.c; its subclasses in encode_rst_oracle.py and encode_prog_oracle.py run the same program
    with restart intervals and with a scan script"""

    def __init__(self, workdir):
        super().__init__(build("libjpeg9_encode.c", libjpeg=True), workdir)

    def stage(self, im, quants=None):
        """the image dict as the helper's input file"""
        src = self.tmp(".bin")
        src.write_bytes(pack_image(im, quants))
        return src

    def _write(self, src, *args) -> bytes:
        """the program on a staged input, which stays: the file it makes, or LibjpegError when libjpeg refuses"""
        out = src.with_suffix(".jpg")
        try:
            r = self._run("write", src, out, *args, ok=(0, 3))
            if r.returncode == 3:
                raise LibjpegError(r.stderr.strip())
            return out.read_bytes()
        finally:
            out.unlink(missing_ok=True)

    def run(self, src, optimize=False) -> bytes:
        """the helper on a staged input: the file jpeg_write_coefficients makes; LibjpegError when libjpeg refuses"""
        return self._write(src, *(["optimize"] if optimize else []))

    def write(self, im, optimize=False, quants=None) -> bytes:
        """the file jpeg_write_coefficients makes of the image dict (coefs, quants, hsamp, vsamp, colorspace,
        image_size); LibjpegError when libjpeg refuses"""
        src = self.stage(im, quants)
        try:
            return self.run(src, optimize)
        finally:
            src.unlink()


def parse_jpeg(data: bytes) -> dict:
    """-> dict(head: the bytes up to and including the SOS header, segment: the entropy-coded bytes, tail,
    markers: [(code, payload)], dc / ac: {table index: (bits[17], huffval)})"""
    assert data[:2] == b"\xff\xd8"
    pos, markers, dc, ac = 2, [], {}, {}
    while True:
        assert data[pos] == 0xFF, f"marker expected at {pos}"
        code = data[pos + 1]
        n = struct.unpack_from(">H", data, pos + 2)[0]
        payload = data[pos + 4:pos + 2 + n]
        markers.append((code, payload))
        pos += 2 + n
        if code == 0xC4:
            p = 0
            while p < len(payload):
                idx = payload[p]
                bits = [0] + list(payload[p + 1:p + 17])
                cnt = sum(bits)
                (ac if idx & 0x10 else dc)[idx & 15] = (bits, list(payload[p + 17:p + 17 + cnt]))
                p += 17 + cnt
        if code == 0xDA:
            break
    end = pos
    while not (data[end] == 0xFF and data[end + 1] not in (0x00,)):
        end += 1
    return dict(head=data[:pos], segment=data[pos:end], tail=data[end:], markers=markers, dc=dc, ac=ac)


# ---- the restatement ---------------------------------------------------------------------------------------------------

class BadCoef(Exception):
    """JERR_BAD_DCT_COEF"""


def scan_blocks(im):
    """(component, block of 64 in natural order) in scan order, dummy blocks of edge MCUs included (jctrans.c:
    compress_output -- all AC zero, DC of the block before it in the MCU)"""
    coefs, hs, vs = im["coefs"], im["hsamp"], im["vsamp"]
    n = len(coefs)
    dims = [blocks_needed(im["image_size"], hs, vs, ci) for ci in range(n)]            # (height, width) in blocks
    if n == 1:
        for by in range(dims[0][0]):
            for bx in range(dims[0][1]):
                yield 0, coefs[0][by, bx]
        return
    w, h = im["image_size"]
    mh, mv = max(hs), max(vs)
    for my in range(-(-h // (8 * mv))):
        for mx in range(-(-w // (8 * mh))):
            last = None
            for c in range(n):
                for y in range(vs[c]):
                    for x in range(hs[c]):
                        bx, by = mx * hs[c] + x, my * vs[c] + y
                        if bx < dims[c][1] and by < dims[c][0]:
                            last = coefs[c][by, bx]
                        else:
                            d = np.zeros(64, np.int16)
                            d[0] = last[0]
                            last = d
                        yield c, last


def nbits(v):
    return int(abs(int(v))).bit_length()


def block_symbols(blk, prev_dc):
    """encode_one_block of jchuff.c -> [(is_ac, symbol, extra bits, number of extra bits)]"""
    out = []
    diff = int(blk[0]) - prev_dc
    nb = nbits(diff)
    if nb > 11:
        raise BadCoef(f"DC difference {diff}")
    out.append((0, nb, (diff if diff >= 0 else diff - 1) & ((1 << nb) - 1), nb))
    run = 0
    for k in range(1, 64):
        v = int(blk[ZIGZAG[k]])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((1, 0xF0, 0, 0))
            run -= 16
        nb = nbits(v)
        if nb > 10:
            raise BadCoef(f"AC value {v}")
        out.append((1, (run << 4) | nb, (v if v >= 0 else v - 1) & ((1 << nb) - 1), nb))
        run = 0
    if run:
        out.append((1, 0, 0, 0))
    return out


def scan_symbols(im, tbl):
    """every symbol of the scan: (is_ac, table, symbol, bits, nbits)"""
    prev = [0] * len(im["coefs"])
    for c, blk in scan_blocks(im):
        for is_ac, sym, bits, nb in block_symbols(blk, prev[c]):
            yield is_ac, tbl[c], sym, bits, nb
        prev[c] = int(blk[0])


def derive(table):
    """(bits, huffval) -> {symbol: (code, length)}"""
    bits, vals = table
    codes, code, p = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l]):
            codes[vals[p]] = (code, l)
            code += 1
            p += 1
        code <<= 1
    return codes


def histogram(im, tbl):
    """uint32[4][257] in the library's order: DC 0, DC 1, AC 0, AC 1"""
    h = np.zeros((4, 257), np.int64)
    for is_ac, t, sym, _bits, _nb in scan_symbols(im, tbl):
        h[2 * is_ac + t, sym] += 1
    return h


def encode_scan(im, tbl, dc_tables, ac_tables) -> bytes:
    """the entropy-coded segment: code words most significant bit first, padded with ones, 0x00 after every 0xFF"""
    dcc = {t: derive(v) for t, v in dc_tables.items()}
    acc = {t: derive(v) for t, v in ac_tables.items()}
    acc_bits, nacc, out = 0, 0, bytearray()
    for is_ac, t, sym, bits, nb in scan_symbols(im, tbl):
        code, size = (acc[t] if is_ac else dcc[t])[sym]
        acc_bits = (acc_bits << (size + nb)) | (code << nb) | bits
        nacc += size + nb
        while nacc >= 8:
            nacc -= 8
            b = (acc_bits >> nacc) & 0xFF
            out.append(b)
            if b == 0xFF:
                out.append(0)
        acc_bits &= (1 << nacc) - 1
    if nacc:
        b = ((acc_bits << (8 - nacc)) | ((1 << (8 - nacc)) - 1)) & 0xFF
        out.append(b)
        if b == 0xFF:
            out.append(0)
    return bytes(out)


# ---- inputs --------------------------------------------------------------------------------------------------------------

# (hsamp, vsamp, colorspace): gray, 1x1, 2x1, 1x2, 2x2, 4x1, RGB, 4 components (CMYK, YCCK with sampled chroma)
LAYOUTS = [([1], [1], 1), ([1, 1, 1], [1, 1, 1], 3), ([2, 1, 1], [1, 1, 1], 3), ([1, 1, 1], [2, 1, 1], 3),
           ([2, 1, 1], [2, 1, 1], 3), ([4, 1, 1], [1, 1, 1], 3), ([1, 1, 1], [1, 1, 1], 2), ([1, 1, 1, 1], [1, 1, 1, 1], 4),
           ([2, 1, 1, 2], [2, 1, 1, 2], 5), ([2, 1, 1], [2, 1, 1], 2)]
SIZES = [(8, 8), (141, 93), (67, 131), (200, 17), (33, 9)]
GOLDEN = ["gray64", "rgb141x93_420", "rgb128x96_420", "rgb141x93_444", "rgb120x88_422_rst", "cmyk96x64", "rgb120x88_prog"]


def synth_scan_image(rng, image_size, hsamp, vsamp, colorspace, amp=40, density=0.35):
    """random in-range arrays: DC a bounded random walk in raster order is not needed -- any two DC values in
    [-1000, 1000] differ by at most 11 bits"""
    coefs = []
    for ci in range(len(hsamp)):
        hb, wb = blocks_needed(image_size, hsamp, vsamp, ci)
        a = rng.integers(-amp, amp + 1, (hb, wb, 64))
        a[rng.random((hb, wb, 64)) > density] = 0
        a[rng.random((hb, wb)) < 0.1, 1:] = 0                                    # some blocks of DC alone
        a[..., 0] = rng.integers(-1000, 1001, (hb, wb))
        tail = rng.random((hb, wb)) < 0.3                                         # long zero runs, then a late value
        a[tail, 1:60] = 0
        a[tail, 63] = rng.integers(1, 1024, int(tail.sum()))
        coefs.append(a.astype(np.int16))
    quants = [rng.integers(1, 256, 64).astype(np.uint16) for _ in hsamp]
    return dict(coefs=coefs, quants=quants, hsamp=list(hsamp), vsamp=list(vsamp), colorspace=colorspace,
                image_size=tuple(image_size))


def block_bit_counts(im, tbl, dc_tables, ac_tables) -> list:
    """bits of each block of the scan, in scan order"""
    dcc = {t: derive(v) for t, v in dc_tables.items()}
    acc = {t: derive(v) for t, v in ac_tables.items()}
    prev, out = [0] * len(im["coefs"]), []
    for c, blk in scan_blocks(im):
        out.append(sum((acc[tbl[c]] if is_ac else dcc[tbl[c]])[sym][1] + nb for is_ac, sym, _b, nb in block_symbols(blk, prev[c])))
        prev[c] = int(blk[0])
    return out


def scan_bit_count(im, tbl, dc_tables, ac_tables) -> int:
    """bits of the scan before padding and stuffing"""
    return sum(block_bit_counts(im, tbl, dc_tables, ac_tables))
