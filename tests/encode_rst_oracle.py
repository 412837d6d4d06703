"""Restart intervals of the device entropy coder: libjpeg 9 as the oracle (tests/libjpeg9_encode.c, compiled on
demand), a plain Python restatement of the restart rules of jchuff.c / jcmaster.c / jcmarker.c on top of
tests/encode_oracle.py (test only: it pins the rules of DESIGN.md section 13 against libjpeg before any GPU is involved),
and the builders of the cases both test modules share."""
import struct

import numpy as np

from encode_oracle import LAYOUTS, SIZES, LibJpeg9Enc, block_symbols, derive, scan_blocks, synth_scan_image
from host_tools import HERE  # noqa: F401

SCHUNK = 4096                      # bytes of the unstuffed stream the stuffing stage takes per step (QS_ENC_SCHUNK)


class LibJpeg9EncRst(LibJpeg9Enc):
    """LibJpeg9Enc with cinfo.restart_interval / cinfo.restart_in_rows"""

    def run(self, src, ri=0, rows=0, optimize=False) -> bytes:
        """the helper on a staged input (stage()), which stays; LibjpegError when libjpeg refuses"""
        return self._write(src, int(ri), int(rows), *(["optimize"] if optimize else []))

    def write(self, im, ri=0, rows=0, optimize=False, quants=None) -> bytes:
        """the file jpeg_write_coefficients makes of the image dict with restart_interval = ri and restart_in_rows =
        rows; LibjpegError when libjpeg refuses"""
        src = self.stage(im, quants)
        try:
            return self.run(src, ri, rows, optimize)
        finally:
            src.unlink()


def parse_rst(data: bytes) -> dict:
    """encode_oracle.parse_jpeg for a file whose scan may hold RSTn markers -> dict(head: the bytes up to and including
    the SOS header, segment: the entropy-coded bytes with their RSTn markers, tail, markers: [(code, payload)], dc / ac:
    {table index: (bits[17], huffval)}, dri: the interval of the DRI marker or None)"""
    assert data[:2] == b"\xff\xd8"
    pos, markers, dc, ac, dri = 2, [], {}, {}, None
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
        if code == 0xDD:
            dri = struct.unpack(">H", payload)[0]
        if code == 0xDA:
            break
    end = pos
    while not (data[end] == 0xFF and data[end + 1] != 0x00 and not 0xD0 <= data[end + 1] <= 0xD7):
        end += 1
    return dict(head=data[:pos], segment=data[pos:end], tail=data[end:], markers=markers, dc=dc, ac=ac, dri=dri)


# ---- the restatement ---------------------------------------------------------------------------------------------------

def mcu_geometry(im):
    """(MCUs per row, MCUs in the scan, blocks per MCU); in a one-component scan an MCU is one block"""
    w, h = im["image_size"]
    hs, vs = im["hsamp"], im["vsamp"]
    if len(im["coefs"]) == 1:
        mx, my, bpm = -(-w // 8), -(-h // 8), 1
    else:
        mx, my, bpm = -(-w // (8 * max(hs))), -(-h // (8 * max(vs))), sum(a * b for a, b in zip(hs, vs))
    return mx, mx * my, bpm


def interval_of(im, ri=0, rows=0):
    """jcmaster.c per_scan_setup: restart_in_rows wins, counted in MCU rows and limited to 16 bits -> the scan's
    restart_interval (what DRI carries)"""
    if rows > 0:
        return min(rows * mcu_geometry(im)[0], 65535)
    return ri


def interval_symbols(im, tbl, Ri):
    """the scan's symbols by restart interval: [[(is_ac, table, symbol, bits, nbits) per symbol] per interval]; DC
    prediction starts at 0 in each (jchuff.c emit_restart_s).  Ri 0: one interval"""
    _mx, mcus, bpm = mcu_geometry(im)
    per = (Ri if Ri else mcus) * bpm
    out, prev = [], None
    for b, (c, blk) in enumerate(scan_blocks(im)):
        if b % per == 0:
            out.append([])
            prev = [0] * len(im["coefs"])
        out[-1] += [(is_ac, tbl[c], sym, bits, nb) for is_ac, sym, bits, nb in block_symbols(blk, prev[c])]
        prev[c] = int(blk[0])
    return out


def histogram_rst(im, tbl, Ri):
    """encode_oracle.histogram with the DC predictions a restart scan makes"""
    h = np.zeros((4, 257), np.int64)
    for syms in interval_symbols(im, tbl, Ri):
        for is_ac, t, sym, _bits, _nb in syms:
            h[2 * is_ac + t, sym] += 1
    return h


def stuff(raw: bytes) -> bytes:
    return raw.replace(b"\xff", b"\xff\x00")


def scan_layout_rst(im, tbl, dc_tables, ac_tables, Ri):
    """-> dict(raw: [the unstuffed bytes of each interval, its padding of one-bits included], bits: [the interval's bits
    before padding])"""
    dcc = {t: derive(v) for t, v in dc_tables.items()}
    acc = {t: derive(v) for t, v in ac_tables.items()}
    raws, lens = [], []
    for syms in interval_symbols(im, tbl, Ri):
        v, n = 0, 0
        for is_ac, t, sym, bits, nb in syms:
            code, size = (acc[t] if is_ac else dcc[t])[sym]
            v = (v << (size + nb)) | (code << nb) | bits
            n += size + nb
        pad = -n % 8
        v = (v << pad) | ((1 << pad) - 1)
        raws.append(v.to_bytes((n + pad) // 8, "big"))
        lens.append(n)
    return dict(raw=raws, bits=lens)


def compose_segment(raws) -> bytes:
    """each interval stuffed, FF D0+((k-1) & 7) unstuffed in front of interval k >= 1, none behind the last"""
    out = bytearray()
    for k, raw in enumerate(raws):
        if k:
            out += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
        out += stuff(raw)
    return bytes(out)


def encode_scan_rst(im, tbl, dc_tables, ac_tables, Ri) -> bytes:
    """the entropy-coded segment of a scan with restart interval Ri (MCUs; 0 or >= the MCU count: no marker)"""
    return compose_segment(scan_layout_rst(im, tbl, dc_tables, ac_tables, Ri)["raw"])


def unit_facts(raws):
    """where the intervals start in the unstuffed stream, for the cases about the stuffing stage's 4 KiB unit ->
    dict(starts: byte index of each interval, on_unit: intervals k >= 1 that start on a unit boundary, ff_before_unit:
    those of them whose preceding byte is 0xFF)"""
    starts, pos = [], 0
    for raw in raws:
        starts.append(pos)
        pos += len(raw)
    on_unit = [k for k in range(1, len(raws)) if starts[k] % SCHUNK == 0]
    return dict(starts=starts, on_unit=on_unit, ff_before_unit=[k for k in on_unit if raws[k - 1][-1] == 0xFF])


# ---- cases ---------------------------------------------------------------------------------------------------------------

# gray, 4:4:4, 4:2:0, 4:2:2, 4:4:0, 4:1:1, CMYK of encode_oracle.LAYOUTS
RST_LAYOUTS = [0, 1, 4, 2, 3, 5, 7]


def layout_cases():
    """[(name, image, restart_interval, restart_in_rows)]: every layout x every size of SIZES (edge MCUs with dummy
    blocks) x Ri in {1, 2, 7, MCUs per row, M - 1, M, M + 1, 65535} for M MCUs, and restart_in_rows in {1, 2}"""
    out = []
    for li in RST_LAYOUTS:
        hs, vs, cs = LAYOUTS[li]
        for size in SIZES:
            im = synth_scan_image(np.random.default_rng(li * 1000 + size[0]), size, hs, vs, cs)
            mx, m, _bpm = mcu_geometry(im)
            for ri in sorted({1, 2, 7, mx, m - 1, m, m + 1, 65535}):
                out.append((f"layout {li} at {size} Ri {ri}", im, ri, 0))
            for rows in (1, 2):
                out.append((f"layout {li} at {size} rows {rows}", im, 0, rows))
    return out


def gray_image(blocks, wb):
    """a grayscale image of the given blocks (64 values in natural order each), wb blocks to a row"""
    blocks = np.asarray(blocks, np.int16).reshape(-1, wb, 64)
    return dict(coefs=[blocks], quants=[np.ones(64, np.uint16)], hsamp=[1], vsamp=[1], colorspace=1,
                image_size=(8 * wb, 8 * blocks.shape[0]))


def literal_block(pairs):
    """{natural index: value} -> the block"""
    b = np.zeros(64, np.int16)
    for k, v in pairs.items():
        b[k] = v
    return b


# Blocks found by a seeded search with the restatement (standard tables, gray, Ri = 1: the block is an interval and its
# DC difference is its DC); tests/test_encode_rst_host.py asserts what each is here for.
#   PAD0       the interval's bits are a multiple of 8 and its last byte is not 0xFF
#   PAD_FF     a partial last byte whose data bits are all ones: the padded byte reads 0xFF and is stuffed
#   DATA_FF    a multiple of 8 bits whose last byte is 0xFF: data FF 00 right in front of the marker
PAD0 = {0: -9, 41: -748}                                            # 48 bits
PAD_FF = {0: 1, 1: 32, 63: 1023}                                    # 76 bits, the last four of them ones
DATA_FF = {1: 1, 63: 1023}                                          # 64 bits, the last ten of them ones
ZERO = {}                                                           # DC 0 and EOB: 6 bits, one byte (0x2B) when padded


def padding_case():
    """gray, Ri = 1: the three literal blocks between plain ones, each followed by a marker"""
    blocks = [literal_block(p) for p in (ZERO, PAD0, ZERO, PAD_FF, ZERO, DATA_FF, ZERO, ZERO)]
    return gray_image(blocks, 4), 1


def unit_case():
    """gray 128 x 100 blocks, Ri = 1: one-byte intervals up to the 4 KiB units of the unstuffed stream, so that a marker
    falls between two units -- after a plain byte at the first boundary, after a padded 0xFF at the second and after
    a data 0xFF at the third"""
    blocks, pos = [], 0
    for unit, last in ((1, ZERO), (2, PAD_FF), (3, DATA_FF)):
        n = len(scan_layout_rst(gray_image([literal_block(last)], 1), (0,), *_STD, 1)["raw"][0])
        fill = unit * SCHUNK - pos - n
        blocks += [literal_block(ZERO)] * fill + [literal_block(last)]
        pos = unit * SCHUNK
    blocks += [literal_block(ZERO)] * (128 * 100 - len(blocks))
    return gray_image(blocks, 128), 1


def dc_range_images():
    """(a) an interval-first DC of 12 bits behind a neighbour that keeps the difference in range: the no-restart scan
    accepts it, the restart scan refuses; (b) the mirror: a difference of 12 bits between two DCs of 11, across an
    interval boundary"""
    a = np.zeros((1, 4, 64), np.int16)
    a[0, :, 0] = [1000, 2000, 2100, 1500]
    b = np.zeros((1, 4, 64), np.int16)
    b[0, :, 0] = [100, -1100, 1100, 200]
    return gray_image(a.reshape(-1, 64), 4), gray_image(b.reshape(-1, 64), 4)


def optimize_cases():
    rng = np.random.default_rng(11)
    return [(synth_scan_image(rng, (141, 93), [2, 1, 1], [2, 1, 1], 3), 7, 0), (synth_scan_image(rng, (67, 131), [1], [1], 1), 1, 0),
            (synth_scan_image(rng, (141, 93), [2, 1, 1], [1, 1, 1], 3), 0, 1), (synth_scan_image(rng, (33, 9), [1, 1, 1, 1], [1, 1, 1, 1], 4), 2, 0)]


_STD = None


def set_standard_tables(dc, ac):
    """the standard tables the builders above code with (the library's qs_hip_huff_standard, set by the test modules)"""
    global _STD
    _STD = (dc, ac)
