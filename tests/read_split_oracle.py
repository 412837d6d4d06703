"""What the tests of the split route of the device scan reader share (tests/test_read_split_host.py,
tests/test_gpu_read_split.py): the host build of csrc/qs_read_split.h (tests/read_split_host.cpp, compiled on demand in
its variants) and the corpus of valid files the number of synchronisation rounds was measured on (DESIGN.md section
14): the grid of tests/read_oracle.py, natural-statistics images at three qualities, RGB, CMYK and YCCK files, standard
and optimized tables."""
import numpy as np

from crafted_scans import ZIGZAG
from host_tools import build
from read_oracle import CaseHost, build_grid, make_case, pack_case, pkg

SPLIT_BYTES = 256                  # QS_RD_SPLIT_BYTES / QS_HIP_READ_SPLIT_BYTES
SPLIT_ROUNDS = 17                  # QS_RD_SPLIT_ROUNDS / QS_HIP_READ_SPLIT_ROUNDS


class SplitHost(CaseHost):
    """tests/read_split_host.cpp: qr_split_serial on the host.  rounds / nbytes: built with -DQS_RD_SPLIT_ROUNDS /
    -DQS_RD_SPLIT_BYTES"""
    PACK, WORDS = staticmethod(pack_case), 3

    def __init__(self, workdir, sanitize=False, rounds=None, nbytes=None):
        defines = [f"{k}={v}" for k, v in (("QS_RD_SPLIT_ROUNDS", rounds), ("QS_RD_SPLIT_BYTES", nbytes)) if v is not None]
        super().__init__(build("read_split_host.cpp", defines=defines, sanitize=sanitize), workdir)

    def run(self, cases, rounds=None):
        """cases as ReadHost.run takes them -> [(status, rounds needed or -1, segments, arrays or None)]; rounds: run
        that many synchronisation rounds instead of the build's constant"""
        return super().run(cases, *([rounds] if rounds is not None else []))


def table_period(header):
    """the smallest period of the table pairs (Td, Ta) over the blocks of an MCU"""
    n = len(header["hsamp"])
    pairs = []
    for ci in range(n):
        pairs += [(header["dc_tbl"][ci], header["ac_tbl"][ci])] * (header["hsamp"][ci] * header["vsamp"][ci] if n > 1 else 1)
    return next(p for p in range(1, len(pairs) + 1)
                if len(pairs) % p == 0 and all(pairs[i] == pairs[i - p] for i in range(p, len(pairs))))


def natural_image(w, h, hs, vs, quality, seed):
    y = pkg.synth.synth_ycc(w, h, hs, vs, quality=quality, seed=seed)
    return dict(coefs=y["coefs"], quants=y["quants"], hsamp=y["hsamp"], vsamp=y["vsamp"], colorspace=3, image_size=(w, h))


def recoloured(im, colorspace):
    """the arrays of a YCbCr 4:4:4 image as RGB (2), or with the first component once more as CMYK (4) / YCCK (5)"""
    coefs, quants = list(im["coefs"]), list(im["quants"])
    if colorspace in (4, 5):
        coefs.append(coefs[0])
        quants.append(quants[0])
    n = len(coefs)
    return dict(coefs=coefs, quants=quants, hsamp=[1] * n, vsamp=[1] * n, colorspace=colorspace, image_size=im["image_size"])


def natural_specs():
    """[(name, image, restart_interval, restart_in_rows, optimize)]: natural statistics at qualities 10, 50 and 90 in
    4:2:0 and 4:4:4, without markers and with one MCU row per interval, standard and optimized tables; the same
    statistics as RGB and CMYK (one table pair: p = 1) and YCCK (p = 4); 60 to 130 segments of 256 bytes at quality 90"""
    out = []
    for q in (10, 50, 90):
        for hs, name in ((2, "4:2:0"), (1, "4:4:4")):
            im = natural_image(259, 203, hs, hs, q, 7 * q + hs)
            for rows in (0, 1):
                for opt in (False, True):
                    out.append((f"natural q{q} {name} rows {rows}{' optimized' if opt else ''}", im, 0, rows, opt))
    base = natural_image(203, 131, 1, 1, 90, 5)
    for cs, name in ((2, "RGB"), (4, "CMYK"), (5, "YCCK")):
        for opt in (False, True):
            out.append((f"{name}{' optimized' if opt else ''}", recoloured(base, cs), 0, 0, opt))
    return out


def natural_cases(enc, lj):
    return [make_case(enc, lj, name, im, ri, rows, k, opt) for k, (name, im, ri, rows, opt) in enumerate(natural_specs())]


def split_corpus(enc, lj):
    """the valid corpus: the grid of tests/read_oracle.py (every layout and size without markers, with one MCU row per
    interval and with short intervals) and natural_cases"""
    return build_grid(enc, lj) + natural_cases(enc, lj)


def without_markers(case):
    """the case with its RSTn markers taken out and DRI 0 in the header the reader gets: the scan is then one interval
    that no longer decodes as the file (the predictions are not reset) -- for the corrupt corpus only"""
    scan = bytes(case["scan"])
    out, i = bytearray(), 0
    while i < len(scan):
        if scan[i] == 0xFF and i + 1 < len(scan) and 0xD0 <= scan[i + 1] <= 0xD7:
            i += 2
            continue
        out.append(scan[i])
        i += 1
    return dict(case, name=case["name"] + ", markers removed", scan=bytes(out), header=dict(case["header"], restart_interval=0))


# ---- what the bytes of a case hold ------------------------------------------------------------------------------------------

def intervals_of(scan):
    """[(start, end)] of the restart intervals of a scan: up to the first marker that is no RSTn, cut at the RSTn"""
    scan = bytes(scan)
    out, start, i = [], 0, 0
    while i < len(scan) - 1:
        if scan[i] == 0xFF and scan[i + 1] != 0:
            if 0xD0 <= scan[i + 1] <= 0xD7:
                out.append((start, i))
                start = i + 2
                i += 2
                continue
            return out + [(start, i)]
        i += 1
    return out + [(start, len(scan))]


def boundary_facts(case, nbytes=SPLIT_BYTES):
    """which of the situations the split route must get right the bytes of this case hold: a segment boundary on an FF,
    one on the 00 behind an FF, an interval shorter than a segment beside one of several, a last interval of one MCU"""
    scan, facts = bytes(case["scan"]), set()
    ivs = intervals_of(scan)
    for a, z in ivs:
        for p in range(a + nbytes, z, nbytes):
            if scan[p] == 0xFF:
                facts.add("boundary on FF")
            if scan[p] == 0 and scan[p - 1] == 0xFF:
                facts.add("boundary on the 00 behind FF")
    lens = [z - a for a, z in ivs]
    if any(n < nbytes for n in lens) and any(n > 2 * nbytes for n in lens):
        facts.add("short interval beside long ones")
    p = case["header"]
    n = len(p["hsamp"])
    w, h = p["image_size"]
    mh, mv = (max(p["hsamp"]), max(p["vsamp"])) if n > 1 else (1, 1)
    mcus = -(-w // (8 * mh)) * -(-h // (8 * mv))
    ri = p["restart_interval"]
    if ri and mcus > ri and mcus % ri == 1:
        facts.add("last interval of one MCU")
    return facts


# ---- crafted scans: gray, a scan written bit by bit -----------------------------------------------------------------------------

def canonical_codes(bits, vals):
    """{symbol: (code, length)} of a DHT table (bits[17], huffval), as JPEG Annex C assigns them"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


class BitWriter:
    """the entropy coder's byte stream: most significant bit first, 00 behind every FF, ones up to the byte at the end
    and in front of a marker"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        for i in range(nbits - 1, -1, -1):
            self.acc = (self.acc << 1) | ((value >> i) & 1)
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                if self.acc == 0xFF:
                    self.out.append(0)
                self.acc = self.n = 0

    def bit_position(self):
        """of the next bit, counted in the stuffed stream"""
        return 8 * len(self.out) + self.n

    def flush(self):
        while self.n:
            self.put(1, 1)

    def marker(self, code):
        self.flush()
        self.out += bytes([0xFF, code])


def value_bits(v):
    """(size, the bits jchuff.c writes for a value)"""
    s = abs(int(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1) & ((1 << s) - 1)


def crafted_gray_case(name, wb, hb, dc, ac, blocks, ri=0):
    """a gray case of wb x hb blocks whose scan is written here, not by libjpeg: dc / ac = (bits[17], huffval) of tables
    0; blocks[i] = (DC difference, [(run, value)] of the AC values in zigzag order, an EOB where the last lies in front
    of 63).  want: the arrays by construction -- DC the running sum from the interval's start, kept as libjpeg's int
    and stored as a short."""
    assert len(blocks) == wb * hb
    dcc, acc = canonical_codes(*dc), canonical_codes(*ac)
    w, want, pred, starts = BitWriter(), np.zeros((hb * wb, 64), np.int16), 0, []
    for i, (diff, acs) in enumerate(blocks):
        if ri and i and i % ri == 0:
            w.marker(0xD0 + (i // ri - 1) % 8)
            pred = 0
        s, b = value_bits(diff)
        starts.append((w.bit_position(), dcc[s][1] + s))
        w.put(*dcc[s])
        w.put(b, s)
        pred += diff
        want[i, 0] = np.int16(((pred + 32768) % 65536) - 32768)
        k = 0
        for run, v in acs:
            k += run + 1
            s, b = value_bits(v)
            starts.append((w.bit_position(), acc[(run << 4) | s][1] + s))
            w.put(*acc[(run << 4) | s])
            w.put(b, s)
            want[i, ZIGZAG[k]] = v
        if k < 63:
            w.put(*acc[0])
    w.flush()
    header = dict(image_size=(8 * wb, 8 * hb), hsamp=[1], vsamp=[1], colorspace=1, dc_tbl=[0], ac_tbl=[0],
                  restart_interval=ri, dc={0: dc}, ac={0: ac})
    return dict(name=name, header=header, scan=bytes(w.out) + b"\xff\xd9", shapes=[(hb, wb)], want=[want.reshape(hb, wb, 64)],
                symbols=starts)


def long_symbol_case():
    """an AC symbol of 31 bits -- a 16-bit code and 15 value bits -- that starts ten bits in front of the second
    segment: 1019 blocks of two bits (DC difference 0, EOB), then the block that holds it"""
    dc = ([0, 1, 1] + [0] * 14, [0, 5])
    ac_bits = [0] * 17
    ac_bits[1] = ac_bits[2] = ac_bits[3] = ac_bits[16] = 1
    ac = (ac_bits, [0x00, 0x01, 0x03, 0x0F])
    blocks = [(0, [])] * 1019 + [(0, [(0, 0x5A5A)])] + [(0, [(0, 1)]), (0, [(0, -5)])] * 10 + [(0, [])] * 560
    return crafted_gray_case("a 16-bit code with 15 value bits across a segment boundary", 40, 40, dc, ac, blocks)


def dc_wrap_cases():
    """DC differences of 15 bits, so that the running sum passes +-32768 many times inside a segment, from one segment
    to the next, and stands far from 0 where an interval ends: one interval, and intervals of 250 blocks (more than
    two segments each)"""
    dc_bits = [0] * 17
    dc_bits[1] = dc_bits[2] = dc_bits[3] = 1
    dc = (dc_bits, [0, 15, 14])
    ac = ([0, 1] + [0] * 15, [0x00])
    rng = np.random.default_rng(11)
    diffs = [int(v) for v in rng.choice([20000, 31000, -17000, 0, -9000], 600)]
    blocks = [(d, []) for d in diffs]
    return [crafted_gray_case("DC sums that wrap, one interval", 30, 20, dc, ac, blocks),
            crafted_gray_case("DC sums that wrap, intervals of 250 blocks", 30, 20, dc, ac, blocks, ri=250)]
