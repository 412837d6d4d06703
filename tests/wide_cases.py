"""Inputs that put the device stages past 2^31 and 2^32 bytes, bits and blocks while the oracle stays small (DESIGN.md
section 19), shared by tests/test_wide_cases.py (their proof against libjpeg 9 at small sizes, no GPU) and
tests/test_gpu_wide_offsets.py.

Two devices.  (1) A tiny image in a huge buffer: a row pitch or an array stride far beyond what the geometry needs puts
the last row or block past 2^32 bytes, and libjpeg 9 still decodes or codes the narrow image in milliseconds.  (2) A
periodic scan: dense blocks (every AC of 10 bits, about 230 bytes a block) repeated so that the bytes of the scan are one
short libjpeg result tiled n times.

  restart form     the scan order is n repetitions of a pattern of 8 restart intervals.  Every interval starts its DC
                   prediction at 0 and is padded to a byte, and RSTn has period 8, so with U = libjpeg's segment of one
                   pattern + FF D7 the segment of n patterns is U * n without its last two bytes.
  no-restart form  every block row is the same row, whose first and last DC are 0: each row then codes to the same bits,
                   8 rows to a whole number of bytes T (no padding inside), and 8 n rows to T * n.
  optimised        all periods being identical, the symbol counts of n periods are n times those of one, so libjpeg's
                   tables come from huff_oracle.libjpeg_optimal of the scaled counts and the restatements of
                   tests/encode_rst_oracle.py / tests/encode_prog_oracle.py code one period under them.
  progressive      the same scan by scan, each under its own tables (progressive_tiled), refinement scans included; two
                   patterns of +-2 / +-3 carry the refinement coder's running weight past 2^32 (refine_pattern with
                   restart interval 1, refine_norestart_pattern without restarts).

Nothing here touches a GPU; the tilers return the period and the count, and the GPU module repeats the period on the
device."""
import struct

import numpy as np

from encode_oracle import ZIGZAG, block_symbols, derive
from encode_prog_oracle import scan_symbols_prog
from encode_refine_oracle import CORR_MAX, GRAY_REFINE, run_pieces, scan_symbols_refine
from encode_rst_oracle import compose_segment, gray_image, parse_rst, stuff
from huff_oracle import libjpeg_optimal

RI = 32                            # restart interval of the restart form, in blocks (gray: MCUs)
PERIOD = 8 * RI                    # blocks of one pattern: 8 intervals, the period of RSTn
SEED = 19                          # the dense pattern every long-scan case uses (split-route rounds: DESIGN.md 19.4)
# block columns: the CPU proof's narrow image, and the two sizes of the GPU module, 8192 and 20 480 pixels wide.  The coders
# take frames of up to 65 500 rows, 8187 block rows: a scan of 2^32 bytes under the standard tables (229 bytes a block) needs
# 18.8 M blocks, and one of 2^32 bits under optimal tables, which give the one AC symbol of the pattern a code of one bit
# (87 bytes a block), 6.1 M
WB_SMALL, WB_BITS, WB_BYTES = 16, 1024, 2560
BITS, BYTES = 1 << 32, 1 << 32     # the two thresholds: bits of a scan, bytes of a scan
SLACK = 1.005                      # how far above a threshold the long cases go
# the most synchronisation rounds the split route needs on a no-restart file of SEED at any of the widths above
# (tests/test_wide_cases.py measures them on the host build); the cap is 17
SPLIT_ROUNDS_MEASURED = 6
# a file that lacks its last TRUNCATE bytes, cut inside the last period: status 2 of the three routes, "an interval with too
# few bytes" (asserted on the host builds at n = 3)
TRUNCATE = 1000
STATUS_TRUNCATED_INTERVALS = STATUS_TRUNCATED_SPLIT = STATUS_TRUNCATED_PROGRESSIVE = 2
# in the scan 63..63 of DC_AC_AC_SCRIPT an interval has 46 bytes, so the same cut takes 21 whole intervals and their markers
# away: status 1, "the RSTn markers of a scan do not fit its interval" (the host build at n = 3 and 5)
STATUS_TRUNCATED_SHORT_SCAN = 1


def dense_blocks(seed, count, dc_range=200):
    """blocks whose 63 AC values all have 10 bits (+-512..1023): the densest a baseline block gets short of the longest
    codes, about 230 bytes each under the standard tables, with about every tenth byte of the scan a stuffed FF 00"""
    rng = np.random.default_rng(seed)
    b = np.empty((count, 64), np.int16)
    b[:, 1:] = rng.integers(512, 1024, (count, 63)) * rng.choice(np.array([-1, 1]), (count, 63))
    b[:, 0] = rng.integers(-dc_range, dc_range + 1, count)
    return b


def restart_pattern(seed=SEED):
    """the PERIOD blocks of the restart form"""
    return dense_blocks(seed, PERIOD)


def restart_image(pattern, n, wb):
    """gray, wb block columns: the pattern n times in scan order (n * PERIOD must fill whole block rows)"""
    assert (n * len(pattern)) % wb == 0, (n, wb)
    return gray_image(np.tile(pattern, (n, 1)), wb)


def norestart_row(seed, wb):
    """one block row of the no-restart form: dense blocks, DC 0 at both ends, and the last coefficient (63 in zigzag and
    in natural order) 0, so that every block ends with an EOB.  The EOB is for the split route of the reader: its
    segments agree on the zigzag index only where a block ends for every decoder, and blocks of 63 non-zero values
    have no such place -- four periods of them need 15 of the 17 rounds at 16 columns and end with status 4 at 2304
    (DESIGN.md section 19.4).  With the EOB they need 6."""
    row = dense_blocks(seed, wb)
    row[0, 0] = row[-1, 0] = 0
    row[:, 63] = 0
    return row


def norestart_image(row, n):
    """gray: 8 n block rows, each of them `row`"""
    return gray_image(np.tile(row, (8 * n, 1)), len(row))


def periods_past(threshold, period_bytes, unit=1):
    """the least multiple of `unit` periods whose bytes pass SLACK x threshold"""
    n = -(-int(threshold * SLACK) // period_bytes)
    return -(-n // unit) * unit


# ---- tilers: (the bytes in front, the period, how many, how many bytes the last repetition lacks, the bytes behind) --------

class Tiled:
    """a byte string given as head + period * n (without the last `cut` bytes) + tail"""

    def __init__(self, head, period, n, cut=0, tail=b""):
        self.head, self.period, self.n, self.cut, self.tail = bytes(head), bytes(period), int(n), int(cut), bytes(tail)

    def __len__(self):
        return len(self.head) + len(self.period) * self.n - self.cut + len(self.tail)

    def body_len(self):
        return len(self.period) * self.n - self.cut

    def bytes(self):
        """the whole string on the host (small n only)"""
        body = self.period * self.n
        return self.head + body[:len(body) - self.cut] + self.tail


def restart_unit(one: bytes) -> bytes:
    """U of the restart form from libjpeg's file (or segment) of ONE pattern: its segment + FF D7"""
    return one + b"\xff\xd7"


def tile_restart_segment(one_segment, n):
    return Tiled(b"", restart_unit(one_segment), n, cut=2)


def tile_norestart_segment(one_segment, n):
    return Tiled(b"", one_segment, n)


def tile_file(one_file, n, image_size, restart=True):
    """libjpeg's whole file of n periods from its file of one: the same markers but for the frame's size, the tiled
    segment, EOI"""
    f = parse_rst(one_file)
    assert f["tail"] == b"\xff\xd9"
    head = resize_head(f["head"], image_size)
    seg = tile_restart_segment(f["segment"], n) if restart else tile_norestart_segment(f["segment"], n)
    return Tiled(head, seg.period, n, seg.cut, b"\xff\xd9")


def resize_head(head: bytes, image_size):
    """the markers up to the SOS header with the frame header's height and width replaced"""
    pos = 2
    head = bytearray(head)
    while True:
        assert head[pos] == 0xFF
        code, n = head[pos + 1], struct.unpack_from(">H", head, pos + 2)[0]
        if code in (0xC0, 0xC1, 0xC2):
            struct.pack_into(">HH", head, pos + 5, image_size[1], image_size[0])
            return bytes(head)
        assert code != 0xDA, "no frame header"
        pos += 2 + n


# ---- scaled counts and the tables libjpeg makes of them --------------------------------------------------------------------

def gray_interval_symbols(blocks, ri):
    """[[(is_ac, symbol, bits, nbits)] per interval] of a gray scan over `blocks` in scan order; ri 0: one interval"""
    out, prev = [], 0
    for b, blk in enumerate(blocks):
        if b == 0 or (ri and b % ri == 0):
            out.append([])
            prev = 0
        out[-1] += block_symbols(blk, prev)
        prev = int(blk[0])
    return out


def counts_of(intervals):
    h = np.zeros((2, 257), np.int64)
    for syms in intervals:
        for is_ac, sym, _bits, _nb in syms:
            h[is_ac, sym] += 1
    return h


def scaled_tables(counts, n):
    """libjpeg's optimal (DC, AC) tables for n periods of these per-period counts"""
    return libjpeg_optimal(counts[0][:256] * n), libjpeg_optimal(counts[1][:256] * n)


def code_intervals(intervals, dc, ac):
    """the unstuffed bytes of each interval, padded with ones"""
    dcc, acc = derive(dc), derive(ac)
    raws = []
    for syms in intervals:
        out, v, held = bytearray(), 0, 0                  # (whole bytes leave v as they fill: a long interval stays cheap)
        for is_ac, sym, bits, nb in syms:
            code, size = (acc if is_ac else dcc)[sym]
            v = (v << (size + nb)) | (code << nb) | bits
            held += size + nb
            if held >= 64:
                keep = held % 8
                out += (v >> keep).to_bytes((held - keep) // 8, "big")
                v &= (1 << keep) - 1
                held = keep
        pad = -held % 8
        v = (v << pad) | ((1 << pad) - 1)
        raws.append(bytes(out) + v.to_bytes((held + pad) // 8, "big"))
    return raws


def optimized_restart(pattern, n):
    """-> (counts (2, 257) of ONE pattern, (dc, ac) tables of n patterns, the tiled segment)"""
    intervals = gray_interval_symbols(pattern, RI)
    counts = counts_of(intervals)
    dc, ac = scaled_tables(counts, n)
    one = compose_segment(code_intervals(intervals, dc, ac))
    return counts, (dc, ac), tile_restart_segment(one, n)


def optimized_norestart(row, n):
    """the same for the no-restart form: the period is 8 rows"""
    intervals = gray_interval_symbols(np.tile(row, (8, 1)), 0)
    counts = counts_of(intervals)
    dc, ac = scaled_tables(counts, n)
    (raw,) = code_intervals(intervals, dc, ac)
    assert sum(_interval_bits(intervals[0], dc, ac)) % 8 == 0            # 8 equal rows: no padding inside the tiling
    return counts, (dc, ac), tile_norestart_segment(stuff(raw), n)


def _interval_bits(syms, dc, ac):
    dcc, acc = derive(dc), derive(ac)
    return [(acc if is_ac else dcc)[sym][1] + nb for is_ac, sym, _bits, nb in syms]


def dht(cls, index, table) -> bytes:
    bits, vals = table
    n = sum(bits[1:17])
    payload = bytes([(cls << 4) | index]) + bytes(int(b) for b in bits[1:17]) + bytes(int(v) for v in vals[:n])
    return b"\xff\xc4" + struct.pack(">H", len(payload) + 2) + payload


# ---- progressive files of the restart form, scan by scan ---------------------------------------------------------------------

DC_AC_SCRIPT = [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0)]
# a short scan behind a long one: with the AC scan 1..62 past 2^31 bytes the last SOS lies past 2^31 bytes of the file
DC_AC_AC_SCRIPT = [((0,), 0, 0, 0, 0), ((0,), 1, 62, 0, 0), ((0,), 63, 63, 0, 0)]
WB_OFFSET = 4096                   # block columns of that case: 25 M blocks of 85 bytes in the long scan


def progressive_tiled(pattern, n, head: bytes, script, ri):
    """the progressive file of n patterns (gray; restart interval ri with the pattern a whole number of 8 intervals, or
    ri = 0 with a pattern that codes to whole bytes in every scan and leaves no state behind: see
    refine_norestart_pattern) under `script`, refinement scans included -> [Tiled per scan]: scan k's Tiled carries in `head` everything in front of its
    entropy-coded bytes (for scan 0 the file's head, `head`, too) and the last one EOI as its tail.  Each scan has its own
    optimal table, made of n times the counts of one pattern; a DC refinement scan has none."""
    im = gray_image(pattern, len(pattern))
    out = []
    for k, scan in enumerate(script):
        _comps, ss, se, ah, al = scan
        intervals = scan_symbols_refine(im, scan, ri) if ah else scan_symbols_prog(im, scan, ri)
        assert (len(intervals) * ri == len(pattern) and len(intervals) % 8 == 0) if ri else len(intervals) == 1
        hist = np.zeros(256, np.int64)
        for syms in intervals:
            for _is_ac, sym, _b, _nb, _c in syms:
                if sym is not None:
                    hist[sym] += 1
        front = bytearray(head if k == 0 else b"")
        codes = None
        if ss or not ah:
            table = libjpeg_optimal(hist * n)
            codes = derive(table)
            front += dht(1 if ss else 0, 0, table)
        if k == 0 and ri:
            front += b"\xff\xdd\x00\x04" + struct.pack(">H", ri)
        front += b"\xff\xda" + struct.pack(">HB", 8, 1) + bytes([1, 0, ss, se, (ah << 4) | al])
        unit = bytearray()
        for i, syms in enumerate(intervals):
            v, nbt = 0, 0
            for _is_ac, sym, bits, nb, _c in syms:
                code, size = codes[sym] if sym is not None else (0, 0)
                v = (v << (size + nb)) | (code << nb) | bits
                nbt += size + nb
            pad = -nbt % 8
            assert ri or pad == 0, "without restarts the pattern must code to whole bytes in every scan"
            v = (v << pad) | ((1 << pad) - 1)
            unit += stuff(v.to_bytes((nbt + pad) // 8, "big")) + (bytes([0xFF, 0xD0 + (i & 7)]) if ri else b"")
        out.append(Tiled(front, unit, n, cut=2 if ri else 0, tail=b"\xff\xd9" if k == len(script) - 1 else b""))
    return out


def progressive_restart(pattern, n, head: bytes):
    """DC scan, then AC 1..63, restart interval RI"""
    return progressive_tiled(pattern, n, head, DC_AC_SCRIPT, RI)


# ---- the refinement coder's running weight (csrc/qs_kernels_encode_prog.inc: qr_wsum, qr_wscan, qr_next) ----------------------
# With GRAY_REFINE (DC; AC 1..63 at Al = 1; its last bit) a coefficient of +-2 or +-3 leaves one correction bit in the
# refinement scan and writes no symbol.  A block of such values ends its band with correction bits buffered (its tail), and
# with restart interval 1 every block starts an interval, so every block but the last weighs its tail + QR_CORR_MAX + 1.

REFINE_TAILS = (63, 40, 55, 63, 47, 63, 60, 52)         # correction bits the 8 blocks of the pattern leave
REFINE_WB = 2048                                         # block columns of the GPU module's image (a multiple of 8)
CORR_CUT = CORR_MAX + 1                                  # QR_CORR_MAX + 1: what a block in front of a head adds


def refine_pattern(seed=SEED):
    rng = np.random.default_rng(seed)
    out = np.zeros((len(REFINE_TAILS), 64), np.int16)
    for b, tail in enumerate(REFINE_TAILS):
        out[b, 0] = rng.integers(-100, 101)
        out[b, [ZIGZAG[z] for z in range(1, tail + 1)]] = rng.choice(np.array([-3, -2, 2, 3]), tail)
    return out


def refine_weight(pattern, n):
    """the sum qr_wscan carries to the end of n patterns under GRAY_REFINE's refinement scan with restart interval 1, from
    the pattern's own run pieces (the restatement's: one piece of one block and its buffered bits per interval)"""
    pieces = run_pieces(gray_image(pattern, len(pattern)), GRAY_REFINE[2], 1)
    assert [length for length, _bits in pieces] == [1] * len(pattern)
    return n * (sum(bits for _length, bits in pieces) + CORR_CUT * len(pattern)) - CORR_CUT


def refine_periods(pattern, weight=None):
    """the least multiple of REFINE_WB / len(pattern) patterns whose weight passes SLACK x 2^32"""
    unit = REFINE_WB // len(pattern)
    per = (weight or refine_weight)(pattern, 1) + CORR_CUT
    n = -(-int((1 << 32) * SLACK) // per)
    return -(-n // unit) * unit


def refine_block_weights(ri):
    """what qr_wsum gives each block of one pattern (every block has a next one): restart interval 1, or the mirror"""
    if ri:
        return [t + CORR_CUT for t in REFINE_TAILS]
    return ([0] + [63] * (GROUP_TAILS - 1) + [63 + CORR_CUT]) * 8


def wrap_block(weights, n):
    """the first block of n patterns whose exclusive running weight -- what qr_next reads for it -- is at least 2^32"""
    per = sum(weights)
    full = (1 << 32) // per
    rest, b, acc = (1 << 32) - full * per, full * len(weights), 0
    for w in weights:
        if acc >= rest:
            break
        acc += w
        b += 1
    assert b < n * len(weights), "the sum does not wrap inside the scan"
    return b


# The mirror without restarts: 8 groups of a block that writes -- its last band coefficient is newly non-zero, so it leaves
# no tail and the run behind it starts afresh -- and GROUP_TAILS blocks of 63 correction bits each.  The writing blocks are
# the only heads: every run piece spans the GROUP_TAILS blocks between two of them, the last of which weighs 63 +
# QR_CORR_MAX + 1.  Tiling: no scan carries state from one group to the next (the DC of a group's last block is 0, a
# writing block flushes the EOB run in front of it), and 8 equal groups code to whole bytes in every scan.

GROUP_TAILS = 3


def refine_norestart_pattern(seed=SEED):
    rng = np.random.default_rng(seed + 1)
    group = np.zeros((1 + GROUP_TAILS, 64), np.int16)
    group[0, 0] = rng.integers(-100, 101)
    group[0, [ZIGZAG[z] for z in range(1, 10)]] = rng.choice(np.array([-3, -2, 2, 3]), 9)
    group[0, ZIGZAG[63]] = 1
    for b in range(1, 1 + GROUP_TAILS):
        group[b, 0] = rng.integers(-100, 101) if b < GROUP_TAILS else 0
        group[b, [ZIGZAG[z] for z in range(1, 64)]] = rng.choice(np.array([-3, -2, 2, 3]), 63)
    return np.tile(group, (8, 1))


def refine_weight_norestart(pattern, n):
    """the sum qr_wscan carries to the end of n such patterns without restarts, from the pattern's own run pieces"""
    pieces = run_pieces(gray_image(pattern, len(pattern)), GRAY_REFINE[2], 0)
    assert pieces == [(GROUP_TAILS, 63 * GROUP_TAILS)] * 8
    return n * (sum(bits for _length, bits in pieces) + CORR_CUT * len(pieces)) - CORR_CUT


def tiled_concat(parts) -> bytes:
    """the file of several Tiled parts on the host (small n only)"""
    return b"".join(p.bytes() for p in parts)
