"""What the tests of the device scan reader share (tests/test_read_host.py, tests/test_gpu_read.py): the host build of
csrc/qs_read.h (tests/read_host.cpp, compiled on demand, optionally with -fsanitize=address,undefined), libjpeg 9 at
both ends of the oracle -- files written by tests/libjpeg9_encode.c, expected arrays read by tests/libjpeg9_decode.c
-- the grid of valid cases and the seeded corrupt corpus."""
import struct

import numpy as np

import jpegqs_pkg
from decode_oracle import LibJpeg9, blocks_needed
from encode_oracle import LAYOUTS, SIZES, synth_scan_image
from encode_rst_oracle import RST_LAYOUTS, dc_range_images, mcu_geometry, optimize_cases, padding_case
from host_tools import CSRC, HERE, Tool, build  # noqa: F401
from wire import frame_words, pack_tables, pad4, parse_image, parse_results

pkg = jpegqs_pkg.load()
from jpeg_quantsmooth_amd import jpeg_file  # noqa: E402

CORPUS_SEED = 1           # the three valid files of the corrupt corpus (corpus_sources); 3.2 % of it decodes clean


class CaseHost(Tool):
    """a host build of a scan reader that takes `run in.bin out.bin`: int32 ncases and the cases of PACK in, per case
    WORDS int32 (the status first) and the arrays out.  A run fails on a non-zero exit or anything on stderr (a sanitizer
    report)."""
    SILENT = True
    WORDS = 1

    def run(self, cases, *args):
        src, dst = self.tmp(".bin"), self.tmp(".out")
        with open(src, "wb") as f:
            f.write(struct.pack("<i", len(cases)))
            for c in cases:
                f.write(self.PACK(c))
        self._run("run", src, dst, *args)
        b = dst.read_bytes()
        src.unlink()
        dst.unlink()
        return parse_results(b, cases, self.WORDS)


def pack_case(c) -> bytes:
    p = c["header"]
    return struct.pack("<28i", *frame_words(p, c["shapes"]), *pad4(p["dc_tbl"]), *pad4(p["ac_tbl"]), p["restart_interval"]) \
        + pack_tables(p) + struct.pack("<Q", len(c["scan"])) + bytes(c["scan"])


class ReadHost(CaseHost):
    """tests/read_host.cpp: qs_read.h on the host.  run(cases): [dict(header: jpeg_file.parse's dict, scan: bytes,
    shapes: [(rows, stride)] per component)] -> [(status, [int16 arrays (rows, stride, 64)] or None)]"""
    PACK = staticmethod(pack_case)

    def __init__(self, workdir, sanitize=False):
        super().__init__(build("read_host.cpp", sanitize=sanitize), workdir)


def true_shapes(p):
    """[(height_in_blocks, width_in_blocks)] of libjpeg's geometry"""
    return [blocks_needed(p["image_size"], p["hsamp"], p["vsamp"], ci) for ci in range(len(p["hsamp"]))]


class LibjpegReader(LibJpeg9):
    """LibJpeg9.read on bytes, and whether libjpeg read them without a warning or an error"""

    def read_bytes(self, data):
        """-> (image dict or None when libjpeg stopped with an error, clean: no warning and no error).  libjpeg's
        default error manager prints the first warning of a file to stderr and counts the rest in num_warnings."""
        src, out = self.tmp(".jpg"), self.tmp(".bin")
        src.write_bytes(data)
        try:
            r = self._run("read", src, out, ok=None)
            return (parse_image(out.read_bytes()), not r.stderr.strip()) if r.returncode == 0 else (None, False)
        finally:
            src.unlink()
            out.unlink(missing_ok=True)


def expected_arrays(ref, shapes):
    """libjpeg's arrays (ref: LibJpeg9.read's dict) in arrays of `shapes`: 0 outside, and -- interleaved scans -- the
    dummy blocks of edge MCUs where the array has room for them: all AC 0, the DC of the block before them in the MCU
    (jdhuff.c decodes the DC difference 0 the encoder wrote for them, jctrans.c compress_output)"""
    hs, vs, n = ref["hsamp"], ref["vsamp"], len(ref["coefs"])
    out = []
    for ci, (rows, stride) in enumerate(shapes):
        a = np.zeros((rows, stride, 64), np.int16)
        hb, wb = ref["coefs"][ci].shape[:2]
        a[:hb, :wb] = ref["coefs"][ci]
        out.append(a)
    if n > 1:
        w, h = ref["image_size"]
        mx, my = -(-w // (8 * max(hs))), -(-h // (8 * max(vs)))
        for ci, a in enumerate(out):
            hb, wb = ref["coefs"][ci].shape[:2]
            for m_y in range(my):
                for m_x in range(mx):
                    last = 0
                    for y in range(vs[ci]):
                        for x in range(hs[ci]):
                            bx, by = m_x * hs[ci] + x, m_y * vs[ci] + y
                            if bx < wb and by < hb:
                                last = a[by, bx, 0]
                            elif bx < a.shape[1] and by < a.shape[0]:
                                a[by, bx, 0] = last
    return out


def padded_shapes(p, k):
    """the arrays of case k: libjpeg's own geometry, or (every third case) wider and taller than needed -- room for the
    dummy blocks of edge MCUs and beyond"""
    t = true_shapes(p)
    if k % 3 != 1:
        return t
    return [(hb + 1 + k % 3, wb + 2 + ci) for ci, (hb, wb) in enumerate(t)]


def make_case(enc, lj, name, im, ri, rows, k, optimize=False):
    """one valid case: the file libjpeg writes, its parsed header, libjpeg's read of it in arrays of padded_shapes"""
    data = enc.write(im, ri, rows, optimize)
    p = jpeg_file.parse(data)
    ref, clean = lj.read_bytes(data)
    assert clean, name
    shapes = padded_shapes(p, k)
    return dict(name=name, data=data, header=p, scan=data[p["scan_offset"]:], shapes=shapes, image=im,
                want=expected_arrays(ref, shapes))


def grid_specs():
    """[(name, image, restart_interval, restart_in_rows, optimize)]: every layout x every size (edge MCUs with dummy
    blocks) x Ri in {1, 2, 7, MCUs per row, M - 1, M, M + 1, 0} and restart_in_rows in {1, 2}; the DC extremes, the
    stuffed FF 00 in front of a marker, optimized tables (codes of up to 16 bits)"""
    out = []
    for li in RST_LAYOUTS:
        hs, vs, cs = LAYOUTS[li]
        for size in SIZES:
            im = synth_scan_image(np.random.default_rng(li * 1000 + size[0]), size, hs, vs, cs)
            mx, m, _bpm = mcu_geometry(im)
            for ri in sorted({1, 2, 7, mx, max(m - 1, 0), m, m + 1, 0}):
                out.append((f"layout {li} at {size} Ri {ri}", im, ri, 0, False))
            for rows in (1, 2):
                out.append((f"layout {li} at {size} rows {rows}", im, 0, rows, False))
    a, b = dc_range_images()
    out.append(("DC range a, one interval", a, 0, 0, False))
    out.append(("DC range b, Ri 1", b, 1, 0, False))
    pim, pri = padding_case()
    out.append(("stuffed FF 00 in front of a marker", pim, pri, 0, False))
    for i, (im, ri, rows) in enumerate(optimize_cases()):
        out.append((f"optimized tables {i}", im, ri, rows, True))
    out.append(("a table with 16-bit codes", long_code_image(), 3, 0, True))
    return out


def long_code_image():
    """gray, with AC symbol counts that fall off geometrically: the optimal table reaches 16-bit codes"""
    blocks = np.zeros((64, 64), np.int16)
    n = 0
    for s in range(1, 11):                                            # symbol (run 0, size s), 2^(11 - s) times
        for _ in range(1 << (11 - s)):
            blocks[n % 64, 1 + (n // 64) % 63] = (1 << (s - 1))
            n += 1
    rng = np.random.default_rng(3)
    for run in range(1, 15):                                          # a tail of rare symbols
        b = rng.integers(0, 64)
        blocks[b] = 0
        blocks[b, 1 + run] = 3
    return dict(coefs=[blocks.reshape(8, 8, 64)], quants=[np.ones(64, np.uint16)], hsamp=[1], vsamp=[1], colorspace=1,
                image_size=(64, 64))


def build_grid(enc, lj):
    return [make_case(enc, lj, name, im, ri, rows, k, opt) for k, (name, im, ri, rows, opt) in enumerate(grid_specs())]


# ---- the corrupt corpus --------------------------------------------------------------------------------------------------

def corpus_sources(enc, lj):
    """three small valid files with restart markers: gray, 4:2:0 with edge MCUs, 4:4:4 with optimized tables"""
    rng = np.random.default_rng(CORPUS_SEED)
    specs = [(synth_scan_image(rng, (24, 16), [1], [1], 1, amp=20, density=0.2), 1, False),
             (synth_scan_image(rng, (33, 17), [2, 1, 1], [2, 1, 1], 3, amp=20, density=0.15), 1, False),
             (synth_scan_image(rng, (17, 9), [1, 1, 1], [1, 1, 1], 3, amp=20, density=0.2), 1, True)]
    return [make_case(enc, lj, f"corpus source {i}", im, ri, 0, 0, opt) for i, (im, ri, opt) in enumerate(specs)]


def _marker_positions(scan):
    return [i for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]


def corrupt_corpus(sources):
    """[dict(name, data: the whole corrupt file, header, scan, shapes)]: truncation at every byte of the scan, each of
    the first 64 scan bytes replaced by 00 / FF / D0, two markers swapped, one marker deleted, a DHT with a missing
    symbol.  Deterministic: the sources are seeded, nothing else is random."""
    out = []
    for si, src in enumerate(sources):
        data, p = src["data"], src["header"]
        off = p["scan_offset"]
        end = data.rindex(b"\xff\xd9")
        head, scan, tail = data[:off], data[off:end], data[end:]

        def add(name, new_scan=None, new_head=None, new_tail=tail, header=p):
            d = (head if new_head is None else new_head) + (scan if new_scan is None else new_scan) + new_tail
            h = jpeg_file.parse(d, header_only=True) if new_head is not None else header
            out.append(dict(name=f"source {si}: {name}", data=d, header=h, scan=d[h["scan_offset"]:],
                            shapes=src["shapes"]))
        for k in range(len(scan)):
            add(f"truncated at {k}", scan[:k], new_tail=b"")
        for k in range(min(64, len(scan))):
            for v in (0x00, 0xFF, 0xD0):
                if scan[k] != v:
                    add(f"byte {k} = {v:02X}", scan[:k] + bytes([v]) + scan[k + 1:])
        marks = _marker_positions(scan)
        assert len(marks) >= 3
        a, b = marks[0], marks[1]
        sw = bytearray(scan)
        sw[a + 1], sw[b + 1] = scan[b + 1], scan[a + 1]
        add("markers 1 and 2 swapped", bytes(sw))
        add("marker 2 deleted", scan[:b] + scan[b + 2:])
        # the DHT of the first AC table without its second symbol: one code of that length less
        pos = 0
        while True:                                                    # the DHT segment that holds an AC table
            pos = head.index(b"\xff\xc4", pos)
            if head[pos + 4] & 0x10:
                break
            pos += 4
        n = struct.unpack_from(">H", head, pos + 2)[0]
        bits = list(head[pos + 5:pos + 21])
        vals = head[pos + 21:pos + 2 + n]
        l = next(i for i, c in enumerate(bits) if c > 0 and sum(bits[:i + 1]) >= 2)
        drop = sum(bits[:l + 1]) - 1                                   # the last symbol of the first length with two codes in all
        bits[l] -= 1
        seg = bytes([head[pos + 4]]) + bytes(bits) + vals[:drop] + vals[drop + 1:]
        new_head = head[:pos] + b"\xff\xc4" + struct.pack(">H", len(seg) + 2) + seg + head[pos + 2 + n:]
        add("DHT with a missing symbol", new_head=new_head)
    return out
