"""What the tests of the scan reader's progressive route share (tests/test_read_prog_host.py, tests/test_gpu_read_prog.py):
the host build of csrc/qs_read_prog.h (tests/read_prog_host.cpp, compiled on demand, optionally with
-fsanitize=address,undefined), libjpeg 9 at both ends of the oracle -- files written by tests/libjpeg9_encode.c,
expected arrays read by tests/libjpeg9_decode.c -- the grid of valid cases and the seeded corrupt corpus."""
import os
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import jpegqs_pkg
from encode_oracle import LAYOUTS, synth_scan_image
from encode_prog_oracle import PROG_SIZES
from encode_refine_oracle import GRAY_REFINE, big_crafted_images, crafted_images, refine_scripts
from encode_rst_oracle import RST_LAYOUTS, dc_range_images, mcu_geometry
from host_tools import HERE, build, run
from read_oracle import CORPUS_SEED, CaseHost, LibjpegReader, padded_shapes
from wire import frame_words, pack_tables, pad4

pkg = jpegqs_pkg.load()
from jpeg_quantsmooth_amd import jpeg_file  # noqa: E402

GOLDEN_PROG = HERE / "golden" / "cli" / "rgb120x88_prog.jpg"


def pack_case(c) -> bytes:
    p = c["header"]
    out = [struct.pack("<20i", *frame_words(p, c["shapes"]), len(p["scans"]))]
    for s in p["scans"]:
        out.append(struct.pack("<18iQ", len(s["comps"]), *pad4(s["comps"]), s["ss"], s["se"], s["ah"], s["al"],
                               *pad4(s["dc_tbl"]), *pad4(s["ac_tbl"]), s["restart_interval"], s["offset"]))
        out.append(pack_tables(s))
    out.append(struct.pack("<Q", len(c["data"])) + bytes(c["data"]))
    return b"".join(out)


class ReadProgHost(CaseHost):
    """tests/read_prog_host.cpp: qs_read_prog.h on the host.  run(cases): [dict(header: jpeg_file.parse_progressive's
    dict, data: the file, shapes: [(rows, stride)] per component)] -> [(status, levels, [int16 arrays (rows, stride, 64)]
    or None)]"""
    PACK, WORDS = staticmethod(pack_case), 2

    def __init__(self, workdir, sanitize=False):
        super().__init__(build("read_prog_host.cpp", flags=["-Wno-unknown-pragmas"], sanitize=sanitize), workdir)


def expected_arrays(ref, shapes, script):
    """libjpeg's arrays (ref: LibJpeg9.read's dict) in arrays of `shapes`: 0 in every block no scan codes and -- frames of
    several components -- the dummy blocks of edge MCUs where the array has room for them: all AC 0, and the DC the
    INTERLEAVED DC scans of the script carry for them.  With D the final DC of the real block before it in the MCU
    (jctrans.c compress_output repeats it), a first scan contributes (D >> Al) << Al (the coded difference is 0) and a
    refinement ORs ((D >> Al) & 1) << Al; one-component scans skip dummy blocks"""
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
            dc_scans = [(ah, al) for comps, ss, _se, ah, al in script if ss == 0 and len(comps) > 1 and ci in comps]
            for m_y in range(my):
                for m_x in range(mx):
                    last = 0
                    for y in range(vs[ci]):
                        for x in range(hs[ci]):
                            bx, by = m_x * hs[ci] + x, m_y * vs[ci] + y
                            if bx < wb and by < hb:
                                last = int(a[by, bx, 0])
                            elif bx < a.shape[1] and by < a.shape[0]:
                                v = 0
                                for ah, al in dc_scans:
                                    v = (v | (((last >> al) & 1) << al)) if ah else ((last >> al) << al)
                                a[by, bx, 0] = np.int16(v)
    return out


def make_case(enc, lj, name, im, script, ri, rows, k):
    """one valid case: the file libjpeg writes, its parsed markers, libjpeg's read of it in arrays of padded_shapes"""
    data = enc.write(im, script, ri, rows)
    return case_of_file(lj, name, data, k, script=script, image=im)


def case_of_file(lj, name, data, k, script=None, image=None):
    p = jpeg_file.parse_progressive(data)
    ref, clean = lj.read_bytes(data)
    assert clean, name
    shapes = padded_shapes(p, k)
    return dict(name=name, data=data, header=p, shapes=shapes, image=image, script=script or p["script"],
                want=expected_arrays(ref, shapes, p["script"]))


def grid_specs():
    """[(name, image, script, restart_interval, restart_in_rows)]"""
    out = []
    for li in RST_LAYOUTS:
        hs, vs, cs = LAYOUTS[li]
        n = len(hs)
        for size in PROG_SIZES:
            im = synth_scan_image(np.random.default_rng(li * 977 + size[0] * 31 + size[1]), size, hs, vs, cs)
            for ri, rows in ((0, 0), (1, 0), (7, 0), (0, 1)):
                out.append((f"layout {li} at {size} simple Ri {ri} rows {rows}", im, jpeg_file.simple_progression(n, cs), ri, rows))
            if size not in ((33, 18), (141, 93)):
                continue
            scripts = dict(refine_scripts(n, cs, jpeg_file.simple_progression))
            del scripts["simple"]
            scripts["spectral"] = jpeg_file.spectral_script(n)
            if n == 1:
                scripts["gray refine"] = GRAY_REFINE
            mx, m, _bpm = mcu_geometry(im)
            for sname, script in scripts.items():
                for ri in sorted({0, 1, 2, mx, max(m - 1, 0), m, m + 1}):
                    out.append((f"layout {li} at {size} {sname} Ri {ri}", im, script, ri, 0))
    for name, im in crafted_images().items():
        out.append((f"crafted {name}", im, GRAY_REFINE, 0, 0))
    out.append(("crafted all zero (32 768 blocks, one lane)", big_crafted_images()["all zero"], GRAY_REFINE, 0, 0))
    dc_script = [((0,), 0, 0, 0, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 0, 0)]
    for i, im in enumerate(dc_range_images()):
        out.append((f"DC range {'ab'[i]}, Al 1 then refined", im, dc_script, i, 0))
    return out


def build_grid(enc, lj):
    grid = [make_case(enc, lj, name, im, script, ri, rows, k) for k, (name, im, script, ri, rows) in enumerate(grid_specs())]
    grid.append(case_of_file(lj, "golden rgb120x88_prog.jpg", GOLDEN_PROG.read_bytes(), len(grid)))
    return grid


# ---- the corrupt corpus --------------------------------------------------------------------------------------------------

def corpus_sources(enc, lj):
    """three small valid files, Ri = 1, libjpeg's simple progression: gray, 4:2:0 with edge MCUs, 4:4:4"""
    rng = np.random.default_rng(CORPUS_SEED)
    specs = [synth_scan_image(rng, (24, 16), [1], [1], 1, amp=20, density=0.2),
             synth_scan_image(rng, (33, 17), [2, 1, 1], [2, 1, 1], 3, amp=20, density=0.15),
             synth_scan_image(rng, (17, 9), [1, 1, 1], [1, 1, 1], 3, amp=20, density=0.2)]
    return [make_case(enc, lj, f"corpus source {i}", im, jpeg_file.simple_progression(len(im["hsamp"]), im["colorspace"]),
                      1, 0, 0) for i, im in enumerate(specs)]


def corrupt_corpus(sources):
    """[dict(name, data: the whole corrupt file, header, shapes)]: truncation at every byte behind the first SOS, each of
    the first 64 bytes of every scan replaced by 00 / FF / D0, two RSTn of one scan swapped, one RSTn deleted, an AC DHT
    with a missing symbol.  The header is the source's (what a prepare on the intact file holds) except where the
    markers move (the deleted RSTn, the shorter DHT): there the damaged file is parsed again.  Deterministic."""
    out = []
    for si, src in enumerate(sources):
        data, p = src["data"], src["header"]

        def add(name, d, header=p):
            out.append(dict(name=f"source {si}: {name}", data=d, header=header, shapes=src["shapes"]))
        first = p["scans"][0]["offset"]
        for k in range(first, len(data)):
            add(f"truncated at {k}", data[:k])
        for i, s in enumerate(p["scans"]):
            for k in range(s["offset"], s["offset"] + min(64, s["length"])):
                for v in (0x00, 0xFF, 0xD0):
                    if data[k] != v:
                        add(f"scan {i} byte {k - s['offset']} = {v:02X}", data[:k] + bytes([v]) + data[k + 1:])
        s = next(s for s in p["scans"] if s["length"] > 8 and
                 sum(1 for j in range(s["offset"], s["offset"] + s["length"] - 1)
                     if data[j] == 0xFF and 0xD0 <= data[j + 1] <= 0xD7) >= 3)
        marks = [j for j in range(s["offset"], s["offset"] + s["length"] - 1) if data[j] == 0xFF and 0xD0 <= data[j + 1] <= 0xD7]
        a, b = marks[0], marks[1]
        sw = bytearray(data)
        sw[a + 1], sw[b + 1] = data[b + 1], data[a + 1]
        add("markers 1 and 2 swapped", bytes(sw))
        d = data[:b] + data[b + 2:]
        add("marker 2 deleted", d, jpeg_file.parse_progressive(d))
        # the first AC DHT without its second symbol: one code of that length less
        pos = 0
        while True:
            pos = data.index(b"\xff\xc4", pos)
            if data[pos + 4] & 0x10 and sum(data[pos + 5:pos + 21]) >= 2:
                break
            pos += 4
        n = struct.unpack_from(">H", data, pos + 2)[0]
        bits = list(data[pos + 5:pos + 21])
        vals = data[pos + 21:pos + 2 + n]
        l = next(i for i, c in enumerate(bits) if c > 0 and sum(bits[:i + 1]) >= 2)
        drop = sum(bits[:l + 1]) - 1
        bits[l] -= 1
        seg = bytes([data[pos + 4]]) + bytes(bits) + vals[:drop] + vals[drop + 1:]
        d = data[:pos] + b"\xff\xc4" + struct.pack(">H", len(seg) + 2) + seg + data[pos + 2 + n:]
        add("DHT with a missing symbol", d, jpeg_file.parse_progressive(d))
    return out


def libjpeg_reads(lj: LibjpegReader, corpus, threads=8):
    """[(image dict or None, clean)] of LibjpegReader.read_bytes for every file of the corpus, several at a time (the
    arrays are read only where libjpeg is clean: nothing else is compared)"""
    def one(job):
        i, data = job
        src, out = lj.dir / f"lr{os.getpid()}_{i}.jpg", lj.dir / f"lr{os.getpid()}_{i}.bin"
        src.write_bytes(data)
        try:
            r = run(lj.exe, "read", src, out, ok=None)
            if r.returncode or r.stderr.strip():
                return None, False
            return src, True
        finally:
            if out.exists():
                out.unlink()
    with ThreadPoolExecutor(threads) as ex:
        first = list(ex.map(one, enumerate(c["data"] for c in corpus)))
    res = []
    for (src, clean), c in zip(first, corpus):
        if clean:
            src.write_bytes(c["data"])
            res.append((lj.read(src), True))
        else:
            res.append((None, False))
    for i in range(len(corpus)):
        f = lj.dir / f"lr{os.getpid()}_{i}.jpg"
        if f.exists():
            f.unlink()
    return res
