"""Progressive files (spectral selection) of the device entropy coder: libjpeg 9 as the oracle
(tests/libjpeg9_encode.c, compiled on demand), a plain Python restatement of jchuff.c's encode_mcu_DC_first /
encode_mcu_AC_first / emit_eobrun, jcmaster.c's per_scan_setup and jcmarker.c's write_scan_header on top of
tests/encode_oracle.py and tests/huff_oracle.py (test only: it pins the rules of DESIGN.md section 17 against libjpeg
before any GPU is involved), the host build of csrc/qs_encode_prog.h (tests/encode_prog_host.cpp), and the builders of the
cases the test modules share."""
import struct

import numpy as np

from decode_oracle import blocks_needed
from encode_oracle import LAYOUTS, ZIGZAG, BadCoef, LibJpeg9Enc, derive, nbits, synth_scan_image
from encode_rst_oracle import RST_LAYOUTS, stuff
from host_tools import Tool, build
from huff_oracle import libjpeg_optimal
from wire import pack_image

PROG_SIZES = [(1, 1), (7, 9), (8, 8), (16, 17), (33, 18), (65, 66), (141, 93)]
EOB_MAX = 0x7FFF


def script_text(script) -> str:
    return "".join("%d %d %d %d %d %d %d %d %d\n" % ((len(c),) + tuple((list(c) + [0, 0, 0, 0])[:4]) + (ss, se, ah, al))
                   for c, ss, se, ah, al in script)


class LibJpeg9EncProg(LibJpeg9Enc):
    """LibJpeg9Enc with cinfo.scan_info set"""

    def write(self, im, script, ri=0, rows=0) -> bytes:
        """the file libjpeg makes of the image dict with the script; LibjpegError when libjpeg refuses"""
        src = self.stage(im)
        txt = src.with_suffix(".txt")
        txt.write_text(script_text(script))
        try:
            return self._write(src, int(ri), int(rows), txt)
        finally:
            src.unlink()
            txt.unlink()


class ProgHost(Tool):
    """tests/encode_prog_host.cpp: csrc/qs_encode_prog.h in its host form, as a process"""
    SOURCE = "encode_prog_host.cpp"

    def __init__(self, workdir, sanitize=False):
        super().__init__(build(self.SOURCE, flags=["-Wno-unknown-pragmas"], sanitize=sanitize), workdir)

    def bounds(self) -> str:
        return self._run("bounds").stdout

    def validate(self, script, ncomp):
        """-> (QP_SCRIPT_* code, scan)"""
        txt = self.tmp(".txt")
        txt.write_text(script_text(script))
        r = self._run("validate", ncomp, txt)
        txt.unlink()
        code, scan = r.stdout.split()[:2]
        return int(code), int(scan)

    def write(self, im, script, head: bytes, ri=0, rows=0):
        """-> the file, or the status (1 / 5) the header's coders end with"""
        src = self.tmp(".bin")
        out, txt, hd = src.with_suffix(".jpg"), src.with_suffix(".txt"), src.with_suffix(".head")
        src.write_bytes(pack_image(im))
        txt.write_text(script_text(script))
        hd.write_bytes(head)
        try:
            r = self._run("write", src, txt, hd, out, int(ri), int(rows), ok=(0, 4, 5))
            if r.returncode == 4:
                return int(r.stdout.split()[1])
            if r.returncode == 5:
                return "mcu"
            return out.read_bytes()
        finally:
            for p in (src, out, txt, hd):
                p.unlink(missing_ok=True)


# ---- the restatement ---------------------------------------------------------------------------------------------------

COMPONENT_IDS = {1: (1,), 2: (0x52, 0x47, 0x42), 3: (1, 2, 3), 4: (0x43, 0x4D, 0x59, 0x4B), 5: (1, 2, 3, 4)}
TABLES = {1: (0,), 2: (0, 0, 0), 3: (0, 1, 1), 4: (0, 0, 0, 0), 5: (0, 1, 1, 0)}


def sub_image(im, comps):
    """the image a scan sees: its components; an interleaved scan keeps the frame's MCU grid (per_scan_setup)"""
    comps = list(comps)
    dims = [blocks_needed(im["image_size"], im["hsamp"], im["vsamp"], c) for c in comps]
    return dict(coefs=[im["coefs"][c][:dims[k][0], :dims[k][1]] for k, c in enumerate(comps)], comps=comps, dims=dims,
                hsamp=[im["hsamp"][c] for c in comps], vsamp=[im["vsamp"][c] for c in comps], image_size=im["image_size"],
                mh=max(im["hsamp"]), mv=max(im["vsamp"]))


def scan_order(sub):
    """(index in the scan, block or None for a dummy, MCU index) in scan order"""
    n = len(sub["coefs"])
    if n == 1:
        hb, wb = sub["dims"][0]
        for by in range(hb):
            for bx in range(wb):
                yield 0, sub["coefs"][0][by, bx], by * wb + bx
        return
    w, h = sub["image_size"]
    mx_n, my_n = -(-w // (8 * sub["mh"])), -(-h // (8 * sub["mv"]))
    for my in range(my_n):
        for mx in range(mx_n):
            for c in range(n):
                for y in range(sub["vsamp"][c]):
                    for x in range(sub["hsamp"][c]):
                        bx, by = mx * sub["hsamp"][c] + x, my * sub["vsamp"][c] + y
                        real = bx < sub["dims"][c][1] and by < sub["dims"][c][0]
                        yield c, (sub["coefs"][c][by, bx] if real else None), my * mx_n + mx


def scan_mcus(sub):
    """(MCUs per row, MCUs) of the scan"""
    if len(sub["coefs"]) == 1:
        hb, wb = sub["dims"][0]
        return wb, wb * hb
    w, h = sub["image_size"]
    mx = -(-w // (8 * sub["mh"]))
    return mx, mx * -(-h // (8 * sub["mv"]))


def eob_symbol(run):
    n = run.bit_length() - 1
    return (1, n << 4, run & ((1 << n) - 1), n)


def scan_symbols_prog(im, scan, Ri):
    """the scan's symbols by restart interval: [[(is_ac, symbol, bits, nbits, index of the component in the scan)]]; Ri:
    what DRI carries (0: none)"""
    comps, ss, se, ah, al = scan
    assert ah == 0
    sub = sub_image(im, comps)
    _mx, mcus = scan_mcus(sub)
    rim = Ri if 0 < Ri < mcus else 0
    out, prev, eobrun, last_m = [[]], [0] * len(comps), 0, 0

    def flush():
        nonlocal eobrun
        if eobrun:
            out[-1].append(eob_symbol(eobrun) + (0,))
            eobrun = 0

    for c, blk, m in scan_order(sub):
        if rim and m != last_m and m % rim == 0:
            flush()
            out.append([])
            prev = [0] * len(comps)
        last_m = m
        if ss == 0:
            cur = prev[c] if blk is None else int(blk[0]) >> al
            diff = cur - prev[c]
            prev[c] = cur
            nb = nbits(diff)
            if nb > 11:
                raise BadCoef(f"DC difference {diff}")
            out[-1].append((0, nb, (diff if diff >= 0 else diff - 1) & ((1 << nb) - 1), nb, c))
            continue
        r = 0
        for k in range(ss, se + 1):
            v = int(blk[ZIGZAG[k]])
            t = abs(v) >> al
            if t == 0:
                r += 1
                continue
            flush()
            while r > 15:
                out[-1].append((1, 0xF0, 0, 0, 0))
                r -= 16
            nb = t.bit_length()
            if nb > 10:
                raise BadCoef(f"AC value {v}")
            out[-1].append((1, (r << 4) | nb, (t if v > 0 else ~t) & ((1 << nb) - 1), nb, 0))
            r = 0
        if r:
            eobrun += 1
            if eobrun == EOB_MAX:
                flush()
    flush()
    return out


def encode_progressive(im, script, head: bytes, ri=0, rows=0) -> bytes:
    """the whole file: head | per scan DHT(s), [DRI], SOS, segment | EOI"""
    tblf, ids = TABLES[im["colorspace"]], COMPONENT_IDS[im["colorspace"]]
    out, last_dri = bytearray(head), 0
    for scan in script:
        comps, ss, se, ah, al = scan
        sub = sub_image(im, comps)
        mx, _mcus = scan_mcus(sub)
        Ri = min(rows * mx, 65535) if rows > 0 else ri
        intervals = scan_symbols_prog(im, scan, Ri)
        tbl = [tblf[c] for c in comps]
        hist = {}
        for syms in intervals:
            for is_ac, sym, _b, _nb, c in syms:
                hist.setdefault(tbl[c], np.zeros(256, np.int64))[sym] += 1
        codes = {}
        for c in range(len(comps)):                                   # each table once, in component order
            t = tbl[c]
            if t in codes:
                continue
            table = libjpeg_optimal(hist.get(t, np.zeros(256, np.int64)))
            codes[t] = derive(table)
            bits, vals = table
            n = sum(bits[1:17])
            payload = bytes([((1 if ss else 0) << 4) | t]) + bytes(int(b) for b in bits[1:17]) + bytes(int(v) for v in vals[:n])
            out += b"\xff\xc4" + struct.pack(">H", len(payload) + 2) + payload
        if Ri != last_dri:
            out += b"\xff\xdd\x00\x04" + struct.pack(">H", Ri)
            last_dri = Ri
        out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * len(comps), len(comps))
        for k, c in enumerate(comps):
            out += bytes([ids[c], tbl[k] if ss else tbl[k] << 4])
        out += bytes([ss, se, (ah << 4) | al])
        for k, syms in enumerate(intervals):
            if k:
                out += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
            v, n = 0, 0
            for is_ac, sym, bits, nb, c in syms:
                code, size = codes[tbl[c]][sym]
                v = (v << (size + nb)) | (code << nb) | bits
                n += size + nb
            pad = -n % 8
            v = (v << pad) | ((1 << pad) - 1)
            out += stuff(v.to_bytes((n + pad) // 8, "big"))
    return bytes(out + b"\xff\xd9")


def scan_summary(data: bytes):
    """the markers of a file in order, entropy-coded bytes skipped: [(code, payload)]"""
    pos, out = 2, []
    while pos < len(data):
        assert data[pos] == 0xFF, f"marker expected at {pos}"
        code = data[pos + 1]
        if code == 0xD9:
            out.append((code, b""))
            break
        n = struct.unpack_from(">H", data, pos + 2)[0]
        out.append((code, data[pos + 4:pos + 2 + n]))
        pos += 2 + n
        if code == 0xDA:
            while not (data[pos] == 0xFF and data[pos + 1] != 0 and not 0xD0 <= data[pos + 1] <= 0xD7):
                pos += 1
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------

def scripts_for(ncomp, spectral_script):
    """{name: script}: the scripts of the issue for a frame of ncomp components"""
    allc = tuple(range(ncomp))
    out = {"spectral": spectral_script(ncomp),
           "dc only": [(allc, 0, 0, 0, 0)],
           "dc per component": [((c,), 0, 0, 0, 0) for c in range(ncomp)],
           "band 1-1": [(allc, 0, 0, 0, 0)] + [((c,), 1, 1, 0, 0) for c in range(ncomp)],
           "band 1-63": [(allc, 0, 0, 0, 0)] + [((c,), 1, 63, 0, 0) for c in range(ncomp)],
           "band 63-63": [(allc, 0, 0, 0, 0)] + [((c,), 63, 63, 0, 0) for c in range(ncomp)],
           "reversed": [((c,), 0, 0, 0, 0) for c in reversed(range(ncomp))]
                       + [((c,), 1, 63, 0, 0) for c in reversed(range(ncomp))],
           "Al 1": [(allc, 0, 0, 0, 1)] + [((c,), 1, 63, 0, 1) for c in range(ncomp)],
           "Al 2": [(allc, 0, 0, 0, 2)] + [((c,), 1, 5, 0, 2) for c in range(ncomp)] + [((c,), 6, 63, 0, 2) for c in range(ncomp)]}
    return out


RESTARTS = [(0, 0), (1, 0), (5, 0), (0, 1)]                            # (restart_interval, restart_in_rows)


def grid_images():
    """{(layout index, size): image}: every layout of RST_LAYOUTS at every size of PROG_SIZES"""
    out = {}
    for li in RST_LAYOUTS:
        hs, vs, cs = LAYOUTS[li]
        for size in PROG_SIZES:
            out[(li, size)] = synth_scan_image(np.random.default_rng(li * 977 + size[0] * 31 + size[1]), size, hs, vs, cs)
    return out


def complete(script, ncomp) -> bool:
    """every coefficient of every component is sent with Al = 0: libjpeg reads the arrays back"""
    sent = [[False] * 64 for _ in range(ncomp)]
    for comps, ss, se, _ah, al in script:
        for c in comps:
            for k in range(ss, se + 1):
                sent[c][k] = al == 0
    return all(all(s) for s in sent)


def big_mcu_cases():
    """a frame of 4x4, 1x1, 1x1: 18 blocks in the MCU of a scan over all components, which libjpeg refuses, while it writes
    the file scan by scan -> (images by size, {name: script} libjpeg writes, the script it refuses)"""
    ims = {size: synth_scan_image(np.random.default_rng(size[0]), size, [4, 1, 1], [4, 1, 1], 3) for size in ((33, 18), (65, 66))}
    good = {"one component per scan": [((c,), 0, 0, 0, 0) for c in range(3)] + [((c,), 1, 63, 0, 0) for c in range(3)],
            "chroma interleaved": [((0,), 0, 0, 0, 0), ((1, 2), 0, 0, 0, 1), ((2,), 1, 5, 0, 0), ((0,), 1, 63, 0, 0),
                                   ((1,), 1, 63, 0, 0), ((2,), 6, 63, 0, 0)]}
    return ims, good, [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 0)]


BAD_SCRIPTS = {
    "Al 11": lambda n: [(tuple(range(n)), 0, 0, 0, 11)],
    "AC before DC": lambda n: [((0,), 1, 63, 0, 0), (tuple(range(n)), 0, 0, 0, 0)],
    "two components in an AC scan": lambda n: [(tuple(range(n)), 0, 0, 0, 0), ((0, 1), 1, 63, 0, 0)],
    "Ss > Se": lambda n: [(tuple(range(n)), 0, 0, 0, 0), ((0,), 5, 4, 0, 0)],
    "Se > 0 with Ss 0": lambda n: [(tuple(range(n)), 0, 5, 0, 0)],
    "component out of range": lambda n: [(tuple(range(n)), 0, 0, 0, 0), ((n,), 1, 63, 0, 0)],
    "sent twice": lambda n: [(tuple(range(n)), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((0,), 5, 9, 0, 0)],
    "no DC for a component": lambda n: [((0,), 0, 0, 0, 0)],
}
