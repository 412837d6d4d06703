"""Progressive files with successive-approximation refinement scans (Ah > 0): a plain Python restatement of jchuff.c's
encode_mcu_DC_refine / encode_mcu_AC_refine / emit_eobrun / emit_buffered_bits in libjpeg's own order of events, on top
of tests/encode_prog_oracle.py (test only: it pins the rules of DESIGN.md section 17.1 against libjpeg's whole files
before any GPU is involved), the host build of csrc/qs_encode_prog.h for such scripts (tests/encode_refine_host.cpp),
libjpeg's own jpeg_simple_progression (tests/libjpeg9_simple_prog.c) and the crafted images the test modules share."""
import struct

import numpy as np

from encode_oracle import ZIGZAG, derive
from encode_prog_oracle import (COMPONENT_IDS, EOB_MAX, TABLES, ProgHost, eob_symbol, scan_mcus, scan_order, scan_symbols_prog,
                                sub_image)
from encode_rst_oracle import gray_image, stuff
from host_tools import build, run
from huff_oracle import libjpeg_optimal

CORR_MAX = 937                                                          # MAX_CORR_BITS - DCTSIZE2 + 1


class RefineHost(ProgHost):
    """tests/encode_refine_host.cpp: csrc/qs_encode_prog.h in its host form for scripts with refinement scans"""
    SOURCE = "encode_refine_host.cpp"


def libjpeg_simple_progression(workdir, ncomp: int, colorspace: int):
    """tests/libjpeg9_simple_prog.c: cinfo.scan_info after jpeg_simple_progression -> the script"""
    r = run(build("libjpeg9_simple_prog.c", libjpeg=True), ncomp, colorspace)
    out = []
    for line in r.stdout.splitlines():
        v = [int(x) for x in line.split()]
        out.append((tuple(v[1:1 + v[0]]), v[5], v[6], v[7], v[8]))
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------
# an item is (is_ac, symbol, bits, nbits, index of the component in the scan); symbol None: bits without a symbol

def scan_symbols_refine(im, scan, Ri):
    """a refinement scan's items by restart interval, in libjpeg's order of events"""
    comps, ss, se, ah, al = scan
    assert ah > 0
    sub = sub_image(im, comps)
    _mx, mcus = scan_mcus(sub)
    rim = Ri if 0 < Ri < mcus else 0
    out, last_dc, last_m = [[]], [0] * len(comps), 0
    eobrun, be = 0, []                                                  # EOBRUN, and bit_buffer[0 .. BE)

    def raw(bits):
        for b in bits:
            out[-1].append((1, None, b, 1, 0))

    def emit_eobrun():
        nonlocal eobrun, be
        if eobrun:
            out[-1].append(eob_symbol(eobrun) + (0,))
            eobrun = 0
            raw(be)
            be = []

    for c, blk, m in scan_order(sub):
        if rim and m != last_m and m % rim == 0:
            emit_eobrun()
            out.append([])
        last_m = m
        if ss == 0:
            # encode_mcu_DC_refine: the bit Al of the DC; a dummy block repeats the DC in front of it (jctrans.c)
            if blk is not None:
                last_dc[c] = int(blk[0])
            out[-1].append((0, None, (last_dc[c] >> al) & 1, 1, c))
            continue
        absv = [abs(int(blk[ZIGZAG[k]])) >> al for k in range(64)]
        eob = max([k for k in range(ss, se + 1) if absv[k] == 1], default=0)
        r, br = 0, []
        for k in range(ss, se + 1):
            t = absv[k]
            if t == 0:
                r += 1
                continue
            while r > 15 and k <= eob:
                emit_eobrun()
                out[-1].append((1, 0xF0, 0, 0, 0))
                r -= 16
                raw(br)
                br = []
            if t > 1:
                br.append(t & 1)
                continue
            emit_eobrun()
            out[-1].append((1, (r << 4) | 1, 0 if int(blk[ZIGZAG[k]]) < 0 else 1, 1, 0))
            raw(br)
            br = []
            r = 0
        if r > 0 or br:
            eobrun += 1
            be += br
            if eobrun == EOB_MAX or len(be) > CORR_MAX:
                emit_eobrun()
    emit_eobrun()
    return out


def encode_refine(im, script, head: bytes, ri=0, rows=0) -> bytes:
    """the whole file of any progressive script: head | per scan DHT(s) (none in front of a DC refinement), [DRI], SOS,
    segment | EOI"""
    tblf, ids = TABLES[im["colorspace"]], COMPONENT_IDS[im["colorspace"]]
    out, last_dri = bytearray(head), 0
    for scan in script:
        comps, ss, se, ah, al = scan
        sub = sub_image(im, comps)
        mx, _mcus = scan_mcus(sub)
        Ri = min(rows * mx, 65535) if rows > 0 else ri
        intervals = scan_symbols_refine(im, scan, Ri) if ah else scan_symbols_prog(im, scan, Ri)
        tbl = [tblf[c] for c in comps]
        hist = {}
        for syms in intervals:
            for _is_ac, sym, _b, _nb, c in syms:
                if sym is not None:
                    hist.setdefault(tbl[c], np.zeros(256, np.int64))[sym] += 1
        codes = {}
        for c in range(len(comps)):
            t = tbl[c]
            if t in codes or (ss == 0 and ah):
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
            # jcmarker.c emit_sos: a DC refinement names no table at all
            out += bytes([ids[c], tbl[k] if ss else 0 if ah else tbl[k] << 4])
        out += bytes([ss, se, (ah << 4) | al])
        for k, syms in enumerate(intervals):
            if k:
                out += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
            v, n = 0, 0
            for _is_ac, sym, bits, nb, c in syms:
                code, size = codes[tbl[c]][sym] if sym is not None else (0, 0)
                v = (v << (size + nb)) | (code << nb) | bits
                n += size + nb
            pad = -n % 8
            v = (v << pad) | ((1 << pad) - 1)
            out += stuff(v.to_bytes((n + pad) // 8, "big"))
    return bytes(out + b"\xff\xd9")


def run_pieces(im, scan, Ri=0):
    """[(run length, buffered bits)] of every EOB-run symbol of an AC refinement scan, in order (restatement)"""
    out = []
    for syms in scan_symbols_refine(im, scan, Ri):
        for i, s in enumerate(syms):
            if s[1] is not None and s[1] & 15 == 0 and s[1] != 0xF0:
                n = 0
                for t in syms[i + 1:]:
                    if t[1] is not None:
                        break
                    n += 1
                out.append(((1 << (s[1] >> 4)) + s[2], n))
    return out


# ---- scripts -------------------------------------------------------------------------------------------------------------

def refine_scripts(ncomp, colorspace, simple_progression):
    """{name: script}: the scripts of the issue for a frame of ncomp components"""
    allc = tuple(range(ncomp))
    last = ncomp - 1
    return {
        "simple": simple_progression(ncomp, colorspace),
        "dc twice": [(allc, 0, 0, 0, 2), (allc, 0, 0, 2, 1), (allc, 0, 0, 1, 0)] + [((c,), 1, 63, 0, 0) for c in allc],
        # one band at Al = 2 and refined to 0 in two scans while another band is sent whole
        "ac two steps": [(allc, 0, 0, 0, 0)] + [((c,), 1, 5, 0, 0) for c in allc] + [((last,), 6, 63, 0, 2), ((last,), 6, 63, 2, 1),
                                                                                    ((last,), 6, 63, 1, 0)]
                        + [((c,), 6, 63, 0, 0) for c in allc[:-1]],
        "dc per component": [((c,), 0, 0, 0, 1) for c in allc] + [((c,), 0, 0, 1, 0) for c in reversed(allc)]
                            + [((c,), 1, 63, 0, 1) for c in allc] + [((c,), 1, 63, 1, 0) for c in allc],
    }


GRAY_REFINE = [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)]       # gray: the whole AC band, then its last bit


# ---- crafted gray images: the smallest sizes at which each rule of the AC refinement bites --------------------------------
# with GRAY_REFINE a coefficient of +-2 or +-3 was nonzero before the refinement scan (one correction bit), +-1 is newly
# nonzero, 0 stays zero

def _block(pairs, dc=7):
    b = np.zeros(64, np.int16)
    b[0] = dc
    for k, v in pairs.items():
        b[ZIGZAG[k]] = v
    return b


def full_tail(n=63):
    """a block that leaves n correction bits and writes nothing"""
    return _block({k: (3 if k % 3 else -2) for k in range(1, 1 + n)})


def crafted_images():
    """{name: gray image}"""
    out = {}
    # the BE cut: 16 blocks of 63 buffered bits -- the run is cut behind block 15 (945 > 937)
    out["be cut"] = gray_image([full_tail()] * 16, 16)
    # BE exactly 937 after 15 blocks (14 * 63 + 55): no cut; 938: cut
    out["be 937"] = gray_image([full_tail()] * 14 + [full_tail(55), full_tail()], 16)
    out["be 938"] = gray_image([full_tail()] * 14 + [full_tail(56), full_tail()], 16)
    # 40 such blocks: cuts behind blocks 15 and 30; a writing block in the middle of a piece; 0xF0 followed by bits
    zrl = _block({**{k: 2 for k in range(1, 6)}, 30: -1, 31: 3, 60: 1, 63: -3})
    tailless = _block({**{k: -3 for k in range(1, 10)}, 63: 1})              # its last band coefficient is newly nonzero
    folded = _block({3: 1, 5: 2, 40: -1})                               # 23 zeros behind the last new coefficient
    late = _block({**{k: 3 for k in range(1, 20)}, 50: 2, 62: -2})       # 30 zeros, then correction bits: no 0xF0 without EOB
    blocks = [full_tail()] * 20 + [zrl] + [full_tail()] * 19 + [tailless] + [full_tail()] * 17 + [folded, late] \
        + [_block({})] * 3 + [tailless, tailless, _block({})]
    out["mixed"] = gray_image(blocks, len(blocks))
    # workgroup borders: 264 and 520 blocks, pieces and runs across blocks 255 | 256 and 511 | 512
    rng = np.random.default_rng(11)
    for n in (264, 520):
        blocks = []
        for i in range(n):
            kind = rng.integers(0, 10)
            blocks.append(full_tail(int(rng.integers(40, 64))) if kind < 7 else _block({}) if kind < 9 else zrl)
        for i in (250, 506):                                                # a long run in front of each border ...
            if i < n:
                blocks[i] = tailless
                for j in range(i + 1, min(n, i + 12)):
                    blocks[j] = full_tail()
        out[f"border {n}"] = gray_image(blocks, n // 8)
    return out


def big_crafted_images():
    """2048 x 1024 (32 768 blocks) with the band all zero: the 0x7FFF cut.  Both rules in one run need 0x7FFF + 15 blocks,
    more than that image has: 2056 x 1024 (32 896 blocks), 14 tails of 63 bits spread over the first 0x7FFF blocks (882
    bits: the count cuts, and the symbol is followed by buffered bits), then 129 blocks of 63 bits (the bits cut, every 15
    blocks)"""
    zero = np.zeros((32768, 64), np.int16)
    zero[:, 0] = 5
    sparse = np.zeros((32896, 64), np.int16)
    sparse[:, 0] = 5
    sparse[100:100 + 14 * 2300:2300, 1:64] = 2
    sparse[0x7FFF:, 1:64] = -3
    return {"all zero": gray_image(zero, 256), "sparse tails": gray_image(sparse, 257)}
