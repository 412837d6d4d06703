"""Crafted streams for the refusal rules of the three scan readers (tests/test_reader_rules_host.py,
tests/test_gpu_reader_rules.py): a symbol-level scan assembler on top of tests/foreign_files.py -- its headers, table
families and _code_intervals -- a lenient plain-Python decoder that reads as libjpeg 9 reads and has none of the rules
under test, and the cases: one file per rule line of csrc/qs_read.h, qs_read_split.h and qs_read_prog.h that trips that
rule and nothing else, each with an accepted twin that sits exactly on the boundary.

An item is (kind, c, symbol, bits, nbits): kind "dc" | "ac" picks the table family, c the component's index in the scan
(its Td / Ta), symbol the Huffman symbol (None: raw bits without a code), bits / nbits what follows the code.  A scan is
[[[item] per block] per restart interval].

    PYTHONPATH=. python tests/crafted_streams.py record     rewrites tests/golden/reader_rules.json from libjpeg 9's reads"""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

from decode_oracle import blocks_needed
from encode_oracle import ZIGZAG, block_symbols, derive, nbits, scan_blocks, synth_scan_image
from encode_prog_oracle import eob_symbol, scan_mcus, scan_order, sub_image
from encode_rst_oracle import mcu_geometry
from foreign_files import _File, _code_intervals, foreign_tables, jpeg_file
from read_oracle import expected_arrays, true_shapes
from read_prog_oracle import expected_arrays as expected_arrays_prog

FIXTURE = Path(__file__).resolve().parent / "golden" / "reader_rules.json"
OK, LENGTH, CODE = 0, 2, 3                                            # QS_RD_OK, QS_RD_LENGTH, QS_RD_CODE
NO_CODE = ("raw", 0, None, 0x1FFFF, 17)    # 16 one-bits start no code of either family; libjpeg takes 17 bits and reads symbol 0


# ---- arrays -> items, block by block --------------------------------------------------------------------------------------

def baseline_blocks(im, restart):
    """the sequential scan of the image dict's arrays: encode_one_block's symbols (encode_oracle.block_symbols) block by
    block, the DC prediction restarting with every interval"""
    _mx, mcus, bpm = mcu_geometry(im)
    per = (restart if restart else mcus) * bpm
    out, prev = [], None
    for b, (c, blk) in enumerate(scan_blocks(im)):
        if b % per == 0:
            out.append([])
            prev = [0] * len(im["coefs"])
        out[-1].append([("ac" if is_ac else "dc", c, sym, bits, nb) for is_ac, sym, bits, nb in block_symbols(blk, prev[c])])
        prev[c] = int(blk[0])
    return out


def _scan_intervals(im, scan, ri):
    """[[(index of the component in the scan, block or None for a dummy)] per interval] of a progressive scan"""
    sub = sub_image(im, scan[0])
    _mx, mcus = scan_mcus(sub)
    rim = ri if 0 < ri < mcus else 0
    out, last_m = [[]], 0
    for c, blk, m in scan_order(sub):
        if rim and m != last_m and m % rim == 0:
            out.append([])
        last_m = m
        out[-1].append((c, blk))
    return out


def _ac_first_block(blk, ss, se, al):
    """-> (the symbols up to the last non-zero value, whether an EOB follows, [])"""
    body, r = [], 0
    for k in range(ss, se + 1):
        v = int(blk[ZIGZAG[k]])
        t = abs(v) >> al
        if t == 0:
            r += 1
            continue
        while r > 15:
            body.append(("ac", 0, 0xF0, 0, 0))
            r -= 16
        nb = t.bit_length()
        body.append(("ac", 0, (r << 4) | nb, (t if v > 0 else ~t) & ((1 << nb) - 1), nb))
        r = 0
    return body, r > 0, []


def _ac_refine_block(blk, ss, se, al):
    """encode_mcu_AC_refine -> (the symbols up to the last newly non-zero value with the correction bits they pass,
    whether the block joins an EOB run, the correction bits behind the last symbol)"""
    absv = [abs(int(blk[ZIGZAG[k]])) >> al for k in range(64)]
    eob = max([k for k in range(ss, se + 1) if absv[k] == 1], default=0)
    body, r, br = [], 0, []
    for k in range(ss, se + 1):
        t = absv[k]
        if t == 0:
            r += 1
            continue
        while r > 15 and k <= eob:
            body.append(("ac", 0, 0xF0, 0, 0))
            r -= 16
            body += br
            br = []
        if t > 1:
            br.append(("raw", 0, None, t & 1, 1))
            continue
        body.append(("ac", 0, (r << 4) | 1, 0 if int(blk[ZIGZAG[k]]) < 0 else 1, 1))
        body += br
        br, r = [], 0
    return body, r > 0 or bool(br), br


def progressive_blocks(im, scan, ri):
    """one scan of a progressive file block by block, as the DECODER meets the items: an EOB run's symbol stands in the
    block the run starts in, behind that block's last value, and each block of the run holds its own correction bits.
    Flattened, that is the order jcphuff.c writes them in (tests/encode_prog_oracle.py, encode_refine_oracle.py)"""
    _comps, ss, se, ah, al = scan
    out = []
    for blocks in _scan_intervals(im, scan, ri):
        iv, prev, run = [], {}, None
        for c, blk in blocks:
            if ss == 0 and ah == 0:
                cur = prev.get(c, 0) if blk is None else int(blk[0]) >> al
                diff = cur - prev.get(c, 0)
                prev[c] = cur
                nb = nbits(diff)
                iv.append([("dc", c, nb, (diff if diff >= 0 else diff - 1) & ((1 << nb) - 1), nb)])
            elif ss == 0:
                if blk is not None:
                    prev[c] = int(blk[0])                              # (a dummy repeats the DC in front of it: jctrans.c)
                iv.append([("raw", c, None, (prev.get(c, 0) >> al) & 1, 1)])
            else:
                body, eob, tail = (_ac_refine_block if ah else _ac_first_block)(blk, ss, se, al)
                if eob and run is not None and not body:
                    run[1] += 1
                    iv.append(list(tail))
                    continue
                if run is not None:
                    run[0][run[2]] = ("ac", 0) + eob_symbol(run[1])[1:]
                    run = None
                items = body + ([None] if eob else []) + tail
                if eob:
                    run = [items, 1, len(body)]
                iv.append(items)
        if run is not None:
            run[0][run[2]] = ("ac", 0) + eob_symbol(run[1])[1:]
        out.append(iv)
    return out


# ---- items -> a whole file ------------------------------------------------------------------------------------------------

def _coded(intervals, codes):
    """items -> _code_intervals' (code, size, bits, nbits); codes: {kind: [{symbol: (code, size)} per scan component]}"""
    return [[((0, 0) if sym is None else codes[kind][c][sym]) + (bits, nb) for blk in iv for kind, c, sym, bits, nb in blk]
            for iv in intervals]


def write_baseline_items(im, intervals, *, tables, dc_ids=None, ac_ids=None, restart=0) -> dict:
    """foreign_files.write_baseline with the scan given as items; tables: fixed ({("dc" | "ac", id): (bits, huffval)})"""
    f = _File(im, None, False, False, dc_ids, ac_ids, tables, b"")
    n = len(im["coefs"])
    dcc, acc = f.scan_tables("dc", f.dc_ids, None), f.scan_tables("ac", f.ac_ids, None)
    f.restart(int(restart), False)
    f.sos(range(n), [(f.dc_ids[c] << 4) | f.ac_ids[c] for c in range(n)], 0, 63, 0, 0, f.dc_ids, f.ac_ids)
    codes = dict(dc=[dcc[t] for t in f.dc_ids], ac=[acc[t] for t in f.ac_ids])
    f.segment(_code_intervals(_coded(intervals, codes), True, 0), b"")
    return f.close(im, 0, b"")


def write_progressive_items(im, script, scans, *, tables, dc_ids=None, ac_ids=None, restart=0) -> dict:
    """foreign_files.write_progressive with every scan given as items; restart may be a list, cycled over the scans"""
    f = _File(im, None, False, True, dc_ids, ac_ids, tables, b"")
    cycle = list(restart) if isinstance(restart, (list, tuple)) else [restart]
    for i, (scan, intervals) in enumerate(zip(script, scans)):
        comps, ss, se, ah, al = scan
        ids = [(f.ac_ids if ss else f.dc_ids)[c] for c in comps]
        codes = {}
        if ss or not ah:
            t = f.scan_tables("ac" if ss else "dc", ids, None)
            codes = {"ac" if ss else "dc": [t[x] for x in ids]}
        f.restart(int(cycle[i % len(cycle)]), False)
        f.sos(comps, [t if ss else 0 if ah else t << 4 for t in ids], ss, se, ah, al,
              [0 if ss or ah else t for t in ids], [t if ss else 0 for t in ids])
        f.segment(_code_intervals(_coded(intervals, codes), True, 0), b"")
    return f.close(im, 0, b"")


def interval_bits(iv, codes) -> int:
    """the bits the blocks of one interval take"""
    return sum(size + nb for _c, size, _b, nb in _coded([iv], codes)[0])


# ---- the lenient decoder --------------------------------------------------------------------------------------------------
# libjpeg 9's own permissive reading (jdhuff.c), bit by bit: bits that start no code are 17 bits and symbol 0, a run may
# pass the band's end or coefficient 63 (the value is dropped), any s is one bit in an AC refinement, a correction bit is
# applied whatever the coefficient holds, an EOB run ends with its interval, and nothing is said about the bits an interval
# has left or lacks: they are counted.

class _Bits:
    def __init__(self, raw):
        self.v, self.n, self.p = int.from_bytes(raw, "big"), 8 * len(raw), 0

    def get(self, k):
        out = 0
        for _ in range(k):
            out = (out << 1) | ((self.v >> (self.n - 1 - self.p)) & 1 if self.p < self.n else 0)
            self.p += 1
        return out

    def symbol(self, inv):
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.get(1)
            if (l, code) in inv:
                return inv[(l, code)]
        self.get(1)
        return 0


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _inverse(table):
    return {(l, code): sym for sym, (code, l) in derive(table).items()}


def _scan_bytes(data, offset):
    """the restart intervals of the scan at `offset`, unstuffed"""
    out, cur, i = [], bytearray(), offset
    while True:
        if data[i] == 0xFF and data[i + 1] != 0:
            out.append(bytes(cur))
            if not 0xD0 <= data[i + 1] <= 0xD7:
                return out
            cur = bytearray()
            i += 2
            continue
        cur.append(data[i])
        i += 2 if data[i] == 0xFF else 1


def _positions(p, comps):
    """[(index in the scan, by, bx)] in scan order, MCU by MCU, and the MCUs of the scan; dummy blocks included (the
    lenient decoder keeps them in arrays padded to the MCU grid, as libjpeg does)"""
    hs, vs = p["hsamp"], p["vsamp"]
    if len(comps) == 1:
        hb, wb = blocks_needed(p["image_size"], hs, vs, comps[0])
        return [[(0, by, bx)] for by in range(hb) for bx in range(wb)]
    w, h = p["image_size"]
    mxn, myn = -(-w // (8 * max(hs))), -(-h // (8 * max(vs)))
    return [[(k, my * vs[c] + y, mx * hs[c] + x) for k, c in enumerate(comps) for y in range(vs[c]) for x in range(hs[c])]
            for my in range(myn) for mx in range(mxn)]


def _lenient_block(b, blk, c, kind, ss, se, al, state, dct, act):
    """one block of scan component c; state: dict(pred: per component, eobrun) of the interval"""
    if kind == "base" or (ss == 0 and kind == "first"):
        s = b.symbol(dct)
        state["pred"][c] += _extend(b.get(s), s)
        blk[0] = (((state["pred"][c] << al) + 32768) % 65536) - 32768
        if kind != "base":
            return
        k = 1
        while k < 64:
            sym = b.symbol(act)
            r, s = sym >> 4, sym & 15
            if s:
                k += r
                v = _extend(b.get(s), s)
                if k <= 63:
                    blk[ZIGZAG[k]] = v
            elif r != 15:
                break
            else:
                k += 15
            k += 1
    elif ss == 0:
        if b.get(1):
            blk[0] |= 1 << al
    elif kind == "first":
        if state["eobrun"]:
            state["eobrun"] -= 1
            return
        k = ss
        while k <= se:
            sym = b.symbol(act)
            r, s = sym >> 4, sym & 15
            if s:
                k += r
                v = _extend(b.get(s), s)
                if k <= 63:
                    blk[ZIGZAG[k]] = v << al
            elif r != 15:
                state["eobrun"] = (1 << r) + b.get(r) - 1
                break
            else:
                k += 15
            k += 1
    else:
        p1, k = 1 << al, ss

        def correct(c):
            if b.get(1):
                blk[c] += p1 if blk[c] >= 0 else -p1
        if state["eobrun"] == 0:
            while k <= se:
                sym = b.symbol(act)
                r, s = sym >> 4, sym & 15
                val = 0
                if s:
                    val = p1 if b.get(1) else -p1
                elif r != 15:
                    state["eobrun"] = (1 << r) + b.get(r)
                    break
                while k <= se:
                    if blk[ZIGZAG[k]]:
                        correct(ZIGZAG[k])
                    else:
                        r -= 1
                        if r < 0:
                            break
                    k += 1
                if val and k <= 63:
                    blk[ZIGZAG[k]] = val
                k += 1
        if state["eobrun"] > 0:
            while k <= se:
                if blk[ZIGZAG[k]]:
                    correct(ZIGZAG[k])
                k += 1
            state["eobrun"] -= 1


def lenient_slack(data, kind):
    """-> [[bits left in each interval behind its last block (negative: bits taken from behind its end)] per scan] of a
    whole file, read leniently; kind "base" | "prog"; also checks that every scan has the intervals its DRI asks for"""
    p = jpeg_file.parse(data) if kind == "base" else jpeg_file.parse_progressive(data)
    n = len(p["hsamp"])
    if kind == "base":
        scans = [dict(comps=list(range(n)), ss=0, se=63, ah=0, al=0, dc_tbl=p["dc_tbl"], ac_tbl=p["ac_tbl"], dc=p["dc"],
                      ac=p["ac"], restart_interval=p["restart_interval"], offset=p["scan_offset"])]
    else:
        scans = p["scans"]
    hs, vs = p["hsamp"], p["vsamp"]
    w, h = p["image_size"]
    grid = [(-(-h // (8 * max(vs))) * vs[c], -(-w // (8 * max(hs))) * hs[c]) for c in range(n)]
    arrs = [np.zeros((gh, gw, 64), np.int64) for gh, gw in grid]
    out = []
    for s in scans:
        mcus = _positions(p, s["comps"])
        ri = s["restart_interval"] if 0 < s["restart_interval"] < len(mcus) else len(mcus)
        raws = _scan_bytes(data, s["offset"])
        assert len(raws) == -(-len(mcus) // ri), "the intervals of a scan"
        how = "base" if kind == "base" else "refine" if s["ah"] else "first"
        slack = []
        for r, raw in enumerate(raws):
            b = _Bits(raw)
            state = dict(pred=[0] * len(s["comps"]), eobrun=0)
            for mcu in mcus[r * ri:(r + 1) * ri]:
                for k, by, bx in mcu:
                    dct = _inverse(s["dc"][s["dc_tbl"][k]]) if s["ss"] == 0 and not s["ah"] else None
                    act = _inverse(s["ac"][s["ac_tbl"][k]]) if s["se"] else None
                    _lenient_block(b, arrs[s["comps"][k]][by, bx], k, how, s["ss"], s["se"], s["al"], state, dct, act)
            slack.append(b.n - b.p)
        out.append(slack)
    return out


# ---- the frames -----------------------------------------------------------------------------------------------------------

FRAMES = {"gray": ((24, 16), [1], [1], 1), "420": ((33, 17), [2, 1, 1], [2, 1, 1], 3), "444": ((17, 9), [1, 1, 1], [1, 1, 1], 3)}
RI = {"gray": 2, "420": 1, "444": 2}
# the three places of a violation: the first block of an interval, the last block of the last interval, and a dummy block
# of an edge MCU outside the caller's array (4:2:0 at 33 x 17: the luma array is 5 blocks wide, MCU 2 holds column 5)
PLACES = {"first": ("gray", 0, 0), "last": ("444", -1, -1), "dummy": ("420", 2, 1)}


def _frame(name, seed=7):
    size, hs, vs, cs = FRAMES[name]
    return synth_scan_image(np.random.default_rng(seed), size, hs, vs, cs, amp=20, density=0.2)


def _tables(im, dc=None):
    n = len(im["coefs"])
    ids = jpeg_file.table_assignment(im["colorspace"], n)
    t = foreign_tables(ids, ids)
    if dc is not None:
        for i in set(ids):
            t[("dc", i)] = dc
    return t


WIDE_DC = ([0] * 5 + [16] + [0] * 11, list(range(16)))               # sixteen 5-bit codes: the categories 0 .. 15


def _dc_item(diff):
    nb = nbits(diff)
    return ("dc", 0, nb, (diff if diff >= 0 else diff - 1) & ((1 << nb) - 1), nb)


def _ac(sym, bits=1):
    s = sym & 15
    return ("ac", 0, sym, bits & ((1 << s) - 1), s)


def _raw(bits, n=1):
    return ("raw", 0, None, bits, n)


def _case(name, kind, rule, f, want, **more):
    return dict(name=name, kind=kind, rule=rule, data=f["data"], want_status=want, **more)


# ---- the baseline cases ---------------------------------------------------------------------------------------------------

# the AC items of one block: a run that lands on 63 / 64, a ZRL that arrives at 63 / passes it (no EOB follows a block
# that ends on 63)
RUN_63 = [_ac(0xF1), _ac(0xF1), _ac(0xF1), _ac(0xE1)]
RUN_64 = [_ac(0xF1), _ac(0xF1), _ac(0xF1), _ac(0xF1)]
ZRL_63 = [_ac(0xF1), _ac(0xF1), _ac(0xE1), _ac(0xF0)]
ZRL_64 = [_ac(0xF1), _ac(0xF1), _ac(0xF1), _ac(0xF0)]


def _tuned(build, want_mod):
    """build(s, t) -> (file dict, bits of the edited interval) for value sizes s, t; the first whose bits are want_mod
    modulo 8"""
    for s in range(1, 11):
        for t in range(1, 11):
            f, bits = build(s, t)
            if bits % 8 == want_mod:
                return f
    raise AssertionError("no sizes give the residue")


def baseline_cases():
    out = []

    def add(name, rule, frame, edit, want, tables=None, **more):
        im = _frame(frame)
        ivs = baseline_blocks(im, RI[frame])
        edit(ivs)
        f = write_baseline_items(im, ivs, tables=tables or _tables(im), restart=RI[frame])
        out.append(_case(name, "base", rule, f, want, **more))

    def ac_edit(place, items):
        _frame_name, iv, blk = PLACES[place]

        def edit(ivs):
            ivs[iv][blk] = [ivs[iv][blk][0]] + [(k, ivs[iv][blk][0][1]) + tuple(rest) for k, _c, *rest in items]
        return edit

    def dc_edit(place, item):
        _frame_name, iv, blk = PLACES[place]

        def edit(ivs):                                                 # (libjpeg reads NO_CODE as the difference 0)
            ivs[iv][blk] = [(item[0], ivs[iv][blk][0][1]) + tuple(item[2:])] + ivs[iv][blk][1:]
        return edit

    both = "qs_read.h:%d qs_read_split.h:%s"
    for place, (frame, _iv, _blk) in PLACES.items():
        add(f"base run lands on 64, {place}", both % (317, "228,242"), frame, ac_edit(place, RUN_64), CODE,
            twin=f"base run lands on 63, {place}")
        add(f"base run lands on 63, {place}", None, frame, ac_edit(place, RUN_63), OK)
        add(f"base ZRL passes 63, {place}", both % (324, "236,242"), frame, ac_edit(place, ZRL_64), CODE,
            twin=f"base ZRL arrives at 63, {place}")
        add(f"base ZRL arrives at 63, {place}", None, frame, ac_edit(place, ZRL_63), OK)
        add(f"base no AC code, {place}", both % (312, "203"), frame, ac_edit(place, [NO_CODE]), CODE,
            twin=f"base EOB alone, {place}")
        add(f"base EOB alone, {place}", None, frame, ac_edit(place, [_ac(0x00)]), OK)
        add(f"base no DC code, {place}", both % (300, "203"), frame, dc_edit(place, NO_CODE), CODE,
            twin=f"base DC difference 0, {place}")
        add(f"base DC difference 0, {place}", None, frame, dc_edit(place, ("dc", 0, 0, 0, 0)), OK)

    # the two LENGTH forms, in the first and in the last interval of the gray frame: the edited block ends on 63 with a
    # value, so its last item can lose a bit
    im = _frame("gray")
    tabs = _tables(im)
    codes = dict(dc=[derive(tabs[("dc", 0)])], ac=[derive(tabs[("ac", 0)])])
    for where, iv in (("first interval", 0), ("last interval", -1)):
        def build(s, t, spare=False, short=False):
            ivs = baseline_blocks(im, RI["gray"])
            last = _ac(0xE0 | t, (1 << t) - 2)                         # a value at 1, runs to 16, 32 (ZRL), 48 (ZRL) and 63
            if short:
                last = last[:3] + (last[3] >> 1, last[4] - 1)
            ivs[iv][-1] = [ivs[iv][-1][0], _ac(s, 1 << (s - 1)), _ac(0xE0 | 1), _ac(0xF0), _ac(0xF0), last]
            bits = interval_bits(ivs[iv], codes)
            if spare:
                ivs[iv][-1].append(_raw(0xFF, 8))
            return write_baseline_items(im, ivs, tables=tabs, restart=RI["gray"]), bits
        on_byte = _tuned(build, 0)
        out.append(_case(f"base blocks end on the byte boundary, {where}", "base", None, on_byte, OK))
        out.append(_case(f"base a whole spare byte, {where}", "base", "qs_read.h:336 qs_read_split.h:254",
                         _tuned(lambda s, t: build(s, t, spare=True), 0), LENGTH, slack=(iv, 8),
                         twin=f"base seven spare pad bits, {where}"))
        out.append(_case(f"base seven spare pad bits, {where}", "base", None, _tuned(build, 1), OK))
        out.append(_case(f"base one bit short, {where}", "base", "qs_read.h:327 qs_read_split.h:216,395",
                         _tuned(lambda s, t: build(s, t, short=True), 0), LENGTH, slack=(iv, -1),
                         twin=f"base blocks end on the byte boundary, {where}"))

    # DC categories 12 .. 15: the prediction leaves int16 and returns; accepted, libjpeg's arrays
    def wide(ivs):
        diffs = [[20000, 20000], [-20000, -20000], [32767, 1]]
        for iv, ds in zip(ivs, diffs):
            for blk, d in zip(iv, ds):
                blk[0] = _dc_item(d)
    add("base DC categories 12 to 15, the prediction leaves int16", None, "gray", wide, OK,
        tables=_tables(_frame("gray"), WIDE_DC))
    return out


# ---- the split route's own places -----------------------------------------------------------------------------------------

def _runs_to(k, target, c):
    """valued runs from the last written coefficient k that land on `target`: run 15 while it is further than 16 away"""
    out = []
    while target - k > 16:
        out.append(("ac", c, 0xF1, 1, 1))
        k += 16
    out.append(("ac", c, ((target - k - 1) << 4) | 1, 1, 1))
    return out


def split_cases():
    """4:2:0 without DRI: one interval of 36 blocks, long enough for two segments of 256 bytes.  The offending symbol --
    the last run of a block, or bits without a code -- straddles the boundary at byte 256, or starts the second segment:
    the block that holds bit 2048 keeps its first items, then three values whose sizes place what follows"""
    im = _frame("420")
    for c in im["coefs"]:                                               # 30 values a block: the scan passes 256 bytes early
        z = [ZIGZAG[k] for k in range(1, 31)]
        c[..., z] = np.where(c[..., z] == 0, 5, c[..., z])
        c[..., [ZIGZAG[k] for k in range(31, 64)]] = 0
    tabs = _tables(im)
    n = len(im["coefs"])
    ids = jpeg_file.table_assignment(im["colorspace"], n)
    codes = dict(dc=[derive(tabs[("dc", t)]) for t in ids], ac=[derive(tabs[("ac", t)]) for t in ids])
    base = baseline_blocks(im, 0)
    assert len(base) == 1

    def position(items):
        """the bit behind `items` from the interval's start, counted in the stuffed stream"""
        v, nb = 0, 0
        for code, size, bits, n in _coded([[items]], codes)[0]:
            v, nb = (v << (size + n)) | (code << n) | bits, nb + size + n
        return nb + 8 * (v >> (nb % 8)).to_bytes(nb // 8, "big").count(0xFF)

    def value(c, s):
        return ("ac", c, s, 1 << (s - 1), s)

    out = []
    for tail_name in ("run lands on 64", "no AC code"):
        for want in ("straddles the segment boundary", "starts the second segment"):
            found = None
            flat = []
            for blk, items in enumerate(base[0]):
                for j in range(1, len(items)):
                    kept = items[:j]
                    p0 = position(flat + kept)
                    c = items[0][1]
                    k = sum((x[2] >> 4) + 1 for x in kept[1:])          # the last coefficient the kept items wrote
                    pre = interval_bits([_runs_to(k + 3, 64, c)[:-1]], codes) if tail_name.startswith("run") else 0
                    if not 2048 - pre - 62 <= p0 <= 2048 - pre - 28 or found:   # (three values take 30 to 57 bits)
                        continue
                    for s, t, u in ((s, t, u) for s in range(1, 11) for t in range(1, 11) for u in range(1, 11)):
                        lead = kept + [value(c, s), value(c, t), value(c, u)]
                        bad = _runs_to(k + 3, 64, c) if tail_name.startswith("run") else [("raw", c) + NO_CODE[2:]]
                        start = position(flat + lead + bad[:-1])
                        size = interval_bits([bad[-1:]], codes)
                        if (start < 2048 < start + size) if want.startswith("straddles") else start == 2048:
                            found = (blk, lead, k + 3, c)
                            break
                flat += items
            assert found, (tail_name, want)
            blk, lead, k, c = found
            twin = f"split twin of {tail_name}: the symbol {want}"
            for refused in (True, False):
                if tail_name.startswith("run"):
                    tail = _runs_to(k, 64 if refused else 63, c)
                else:
                    tail = [("raw", c) + NO_CODE[2:]] if refused else [("ac", c, 0, 0, 0)]
                ivs = [[list(b) for b in base[0]]]
                ivs[0][blk] = lead + tail
                f = write_baseline_items(im, ivs, tables=tabs, restart=0)
                if refused:
                    out.append(_case(f"split {tail_name}: the symbol {want}", "base",
                                     "qs_read_split.h:228,242" if tail_name.startswith("run") else "qs_read_split.h:203", f, CODE,
                                     twin=twin, boundary=(want, 2048)))
                else:
                    out.append(_case(twin, "base", None, f, OK))
    return out


# ---- the progressive cases ------------------------------------------------------------------------------------------------

def _spectral(n):
    """no successive approximation: DC, then per component the bands 1 .. 5 and 6 .. 63"""
    return [(tuple(range(n)), 0, 0, 0, 0)] + [s for c in range(n) for s in (((c,), 1, 5, 0, 0), ((c,), 6, 63, 0, 0))]


def _refining(n):
    """component 0 in two bands at Al 1, refined; its band 1 .. 5 last: the scan the refinement cases edit"""
    return ([(tuple(range(n)), 0, 0, 0, 0), ((0,), 1, 5, 0, 1), ((0,), 6, 63, 0, 1)] + [((c,), 1, 63, 0, 0) for c in range(1, n)]
            + [((0,), 6, 63, 1, 0), ((0,), 1, 5, 1, 0)])


def _prog_frame(name):
    """the frame with component 0 shaped so that no block of its AC scans joins an EOB run and every block of the
    refinement of 1 .. 5 is the same three items: zigzag 2 is history (4: one correction bit, 0), zigzag 5 becomes
    non-zero (1), the band 6 .. 63 is non-zero at both ends"""
    im = _frame(name)
    a = im["coefs"][0]
    a[..., [ZIGZAG[k] for k in (1, 3, 4)]] = 0
    a[..., ZIGZAG[2]] = 4
    a[..., ZIGZAG[5]] = 1
    a[..., ZIGZAG[6]] = 2
    a[..., ZIGZAG[63]] = 2
    return im


def progressive_cases():
    out = []

    def add(name, rule, frame, script_of, scan, edit, want, ri=None, tables=None, **more):
        im = _prog_frame(frame)
        script = script_of(len(im["coefs"]))
        ri = RI[frame] if ri is None else ri
        scans = [progressive_blocks(im, s, ri) for s in script]
        edit(scans[scan])
        f = write_progressive_items(im, script, scans, tables=tables or _tables(im), restart=ri)
        out.append(_case(name, "prog", rule, f, want, **more))

    def put(iv, blk, items, then=None):
        def edit(ivs):
            c = ivs[iv][blk][0][1] if ivs[iv][blk] else 0
            ivs[iv][blk] = [(k, c) + tuple(rest) for k, _c, *rest in items]
            if then is not None:
                ivs[iv][blk + 1] = list(then)
        return edit

    # DC first: bits without a code, at the three places (the interleaved DC scan is the one with dummy blocks)
    for place, (frame, iv, blk) in PLACES.items():
        add(f"prog DC first: no code, {place}", "qs_read_prog.h:182", frame, _spectral, 0, put(iv, blk, [NO_CODE]), CODE,
            twin=f"prog DC first: difference 0, {place}")
        add(f"prog DC first: difference 0, {place}", None, frame, _spectral, 0, put(iv, blk, [("dc", 0, 0, 0, 0)]), OK)
    # AC scans carry one component and no dummy blocks: the first block of an interval and the last of the last one.  In
    # both frames component 0 has intervals of two blocks (gray 3 x 2 blocks, 4:4:4 3 x 2 blocks, Ri 2)
    for place in ("first", "last"):
        frame, iv, blk = PLACES[place]
        # AC first, band 1 .. 5 (scan 1) and band 6 .. 63 (scan 2)
        add(f"prog AC first: run lands on Se + 1, {place}", "qs_read_prog.h:216", frame, _spectral, 1, put(iv, blk, [_ac(0x51)]),
            CODE,             twin=f"prog AC first: run lands on Se, {place}")
        add(f"prog AC first: run lands on Se, {place}", None, frame, _spectral, 1, put(iv, blk, [_ac(0x41)]), OK)
        add(f"prog AC first: ZRL passes Se, {place}", "qs_read_prog.h:231", frame, _spectral, 2,
            put(iv, blk, [_ac(0xF1), _ac(0xF1), _ac(0xA1), _ac(0xF0)]), CODE, twin=f"prog AC first: ZRL arrives at Se, {place}")
        add(f"prog AC first: ZRL arrives at Se, {place}", None, frame, _spectral, 2,
            put(iv, blk, [_ac(0xF1), _ac(0xF1), _ac(0x91), _ac(0xF0)]), OK)
        # (in the band 6 .. 63: a reader without the rule would take the bits for a value and a run, and in the short band
        # it runs into the next rule)
        add(f"prog AC first: no code, {place}", "qs_read_prog.h:212", frame, _spectral, 2, put(iv, blk, [NO_CODE]), CODE,
            twin=f"prog AC first: EOB, {place}")
        add(f"prog AC first: EOB, {place}", None, frame, _spectral, 2, put(iv, blk, [_ac(0x00)]), OK)
        # AC refinement of 1 .. 5 (the last scan); history at zigzag 2: one correction bit where the run passes it
        last = len(_refining(len(FRAMES[frame][1]))) - 1
        add(f"prog AC refine: s = 2, {place}", "qs_read_prog.h:258", frame, _refining, last,
            put(iv, blk, [("ac", 0, 0x32, 1, 1), _raw(0)]), CODE, twin=f"prog AC refine: run lands on Se past history, {place}")
        add(f"prog AC refine: run passes Se past history, {place}", "qs_read_prog.h:276", frame, _refining, last,
            put(iv, blk, [_ac(0x41), _raw(0)]), CODE, twin=f"prog AC refine: run lands on Se past history, {place}")
        add(f"prog AC refine: run lands on Se past history, {place}", None, frame, _refining, last,
            put(iv, blk, [_ac(0x31), _raw(1)]), OK)
        add(f"prog AC refine: no code, {place}", "qs_read_prog.h:254", frame, _refining, last, put(iv, blk, [NO_CODE, _raw(0)]),
            CODE, twin=f"prog AC refine: EOB, {place}")
        add(f"prog AC refine: EOB, {place}", None, frame, _refining, last, put(iv, blk, [_ac(0x00), _raw(1)]), OK)
    # EOB runs: EOB1 is the symbol 0x10 and one bit: a run of 2 + bit blocks
    for frame, iv in (("gray", 0), ("444", -1)):
        tag = "first interval" if iv == 0 else "last interval"
        last = len(_refining(len(FRAMES[frame][1]))) - 1
        add(f"prog AC first: EOB run of left + 1 from the last block, {tag}", "qs_read_prog.h:226", frame, _spectral, 1,
            put(iv, 1, [("ac", 0, 0x10, 0, 1)]), CODE, twin=f"prog AC first: EOB run of left from the last block, {tag}")
        add(f"prog AC first: EOB run of left from the last block, {tag}", None, frame, _spectral, 1, put(iv, 1, [_ac(0x00)]), OK)
        add(f"prog AC first: EOB run of left + 1 over two blocks, {tag}", "qs_read_prog.h:226", frame, _spectral, 1,
            put(iv, 0, [("ac", 0, 0x10, 1, 1)], []), CODE, twin=f"prog AC first: EOB run of left over two blocks, {tag}")
        add(f"prog AC first: EOB run of left over two blocks, {tag}", None, frame, _spectral, 1,
            put(iv, 0, [("ac", 0, 0x10, 0, 1)], []), OK)
        add(f"prog AC refine: EOB run of left + 1 from the last block, {tag}", "qs_read_prog.h:267", frame, _refining, last,
            put(iv, 1, [("ac", 0, 0x10, 0, 1), _raw(1)]), CODE,
            twin=f"prog AC refine: EOB run of left from the last block, {tag}")
        add(f"prog AC refine: EOB run of left from the last block, {tag}", None, frame, _refining, last,
            put(iv, 1, [_ac(0x00), _raw(1)]), OK)
        add(f"prog AC refine: EOB run of left + 1 over two blocks, {tag}", "qs_read_prog.h:267", frame, _refining, last,
            put(iv, 0, [("ac", 0, 0x10, 1, 1), _raw(1)], [_raw(0)]), CODE,
            twin=f"prog AC refine: EOB run of left over two blocks, {tag}")
        add(f"prog AC refine: EOB run of left over two blocks, {tag}", None, frame, _refining, last,
            put(iv, 0, [("ac", 0, 0x10, 0, 1), _raw(1)], [_raw(0)]), OK)

    # the two LENGTH forms in the band 6 .. 63 of the gray frame (scan 2 of the spectral script)
    im = _prog_frame("gray")
    tabs = _tables(im)
    script = _spectral(1)
    codes = dict(ac=[derive(tabs[("ac", 0)])])
    for where, iv in (("first interval", 0), ("last interval", -1)):
        def build(s, t, spare=False, short=False):
            scans = [progressive_blocks(im, x, RI["gray"]) for x in script]
            end = _ac(0xF0 | t, (1 << t) - 2)                          # a value at 6, runs to 15, 31 (ZRL), 47 (ZRL) and 63
            if short:
                end = end[:3] + (end[3] >> 1, end[4] - 1)
            scans[2][iv][-1] = [_ac(s, 1 << (s - 1)), _ac(0x81), _ac(0xF0), _ac(0xF0), end]
            bits = interval_bits(scans[2][iv], codes)
            if spare:
                scans[2][iv][-1].append(_raw(0xFF, 8))
            return write_progressive_items(im, script, scans, tables=tabs, restart=RI["gray"]), bits
        out.append(_case(f"prog blocks end on the byte boundary, {where}", "prog", None, _tuned(build, 0), OK))
        out.append(_case(f"prog a whole spare byte, {where}", "prog", "qs_read_prog.h:335",
                         _tuned(lambda s, t: build(s, t, spare=True), 0), LENGTH, slack=(2, iv, 8),
                         twin=f"prog seven spare pad bits, {where}"))
        out.append(_case(f"prog seven spare pad bits, {where}", "prog", None, _tuned(build, 1), OK))
        out.append(_case(f"prog one bit short, {where}", "prog", "qs_read_prog.h:325",
                         _tuned(lambda s, t: build(s, t, short=True), 0), LENGTH, slack=(2, iv, -1),
                         twin=f"prog blocks end on the byte boundary, {where}"))

    # DC first at Al 1 under a table with the categories 12 .. 15: the prediction leaves int16 after << Al; accepted
    im = _frame("gray")
    script = [((0,), 0, 0, 0, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 0, 0)]
    scans = [progressive_blocks(im, s, RI["gray"]) for s in script]
    for iv, ds in zip(scans[0], [[20000, 20000], [-20000, -20000], [32767, 1]]):
        for blk, d in zip(iv, ds):
            blk[0] = _dc_item(d)
    f = write_progressive_items(im, script, scans, tables=_tables(im, WIDE_DC), restart=RI["gray"])
    out.append(_case("prog DC first at Al 1, categories 12 to 15: the prediction leaves int16", "prog", None, f, OK))
    return out


def all_cases():
    return baseline_cases() + split_cases() + progressive_cases()


# ---- libjpeg's verdict ----------------------------------------------------------------------------------------------------

def digest(arrs) -> str:
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a, "<i2").tobytes())
    return h.hexdigest()[:32]


def read_case(lj, c):
    """the case as the host builds and the GPU batches take it, with libjpeg 9's read: verdict "clean" | "warns" |
    "stops", and where it is clean its arrays in the arrays of libjpeg's own geometry"""
    data = c["data"]
    ref, clean = lj.read_bytes(data)
    verdict = "stops" if ref is None else "clean" if clean else "warns"
    if c["kind"] == "prog":
        header = jpeg_file.parse_progressive(data)
        shapes = true_shapes(header)
        want = expected_arrays_prog(ref, shapes, header["script"]) if clean else None
        return dict(c, header=header, shapes=shapes, verdict=verdict, want=want)
    header = jpeg_file.parse(data)
    shapes = true_shapes(header)
    want = expected_arrays(ref, shapes) if clean else None
    return dict(c, header=header, scan=data[header["scan_offset"]:], shapes=shapes, verdict=verdict, want=want)


def rule_lines(rule):
    """"qs_read.h:317 qs_read_split.h:228,242" -> {("qs_read.h", 317), ("qs_read_split.h", 228), ("qs_read_split.h", 242)}"""
    return {(part.split(":")[0], int(l)) for part in (rule or "").split() for l in part.split(":")[1].split(",")}


def routes(c):
    return ("interval", "split") if c["kind"] == "base" else ("progressive",)


def record(lj, note_of):
    """the fixture: per case its name, the status every route must report, libjpeg 9's verdict, the digest of its arrays
    where it reads clean, and for a refused case libjpeg reads clean where DESIGN.md states the stricter status"""
    rows = []
    for c in all_cases():
        r = read_case(lj, c)
        row = dict(name=c["name"], rule=c["rule"], status={k: c["want_status"] for k in routes(c)}, libjpeg=r["verdict"])
        if r["verdict"] == "clean":
            row["digest"] = digest(r["want"])
            if c["want_status"]:
                row["documented"] = note_of(c)
        rows.append(row)
    return rows


def documented_limit(c) -> str:
    """where DESIGN.md states that the readers refuse what libjpeg 9 reads without a warning"""
    if c["kind"] == "base":
        return ("DESIGN.md section 14, Status: 'libjpeg 9 itself reads a run or a ZRL that passes coefficient 63 without a "
                "warning (the spare entries of its zigzag table send the value to coefficient 63); the readers refuse the file'")
    if c["want_status"] == LENGTH:
        return ("DESIGN.md section 18, Statuses: 'libjpeg 9 says nothing about whole bytes left behind the last interval of a "
                "file's last scan (it stops reading at the last MCU); the reader reports them like any other interval's'")
    return ("DESIGN.md section 18, Statuses: 'libjpeg only warns on, or silently accepts, some of these (it stores a "
            "coefficient past `Se`, and lets an EOB run end with the interval)'")


if __name__ == "__main__":
    import tempfile
    from read_oracle import LibjpegReader
    if sys.argv[1:] == ["record"]:
        with tempfile.TemporaryDirectory() as d:
            rows = record(LibjpegReader(Path(d)), documented_limit)
        FIXTURE.write_text(json.dumps(rows, indent=1) + "\n")
        print(f"{len(rows)} cases -> {FIXTURE}")
