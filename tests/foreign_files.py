"""Files libjpeg 9 does not write, for the three scan readers (tests/test_foreign_files_host.py,
tests/test_gpu_foreign_files.py): a test-side writer of whole baseline and progressive files on top of the suite's
restatements of libjpeg's coders (tests/encode_oracle.py, encode_rst_oracle.py, encode_prog_oracle.py,
encode_refine_oracle.py) and jpeg_file.compose_parts, with the freedoms other encoders take -- table ids up to 3,
Td != Ta, tables defined once behind the frame header and never again, complete non-optimal tables with 16-bit codes, a
DRI that changes from scan to scan, zero pad bits, segments and fill bytes between scans, component ids of any value --
and the corpus of such files.  With every knob at its default the writer gives libjpeg's own bytes
(test_foreign_files_host.py pins that first).  The oracle of every file is libjpeg 9's own read of it
(read_oracle.LibjpegReader), never what the writer meant to write."""
import struct

import numpy as np

from encode_oracle import LAYOUTS, derive, synth_scan_image
from encode_prog_oracle import scan_mcus, scan_symbols_prog, sub_image
from encode_refine_oracle import GRAY_REFINE, refine_scripts, scan_symbols_refine
from encode_rst_oracle import interval_symbols, stuff
from huff_oracle import libjpeg_optimal
from read_oracle import expected_arrays, padded_shapes, pkg
from read_prog_oracle import expected_arrays as expected_arrays_prog

jpeg_file = pkg.jpeg_file

# ---- the two table families ------------------------------------------------------------------------------------------------

LONG_AC = [0x00, 0xF0, 0x01, 0x10, 0x20, 0x11, 0x02, 0x21, 0x30]     # the symbols of the nine 16-bit AC codes


def _rot(v, k):
    k %= len(v)
    return list(v[k:]) + list(v[:k])


def foreign_ac_table(t: int):
    """AC table of id t: all 256 symbols; one code each of 2 .. 8 bits, 240 codes of 9 bits and 9 codes of 16 bits (the
    all-ones code stays unused: the 16-bit codes follow the 9-bit ones far below it).  The 16-bit codes go to EOB, ZRL, the
    EOB runs of 2 .. 15 blocks and the +-1 symbols of short runs, so every scan uses them all the time.  Each id is another
    assignment: both groups are rotated by an amount of their own per id"""
    bits = [0] * 17
    for l in range(2, 9):
        bits[l] = 1
    bits[9], bits[16] = 240, 9
    rest = [s for s in range(256) if s not in LONG_AC]
    return bits, _rot(rest, 1 + 37 * t) + _rot(LONG_AC, 2 * t)


def foreign_dc_table(t: int):
    """DC table of id t: the symbols 0 .. 11, eleven codes of 2 .. 12 bits and one of 16, rotated by 3 t + 1"""
    bits = [0] * 17
    for l in range(2, 13):
        bits[l] = 1
    bits[16] = 1
    return bits, _rot(list(range(12)), 3 * t + 1)


def foreign_tables(dc_ids, ac_ids):
    """the `tables` knob for these ids: {("dc" | "ac", id): (bits, huffval)}"""
    out = {("dc", t): foreign_dc_table(t) for t in sorted(set(dc_ids))}
    out.update({("ac", t): foreign_ac_table(t) for t in sorted(set(ac_ids))})
    return out


def oversubscribed_table(index: int) -> bytes:
    """a raw DHT table definition with three codes of one bit: nothing may use it"""
    return bytes([index, 3] + [0] * 15 + [1, 2, 3])


# ---- the writer ------------------------------------------------------------------------------------------------------------

def _marker(code, payload=b""):
    return bytes([0xFF, code]) + struct.pack(">H", len(payload) + 2) + bytes(payload)


def _table_def(index, table) -> bytes:
    bits, vals = table
    n = sum(bits[1:17])
    return bytes([index]) + bytes(int(b) for b in bits[1:17]) + bytes(int(v) for v in vals[:n])


def _raw_tables(raw: bytes):
    """[(is_ac, id, (bits, huffval))] of raw table definitions"""
    out, p = [], 0
    while p < len(raw):
        bits = [0] + list(raw[p + 1:p + 17])
        cnt = sum(bits)
        out.append((raw[p] >> 4, raw[p] & 15, (bits, list(raw[p + 17:p + 17 + cnt]))))
        p += 17 + cnt
    return out


def _head(im, component_ids, sof1, progressive):
    """SOI .. SOF of jpeg_file.compose_parts, with the frame's component ids replaced and SOF0 made SOF1 on demand ->
    (the bytes, the component ids)"""
    n = len(im["coefs"])
    head = bytearray(jpeg_file.compose_parts(im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"],
                                             progressive=progressive)[0])
    pos = len(head) - (8 + 3 * n) - 2                                   # SOF is the last marker of the head
    assert head[pos] == 0xFF and head[pos + 1] in (0xC0, 0xC1, 0xC2)
    if sof1 and not progressive:
        head[pos + 1] = 0xC1
    ids = [head[pos + 10 + 3 * i] for i in range(n)]
    if component_ids is not None:
        ids = [int(c) for c in component_ids]
        assert len(ids) == n and len(set(ids)) == n
        for i, c in enumerate(ids):
            head[pos + 10 + 3 * i] = c
    return bytes(head), ids


def _code_intervals(intervals, pad_ones, fill_before_rst) -> bytes:
    """intervals: [[(code, size, bits, nbits)]] -> the entropy-coded segment: each interval padded to a byte with one or
    zero bits and stuffed, FF D0+n (behind fill_before_rst fill bytes) in front of every interval but the first"""
    out = bytearray()
    for k, items in enumerate(intervals):
        if k:
            out += b"\xff" * fill_before_rst + bytes([0xFF, 0xD0 + ((k - 1) & 7)])
        v, n = 0, 0
        for code, size, bits, nb in items:
            v = (v << (size + nb)) | (code << nb) | bits
            n += size + nb
        pad = -n % 8
        v = (v << pad) | (((1 << pad) - 1) if pad_ones else 0)
        out += stuff(v.to_bytes((n + pad) // 8, "big"))
    return bytes(out)


class _File:
    """the bytes written so far and what a parser must find in them"""

    def __init__(self, im, component_ids, sof1, progressive, dc_ids, ac_ids, tables, extra_dht):
        self.out = bytearray()
        head, self.ids = _head(im, component_ids, sof1, progressive)
        self.out += head
        n = len(im["coefs"])
        default = jpeg_file.table_assignment(im["colorspace"], n)
        self.dc_ids = [int(t) for t in (default if dc_ids is None else dc_ids)]
        self.ac_ids = [int(t) for t in (default if ac_ids is None else ac_ids)]
        assert len(self.dc_ids) == len(self.ac_ids) == n and all(0 <= t <= 3 for t in self.dc_ids + self.ac_ids)
        self.dc, self.ac, self.fixed = {}, {}, None
        self.dri, self.scans = 0, []
        if tables is not None:
            self.fixed = {k: (list(b), list(v)) for k, (b, v) in tables.items()}
            body = b"".join(_table_def((kind == "ac") << 4 | t, tab) for (kind, t), tab in self.fixed.items())
            for (kind, t), tab in self.fixed.items():
                (self.ac if kind == "ac" else self.dc)[t] = tab
            for is_ac, t, tab in _raw_tables(extra_dht):
                (self.ac if is_ac else self.dc)[t] = tab
            self.out += _marker(0xC4, body + bytes(extra_dht))
        else:
            assert not extra_dht, "extra_dht goes into the one DHT segment of fixed tables"

    def scan_tables(self, kind, used, hist):
        """the code tables {id: {symbol: (code, size)}} of a scan; without fixed tables libjpeg's: the optimal table of
        each id the scan uses, written in front of it, each once, in the order of first use"""
        cur = self.ac if kind == "ac" else self.dc
        if self.fixed is None:
            for t in dict.fromkeys(used):
                cur[t] = libjpeg_optimal(hist.get(t, np.zeros(256, np.int64)))
                self.out += _marker(0xC4, _table_def((kind == "ac") << 4 | t, cur[t]))
        return {t: derive(cur[t]) for t in set(used)}

    def restart(self, ri, repeat):
        if ri != self.dri or repeat:
            self.out += _marker(0xDD, struct.pack(">H", ri))
            self.dri = ri

    def sos(self, comps, selectors, ss, se, ah, al, dc_tbl, ac_tbl):
        self.out += _marker(0xDA, bytes([len(comps)]) + b"".join(bytes([self.ids[c], s]) for c, s in zip(comps, selectors))
                            + bytes([ss, se, (ah << 4) | al]))
        self.scans.append(dict(comps=list(comps), ss=ss, se=se, ah=ah, al=al, dc_tbl=list(dc_tbl), ac_tbl=list(ac_tbl),
                               dc=dict(self.dc), ac=dict(self.ac), restart_interval=self.dri, offset=len(self.out)))

    def segment(self, seg, behind):
        self.out += seg
        self.scans[-1]["length"] = len(seg)
        self.out += behind

    def close(self, im, fill_before_eoi, tail):
        self.out += b"\xff" * fill_before_eoi + b"\xff\xd9" + bytes(tail)
        return dict(data=bytes(self.out), scans=self.scans, component_ids=self.ids, dc_ids=self.dc_ids, ac_ids=self.ac_ids,
                    quants=[np.ones(64, np.uint16) if q is None else np.asarray(q, np.uint16) for q in im["quants"]])


def write_baseline(im, *, tables=None, dc_ids=None, ac_ids=None, component_ids=None, restart=0, repeat_dri=False,
                   pad_ones=True, between_scans=b"", fill_before_eoi=0, fill_before_rst=0, extra_dht=b"", sof1=False,
                   tail=b"") -> dict:
    """A whole sequential file (SOF0; SOF1 with sof1 or a quantiser above 255) of the image dict's arrays: one scan over
    all components.  -> dict(data, scans: [what jpeg_file.parse_progressive tells of a scan: here the one], component_ids,
    dc_ids, ac_ids, quants).

    tables: {("dc" | "ac", id): (bits, huffval)} written in one DHT segment behind the frame header; None: libjpeg's
    optimize_coding -- one DHT marker per table, optimal for this scan.  dc_ids / ac_ids: Td / Ta per component (default:
    jpeg_set_colorspace's).  restart: the interval in MCUs (DRI is written when it is not 0, or with repeat_dri).
    pad_ones: the bits that fill the last byte of an interval.  between_scans: bytes behind the scan, in front of EOI.
    fill_before_eoi / fill_before_rst: how many FF fill bytes precede EOI / every RSTn.  extra_dht: raw table
    definitions appended to the DHT segment of `tables`.  tail: bytes behind EOI."""
    f = _File(im, component_ids, sof1, False, dc_ids, ac_ids, tables, extra_dht)
    n = len(im["coefs"])
    intervals = interval_symbols(im, list(range(n)), int(restart))     # the table field carries the component
    hist = {"dc": {}, "ac": {}}
    for syms in intervals:
        for is_ac, c, sym, _b, _nb in syms:
            t = (f.ac_ids if is_ac else f.dc_ids)[c]
            hist["ac" if is_ac else "dc"].setdefault(t, np.zeros(256, np.int64))[sym] += 1
    if f.fixed is None:                                                  # jcmarker.c: per component its DC, then its AC table
        dcc, acc = {}, {}
        for c in range(n):
            if f.dc_ids[c] not in dcc:
                dcc.update(f.scan_tables("dc", [f.dc_ids[c]], hist["dc"]))
            if f.ac_ids[c] not in acc:
                acc.update(f.scan_tables("ac", [f.ac_ids[c]], hist["ac"]))
    else:
        dcc, acc = f.scan_tables("dc", f.dc_ids, None), f.scan_tables("ac", f.ac_ids, None)
    f.restart(int(restart), repeat_dri)
    f.sos(range(n), [(f.dc_ids[c] << 4) | f.ac_ids[c] for c in range(n)], 0, 63, 0, 0, f.dc_ids, f.ac_ids)
    coded = [[((acc[f.ac_ids[c]] if is_ac else dcc[f.dc_ids[c]])[sym]) + (bits, nb) for is_ac, c, sym, bits, nb in syms]
             for syms in intervals]
    f.segment(_code_intervals(coded, pad_ones, fill_before_rst), between_scans)
    return f.close(im, fill_before_eoi, tail)


def write_progressive(im, script, *, tables=None, dc_ids=None, ac_ids=None, component_ids=None, restart=0,
                      repeat_dri=False, pad_ones=True, between_scans=b"", fill_before_eoi=0, fill_before_rst=0,
                      extra_dht=b"", tail=b"") -> dict:
    """A whole progressive file (SOF2) of the image dict's arrays with the scans of `script` ((comps, Ss, Se, Ah, Al)), in
    the script's order whether libjpeg's validate_script would take it or not.  The knobs and the result are
    write_baseline's, with these differences: tables None is libjpeg's behaviour -- optimal tables in front of every
    scan that uses one; restart may be a list, cycled over the scans (DRI is written whenever the value changes, also
    back to 0; with repeat_dri in front of every scan); between_scans follows every scan; fill_before_rst may be
    {scan index: count}.  A scan names what libjpeg names: Td in a first DC scan, Ta in an AC scan, nothing in a DC
    refinement."""
    f = _File(im, component_ids, False, True, dc_ids, ac_ids, tables, extra_dht)
    cycle = list(restart) if isinstance(restart, (list, tuple)) else [restart]
    for i, scan in enumerate(script):
        comps, ss, se, ah, al = scan
        ri = int(cycle[i % len(cycle)])
        intervals = scan_symbols_refine(im, scan, ri) if ah else scan_symbols_prog(im, scan, ri)
        kind = "ac" if ss else "dc"
        ids = [(f.ac_ids if ss else f.dc_ids)[c] for c in comps]
        codes = {}
        if ss or not ah:                                                # a DC refinement codes nothing
            hist = {}
            for syms in intervals:
                for _is_ac, sym, _b, _nb, k in syms:
                    if sym is not None:
                        hist.setdefault(ids[k], np.zeros(256, np.int64))[sym] += 1
            codes = f.scan_tables(kind, ids, hist)
        f.restart(ri, repeat_dri)
        f.sos(comps, [t if ss else 0 if ah else t << 4 for t in ids], ss, se, ah, al,
              [0 if ss or ah else t for t in ids], [t if ss else 0 for t in ids])
        coded = [[(codes[ids[k]][sym] if sym is not None else (0, 0)) + (bits, nb) for _is_ac, sym, bits, nb, k in syms]
                 for syms in intervals]
        fill = fill_before_rst.get(i, 0) if isinstance(fill_before_rst, dict) else fill_before_rst
        f.segment(_code_intervals(coded, pad_ones, fill), between_scans)
    return f.close(im, fill_before_eoi, tail)


# ---- the corpus --------------------------------------------------------------------------------------------------------------

SIZE, BIG = (33, 18), (141, 93)
COM = _marker(0xFE, b"a comment \xff\xda\xff\xd9 \xff\xd0")         # a COM segment whose text holds marker bytes
QUAD = ([2, 1, 1, 2], [2, 1, 1, 2])                                     # 10 blocks in the MCU: the readers' limit
# layouts the reader grids leave out: (hsamp, vsamp, colorspace)
OMITTED = [([1, 1, 1], [1, 1, 1], 2), ([2, 1, 1], [2, 1, 1], 2), (*QUAD, 4), (*QUAD, 5), ([1, 2, 2], [1, 1, 1], 3),
           ([3, 1, 1], [1, 1, 1], 3), ([2, 2, 1], [2, 1, 2], 3), ([1, 1, 1], [4, 1, 1], 3), ([4, 2, 1], [1, 1, 1], 3),
           ([2, 1, 2], [2, 2, 1], 3), ([3], [3], 1)]

Y_SPANS_TWO = [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 5, 0, 1), ((0,), 6, 63, 0, 1), ((0,), 1, 63, 1, 0), ((1,), 1, 63, 0, 0),
               ((2,), 1, 63, 0, 0)]
Y_SPLIT_IN_TWO = [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 9, 1, 0), ((0,), 10, 63, 1, 0), ((1,), 1, 63, 0, 0),
                  ((2,), 1, 63, 0, 0)]
INCOMPLETE = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 0), ((2,), 3, 3, 0, 0)]
AC_BEFORE_DC = [((0,), 1, 63, 0, 0), ((0, 1, 2), 0, 0, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)]


def _image(seed, size=SIZE, hs=(2, 1, 1), vs=(2, 1, 1), cs=3, **kw):
    return synth_scan_image(np.random.default_rng(seed), size, list(hs), list(vs), cs, **kw)


def _spec(name, kind, f, fixed, script=None, **more):
    return dict(name=name, kind=kind, data=f["data"], written=f, fixed=fixed, script=script, **more)


def foreign_cases(enc_prog, enc_rst) -> dict:
    """-> dict(prog, base, refused): lists of dict(name, kind ("prog" | "base"), data, written (the writer's record), fixed
    (the tables are the foreign families), script); a refused case also holds intact (the same file without what makes it
    refused, where there is one) and match (what the parser's ValueError says).  enc_prog / enc_rst: LibJpeg9EncProg and
    LibJpeg9EncRst, for the files of the layouts the reader grids leave out"""
    simple = jpeg_file.simple_progression
    prog, base, refused = [], [], []

    def p(name, im, script, fixed=True, **kw):
        if fixed and "tables" not in kw:
            n = len(im["coefs"])
            default = jpeg_file.table_assignment(im["colorspace"], n)
            kw["tables"] = foreign_tables(kw.get("dc_ids", default), kw.get("ac_ids", default))
        prog.append(_spec(name, "prog", write_progressive(im, script, **kw), fixed, script))

    def b(name, im, fixed=True, **kw):
        if fixed and "tables" not in kw:
            n = len(im["coefs"])
            default = jpeg_file.table_assignment(im["colorspace"], n)
            kw["tables"] = foreign_tables(kw.get("dc_ids", default), kw.get("ac_ids", default))
        base.append(_spec(name, "base", write_baseline(im, **kw), fixed))

    ycc = _image(1)
    s3 = simple(3, 3)
    p("simple progression, fixed tables 0/1 in one DHT", ycc, s3)
    p("simple progression, Td (3,2,1) Ta (1,2,3)", ycc, s3, dc_ids=(3, 2, 1), ac_ids=(1, 2, 3))
    for sname, script in refine_scripts(3, 3, simple).items():
        p(f"script '{sname}', Td (2,0,3) Ta (3,1,0), Ri 1", _image(2), script, dc_ids=(2, 0, 3), ac_ids=(3, 1, 0), restart=1)
    gray = _image(3, (24, 16), [1], [1], 1)
    p("gray refine, ids 2/3, no DRI, zero pad bits", gray, GRAY_REFINE, dc_ids=(2,), ac_ids=(3,), pad_ones=False)
    p("zero pad bits, Ri 2", _image(4), s3, pad_ones=False, restart=2)
    p("zero pad bits, no DRI", _image(4), s3, pad_ones=False)
    p("DRI cycling 2, 0, 5, 1, 0 over the scans", _image(5), s3, restart=[2, 0, 5, 1, 0])
    p("DRI repeated in front of every scan", _image(5), s3, restart=2, repeat_dri=True)
    quad = _image(6, SIZE, *QUAD, 5)
    q5 = simple(4, 5)
    p("2x2,1x1,1x1,2x2 YCCK, Td (0,1,2,3) Ta (3,2,1,0), Ri 1", quad, q5, dc_ids=(0, 1, 2, 3), ac_ids=(3, 2, 1, 0), restart=1)
    p("2x2,1x1,1x1,2x2 YCCK, Td (2,3,0,1) Ta (0,0,3,3), no DRI", quad, q5, dc_ids=(2, 3, 0, 1), ac_ids=(0, 0, 3, 3))
    p("an over-subscribed AC table 3 nothing uses", _image(7), s3, extra_dht=oversubscribed_table(0x13), restart=3)
    p("a COM segment behind every scan", _image(8), s3, between_scans=COM, restart=2)
    p("FF FF in front of the marker behind every scan", _image(8), s3, between_scans=b"\xff\xff")
    p("FF in front of EOI", _image(8), s3, fill_before_eoi=1, restart=1)
    p("three bytes of garbage behind EOI", _image(8), s3, tail=b"\x00\xff\xda")
    p("a refinement that spans two first-scan bands", _image(9), Y_SPANS_TWO, restart=1)
    p("a first-scan band refined in two", _image(9), Y_SPLIT_IN_TWO, restart=2)
    p("an incomplete script", _image(10), INCOMPLETE)
    wide = _image(11)
    wide["quants"][1] = np.full(64, 40000, np.uint16)
    p("a quantiser of 40000: a 16-bit DQT", wide, s3, restart=2)
    p("component ids (0,1,2)", _image(12), s3, component_ids=(0, 1, 2))
    p("component ids (200,7,90)", _image(12), s3, component_ids=(200, 7, 90), dc_ids=(1, 3, 0), ac_ids=(2, 0, 1), restart=1)
    p("gray 141x93, Ri 1, fixed tables: 216 intervals", _image(13, BIG, [1], [1], 1), simple(1, 1), dc_ids=(1,), ac_ids=(2,),
      restart=1)
    for li, (hs, vs, cs) in enumerate(OMITTED):
        for size in (SIZE, (65, 66)):
            im = _image(100 + li, size, hs, vs, cs)
            script = simple(len(hs), cs)
            f = enc_prog.write(im, script, li % 3, 0)
            prog.append(_spec(f"libjpeg's file of {hs}x{vs} colour space {cs} at {size}, Ri {li % 3}", "prog",
                              dict(data=f, scans=None), False, script))

    for sof1 in (False, True):
        b(f"SOF{int(sof1)} 4:2:0, Td (2,3,0) Ta (3,1,2)", _image(20), dc_ids=(2, 3, 0), ac_ids=(3, 1, 2), sof1=sof1)
    for ri in (0, 2):
        tag = f"141x93, Ri {ri}: "
        b(tag + "4:2:0 with three table pairs", _image(21, BIG), dc_ids=(0, 1, 2), ac_ids=(0, 1, 2), restart=ri)
        b(tag + "2x2,1x1,1x1,2x2 with four table pairs", _image(22, BIG, *QUAD, 5), dc_ids=(0, 1, 2, 3), ac_ids=(0, 1, 2, 3),
          restart=ri)
        b(tag + "4:4:4 with Td (3,3,1) Ta (0,2,2)", _image(23, BIG, [1, 1, 1], [1, 1, 1]), dc_ids=(3, 3, 1), ac_ids=(0, 2, 2),
          restart=ri)
        b(tag + "gray with Td 3 Ta 2", _image(24, BIG, [1], [1], 1), dc_ids=(3,), ac_ids=(2,), restart=ri)
    # the same frame and tables on other seeded arrays: the split route's host build needs 15 and 17 of its 17 rounds here
    # (tests/test_foreign_files_host.py measures them), and reports 4 for the file of seed 22 above
    for seed in (300, 301):
        b(f"141x93, Ri 0: 2x2,1x1,1x1,2x2 with four table pairs, seed {seed}", _image(seed, BIG, *QUAD, 5), dc_ids=(0, 1, 2, 3),
          ac_ids=(0, 1, 2, 3))
    b("zero pad bits, Ri 1", _image(25), pad_ones=False, restart=1)
    b("zero pad bits, no DRI", _image(25), pad_ones=False)
    b("FF in front of EOI", _image(26), fill_before_eoi=1, restart=2)
    b("garbage behind EOI", _image(26), tail=b"\x00\xff\xda", restart=2)
    for li, (hs, vs, cs) in enumerate(OMITTED):
        for size in (SIZE, (65, 66)):
            im = _image(200 + li, size, hs, vs, cs)
            f = enc_rst.write(im, 2, 0, bool(li % 2))
            base.append(_spec(f"libjpeg's file of {hs}x{vs} colour space {cs} at {size}, Ri 2", "base", dict(data=f, scans=None),
                              False))

    # the stated limits
    im = _image(30)
    kw = dict(tables=foreign_tables((0, 1, 1), (0, 1, 1)), restart=1)
    for nfill in (1, 2):
        refused.append(_spec(f"{nfill} fill byte(s) in front of every RSTn, baseline", "base",
                             write_baseline(im, fill_before_rst=nfill, **kw), True, intact=write_baseline(im, **kw),
                             match="fill bytes inside a scan"))
    last = len(s3) - 1
    refused.append(_spec("a fill byte in front of the RSTn of the last scan", "prog",
                         write_progressive(im, s3, fill_before_rst={last: 1}, **kw), True, s3,
                         intact=write_progressive(im, s3, **kw), match="fill bytes inside a scan"))
    refused.append(_spec("an AC scan of component 0 in front of its DC scan", "prog",
                         write_progressive(im, AC_BEFORE_DC, **kw), True, AC_BEFORE_DC, intact=None,
                         match="scan 0: an AC scan before the component's DC scan"))
    return dict(prog=prog, base=base, refused=refused)


def read_case(lj, spec, k):
    """the case the host builds and the GPU batches take: the file's parsed markers, libjpeg 9's read of it -- asserted
    clean -- in arrays of read_oracle.padded_shapes (every third case larger than libjpeg's geometry)"""
    data = spec["data"]
    ref, clean = lj.read_bytes(data)
    assert ref is not None and clean, f"{spec['name']}: libjpeg 9 warns on the file or refuses it"
    if spec["kind"] == "prog":
        header = jpeg_file.parse_progressive(data)
        shapes = padded_shapes(header, k)
        return dict(spec, header=header, shapes=shapes, ref=ref, want=expected_arrays_prog(ref, shapes, header["script"]))
    header = jpeg_file.parse(data)
    shapes = padded_shapes(header, k)
    return dict(spec, header=header, scan=data[header["scan_offset"]:], shapes=shapes, ref=ref, want=expected_arrays(ref, shapes))


def read_cases(lj, specs, first=0):
    return [read_case(lj, s, first + k) for k, s in enumerate(specs)]


def refused_case(lj, spec):
    """a refused file with the header of its intact twin: what a reader prepared on the intact file is given"""
    intact = spec["intact"]["data"]
    ref, clean = lj.read_bytes(spec["data"])
    assert ref is not None and clean, f"{spec['name']}: libjpeg 9 warns on the file or refuses it"
    if spec["kind"] == "prog":
        header = jpeg_file.parse_progressive(intact)
        return dict(spec, header=header, shapes=padded_shapes(header, 0))
    header = jpeg_file.parse(intact)
    return dict(spec, header=header, scan=spec["data"][header["scan_offset"]:], shapes=padded_shapes(header, 0))
