"""The markers of a baseline JPEG file around one entropy-coded segment, as libjpeg 9 writes them for a fresh compress
object after jpeg_write_coefficients (jcmarker.c): SOI, JFIF APP0 or Adobe APP14, one DQT per component, SOF0 (SOF1
when a quantiser exceeds 8 bits), one DHT per table the scan uses, DRI when the scan has a restart interval, SOS, the
segment, EOI.  Host only, no device.

parse() is compose()'s inverse: the markers in front of one sequential Huffman scan, for the device scan reader
(qs_hip_read_device_batch).

Conventions of the library's encoder (include/jpegqs_hip.h): component ci uses quant table ci and the Huffman tables
jpeg_set_colorspace assigns.  Extra markers of a source file (jcopy_markers) are not written."""
from __future__ import annotations

import struct

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                   61, 54, 47, 55, 62, 63])

# jpeg_set_colorspace: (component ids, Huffman table per component, JFIF header, Adobe transform or None)
COLORSPACES = {
    1: ((1,), (0,), True, None),
    2: ((0x52, 0x47, 0x42), (0, 0, 0), False, 0),
    3: ((1, 2, 3), (0, 1, 1), True, None),
    4: ((0x43, 0x4D, 0x59, 0x4B), (0, 0, 0, 0), False, 0),
    5: ((1, 2, 3, 4), (0, 1, 1, 0), False, 2),
}


def table_assignment(colorspace: int, ncomp: int):
    """the Huffman table (0 / 1) of each component"""
    if colorspace not in COLORSPACES or len(COLORSPACES[colorspace][0]) != ncomp:
        raise ValueError(f"{ncomp} components in colour space {colorspace}: no JPEG file layout for it")
    return COLORSPACES[colorspace][1]


def _marker(code: int, payload: bytes) -> bytes:
    return bytes([0xFF, code]) + struct.pack(">H", len(payload) + 2) + payload


def _dht(index: int, table) -> bytes:
    bits, huffval = table
    bits = [int(b) for b in bits]
    n = sum(bits[1:17])
    return _marker(0xC4, bytes([index]) + bytes(bits[1:17]) + bytes(int(v) for v in huffval[:n]))


def compose_parts(quants, hsamp, vsamp, colorspace: int, image_size, dc_tables=None, ac_tables=None,
                  restart_interval: int = 0, progressive: bool = False):
    """-> (head, mid): the bytes of compose()'s file around its DHT markers and its segment.  head: SOI .. SOF, closed by
    the DHT markers when dc_tables / ac_tables are given; mid: DRI (when restart_interval is not 0) and the SOS header.
    head + [the DHT markers, where head has none] + mid + segment + FF D9 is compose()'s file: what the device's whole-file
    run (qs_hip_encode_device_batch_files) takes as a qs_hip_encode_frame.
    progressive: SOF2 in place of SOF0 / SOF1 and nothing else -- the head of a progressive file, whose scans are the
    progressive run's (qs_hip_encode_progressive_device_batch_files); mid is then of no use"""
    if not 0 <= int(restart_interval) <= 65535:
        raise ValueError(f"restart_interval {restart_interval}: 0 .. 65535")
    if (dc_tables is None) != (ac_tables is None):
        raise ValueError("compose_parts: dc_tables and ac_tables go together")
    n = len(quants)
    ids, tbl, jfif, adobe = COLORSPACES[colorspace][0], table_assignment(colorspace, n), *COLORSPACES[colorspace][2:]
    w, h = image_size
    out = [b"\xff\xd8"]
    if jfif:
        out.append(_marker(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])))
    if adobe is not None:
        out.append(_marker(0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, adobe)))
    wide = False
    for ci, q in enumerate(quants):
        q = np.ones(64, np.int64) if q is None else np.asarray(q, np.int64).reshape(64)
        prec = int(q.max() > 255)
        wide |= bool(prec)
        z = q[ZIGZAG]
        body = b"".join(struct.pack(">H", int(v)) for v in z) if prec else bytes(int(v) for v in z)
        out.append(_marker(0xDB, bytes([(prec << 4) | ci]) + body))
    sof = struct.pack(">BHHB", 8, h, w, n) + b"".join(bytes([ids[ci], (hsamp[ci] << 4) | vsamp[ci], ci]) for ci in range(n))
    out.append(_marker(0xC2 if progressive else 0xC1 if wide else 0xC0, sof))
    if dc_tables is not None:
        sent = set()
        for ci in range(n):
            for is_ac, tabs in ((0, dc_tables), (1, ac_tables)):
                if (is_ac, tbl[ci]) not in sent:
                    sent.add((is_ac, tbl[ci]))
                    out.append(_dht((is_ac << 4) | tbl[ci], tabs[tbl[ci]]))
    mid = []
    if restart_interval:
        mid.append(_marker(0xDD, struct.pack(">H", int(restart_interval))))
    sos = bytes([n]) + b"".join(bytes([ids[ci], (tbl[ci] << 4) | tbl[ci]]) for ci in range(n)) + bytes([0, 63, 0])
    mid.append(_marker(0xDA, sos))
    return b"".join(out), b"".join(mid)


def compose(segment: bytes, quants, hsamp, vsamp, colorspace: int, image_size, dc_tables, ac_tables,
            restart_interval: int = 0) -> bytes:
    """-> the whole file.  quants[ci]: 64 quantisers in natural order (None: all ones); dc_tables / ac_tables: the two
    (bits[17], huffval) pairs each; only the tables the components use are written.  restart_interval: the scan's
    interval in MCUs; libjpeg writes DRI behind the last DHT whenever it is not 0, also when it exceeds the MCU count"""
    head, mid = compose_parts(quants, hsamp, vsamp, colorspace, image_size, dc_tables, ac_tables, restart_interval)
    return head + mid + bytes(segment) + b"\xff\xd9"


# ---- scan scripts of progressive files (jpeg_scan_info: what cjpeg -scans reads) ------------------------------------------

def scan(comps, ss: int, se: int, ah: int = 0, al: int = 0):
    """one scan of a script: (component indices in frame order, Ss, Se, Ah, Al)"""
    return (tuple(int(c) for c in comps), int(ss), int(se), int(ah), int(al))


def spectral_script(ncomp: int):
    """the DC scan over all components, then per component the bands 1-5 and 6-63, Al = 0 throughout: libjpeg's
    jpeg_simple_progression without its successive-approximation steps"""
    out = [scan(range(ncomp), 0, 0)]
    for c in range(ncomp):
        out += [scan([c], 1, 5), scan([c], 6, 63)]
    return out


def simple_progression(ncomp: int, colorspace: int):
    """libjpeg 9's jpeg_simple_progression (jcparam.c), the script of cjpeg -progressive: for YCbCr (colorspace 3) with three
    components its ten scans, for every other frame the all-purpose script of 2 + 4 * ncomp scans.  Four respectively
    1 + 2 * ncomp of them are refinement scans (Ah > 0)"""
    allc = range(ncomp)                                                # (ncomp <= 4: one DC scan carries all components)
    if ncomp == 3 and colorspace == 3:
        return [scan(allc, 0, 0, 0, 1), scan([0], 1, 5, 0, 2), scan([2], 1, 63, 0, 1), scan([1], 1, 63, 0, 1),
                scan([0], 6, 63, 0, 2), scan([0], 1, 63, 2, 1), scan(allc, 0, 0, 1, 0), scan([2], 1, 63, 1, 0),
                scan([1], 1, 63, 1, 0), scan([0], 1, 63, 1, 0)]
    out = [scan(allc, 0, 0, 0, 1)]
    out += [scan([c], 1, 5, 0, 2) for c in allc] + [scan([c], 6, 63, 0, 2) for c in allc]
    out += [scan([c], 1, 63, 2, 1) for c in allc]
    out += [scan(allc, 0, 0, 1, 0)]
    out += [scan([c], 1, 63, 1, 0) for c in allc]
    return out


class ScriptError(ValueError):
    """a scan script libjpeg's validate_script refuses (or takes as sequential); .scan: where, or None"""

    def __init__(self, msg, scan_index=None):
        super().__init__(msg if scan_index is None else f"scan {scan_index}: {msg}")
        self.scan = scan_index


def validate_script(script, ncomp: int) -> bool:
    """validate_script of jcmaster.c (libjpeg 9) for a progressive script on a frame of ncomp components.  -> True when
    every scan has Ah = 0 (what the device writes), False when the script is valid but holds refinement scans; raises
    ScriptError for what libjpeg refuses and for a script it takes as sequential multi-scan (first scan 0 .. 63)"""
    script = list(script)
    if not script:
        raise ScriptError("no scans")
    if script[0][1] == 0 and script[0][2] == 63:                       # libjpeg validates it by its sequential rules
        sent = set()
        for i, (comps, ss, se, ah, al) in enumerate(script):
            if not 1 <= len(comps) <= 4 or any(not 0 <= c < ncomp for c in comps) \
                    or any(b <= a for a, b in zip(comps, comps[1:])):
                raise ScriptError("1 .. 4 components of the frame, in frame order", i)
            if (ss, se, ah, al) != (0, 63, 0, 0) or sent & set(comps):
                raise ScriptError("a scan of a sequential script that is not 0 .. 63 with Ah = Al = 0, or a component "
                                  "sent twice", i)
            sent |= set(comps)
        if len(sent) != ncomp:
            raise ScriptError("a component the sequential script does not send")
        raise ScriptError("a sequential multi-scan script, not a progressive one", 0)
    last = [[-1] * 64 for _ in range(ncomp)]
    spectral = True
    for i, (comps, ss, se, ah, al) in enumerate(script):
        if not 1 <= len(comps) <= 4:
            raise ScriptError("1 .. 4 components in a scan", i)
        for k, c in enumerate(comps):
            if not 0 <= c < ncomp:
                raise ScriptError("a component index out of range", i)
            if k and c <= comps[k - 1]:
                raise ScriptError("components out of frame order", i)
        if not (0 <= ss <= se <= 63 and 0 <= ah <= 10 and 0 <= al <= 10):
            raise ScriptError("Ss <= Se within 0 .. 63 and Ah, Al within 0 .. 10", i)
        if ss == 0 and se != 0:
            raise ScriptError("DC and AC coefficients in one scan", i)
        if ss != 0 and len(comps) != 1:
            raise ScriptError("an AC scan carries one component", i)
        for c in comps:
            if ss != 0 and last[c][0] < 0:
                raise ScriptError("an AC scan before the component's DC scan", i)
            for k in range(ss, se + 1):
                if last[c][k] < 0:
                    if ah != 0:
                        raise ScriptError("a first scan of a coefficient with Ah > 0", i)
                elif ah != last[c][k] or al != ah - 1:
                    raise ScriptError("a coefficient sent again without Ah = the last Al and Al = Ah - 1", i)
                last[c][k] = al
        spectral &= ah == 0
    for c in range(ncomp):
        if last[c][0] < 0:
            raise ScriptError(f"component {c} has no DC scan")
    return spectral


# ---- the inverse: the markers of a file in front of its one scan ----------------------------------------------------------

_SOF_NAMES = {0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential sequential (SOF5)",
              0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)",
              0xC9: "arithmetic coding (SOF9)", 0xCA: "arithmetic coding (SOF10)", 0xCB: "arithmetic coding (SOF11)",
              0xCD: "arithmetic coding (SOF13)", 0xCE: "arithmetic coding (SOF14)", 0xCF: "arithmetic coding (SOF15)"}
_MARKER_NAMES = {0xC4: "DHT", 0xDB: "DQT", 0xDA: "SOS (a second scan)", 0xDC: "DNL", 0xDD: "DRI", 0xCC: "DAC"}


def _colorspace(ids, jfif, adobe):
    """jdapimin.c default_decompress_parms of libjpeg 9: component ids first, then JFIF, then Adobe's transform"""
    n = len(ids)
    if n == 1:
        return 1
    if n == 3:
        known = {(0x01, 0x02, 0x03): 3, (0x01, 0x22, 0x23): 7, (0x52, 0x47, 0x42): 2, (0x72, 0x67, 0x62): 6}
        if tuple(ids) in known:
            return known[tuple(ids)]
        if jfif:
            return 3
        if adobe is not None:
            return 2 if adobe == 0 else 3
        return 3
    if n == 4:
        if adobe is not None:
            return 4 if adobe == 0 else 5
        return 4
    return 0


def parse(data, header_only: bool = False) -> dict:
    """The markers of a JPEG file up to its scan -> dict(image_size, colorspace, hsamp, vsamp, quants (natural order, one
    per component by its Tq), dc / ac ({DHT id: (bits[17], huffval)}), dc_tbl / ac_tbl (Td / Ta of each component),
    restart_interval (DRI, 0 if absent), scan_offset (the first byte behind the SOS header), sof (0xC0 / 0xC1),
    component_ids).  Looks at markers only, never at the entropy-coded bytes.

    Accepted: SOF0 or SOF1, 8 bits, Huffman, exactly one scan that carries all components of the frame in frame order
    with Ss = 0, Se = 63, Ah = Al = 0.  Everything else raises ValueError naming what it met: SOF2 and up, arithmetic
    coding, 12 bits, more than one scan, a DHT or DQT between scans, a DNL, fill bytes in front of an RSTn (T.81 B.1.1.2
    allows them; the device readers do not skip them).  Fill bytes in front of the EOI behind the scan are skipped, as
    the readers skip them.  header_only: `data` may end anywhere behind the SOS header (what follows the scan is then not
    looked at)."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("parse: no SOI at the start")
    pos, qt, dc, ac, dri, frame, jfif, adobe = 2, {}, {}, {}, 0, None, False, None
    while True:
        while pos < len(data) and data[pos] == 0xFF and pos + 1 < len(data) and data[pos + 1] == 0xFF:
            pos += 1                                                   # fill bytes
        if pos + 4 > len(data):
            raise ValueError("parse: the data ends in front of SOS")
        if data[pos] != 0xFF:
            raise ValueError(f"parse: marker expected at byte {pos}")
        code = data[pos + 1]
        if code == 0xD9:
            raise ValueError("parse: EOI in front of any scan")
        if code == 0x01 or 0xD0 <= code <= 0xD7:
            pos += 2
            continue
        n = struct.unpack_from(">H", data, pos + 2)[0]
        if n < 2 or pos + 2 + n > len(data):
            raise ValueError(f"parse: marker FF{code:02X} at byte {pos} runs past the data")
        body = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if code in _SOF_NAMES:
            raise ValueError(f"parse: {_SOF_NAMES[code]}: only baseline and extended sequential Huffman (SOF0, SOF1)")
        if code == 0xCC:
            raise ValueError("parse: arithmetic coding (DAC)")
        if code == 0xDC:
            raise ValueError("parse: DNL")
        if code in (0xC0, 0xC1):
            if frame is not None:
                raise ValueError("parse: a second SOF")
            prec, h, w, nc = struct.unpack_from(">BHHB", body, 0)
            if prec != 8:
                raise ValueError(f"parse: {prec}-bit samples: only 8")
            if h == 0:
                raise ValueError("parse: height 0 (DNL)")
            if not 1 <= nc <= 4 or len(body) != 6 + 3 * nc:
                raise ValueError(f"parse: {nc} components in the frame")
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nc)]
            frame = dict(sof=code, image_size=(w, h), comps=comps)
        elif code == 0xDB:
            p = 0
            while p < len(body):
                prec, idx = body[p] >> 4, body[p] & 15
                if prec > 1 or idx > 3 or p + 1 + 64 * (prec + 1) > len(body):
                    raise ValueError("parse: bad DQT")
                vals = struct.unpack_from(">64H" if prec else "64B", body, p + 1)
                q = np.zeros(64, np.uint16)
                q[ZIGZAG] = vals
                qt[idx] = q
                p += 1 + 64 * (prec + 1)
        elif code == 0xC4:
            p = 0
            while p < len(body):
                if p + 17 > len(body):
                    raise ValueError("parse: bad DHT")
                idx = body[p]
                bits = [0] + list(body[p + 1:p + 17])
                cnt = sum(bits)
                if (idx & 0xEF) > 3 or cnt > 256 or p + 17 + cnt > len(body):
                    raise ValueError("parse: bad DHT")
                (ac if idx & 0x10 else dc)[idx & 15] = (bits, list(body[p + 17:p + 17 + cnt]))
                p += 17 + cnt
        elif code == 0xDD:
            dri = struct.unpack(">H", body)[0]
        elif code == 0xE0 and body[:5] == b"JFIF\0":
            jfif = True
        elif code == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif code == 0xDA:
            if frame is None:
                raise ValueError("parse: SOS in front of SOF")
            comps = frame["comps"]
            ns = body[0]
            if len(body) != 4 + 2 * ns:
                raise ValueError("parse: bad SOS")
            sel = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(ns)]
            if [c for c, _d, _a in sel] != [c[0] for c in comps]:
                raise ValueError(f"parse: the scan carries components {[c for c, _d, _a in sel]} of the frame's "
                                 f"{[c[0] for c in comps]}: more than one scan")
            ss, se, ahal = body[1 + 2 * ns:4 + 2 * ns]
            if (ss, se, ahal) != (0, 63, 0):
                raise ValueError(f"parse: Ss {ss} Se {se} Ah/Al {ahal:#04x}: not a sequential scan")
            break
    for _c, _h, _v, tq in comps:
        if tq not in qt:
            raise ValueError(f"parse: quantisation table {tq} is used but not defined")
    for _c, td, ta in sel:
        if td not in dc or ta not in ac:
            raise ValueError(f"parse: Huffman table DC {td} / AC {ta} is used but not defined")
    if not header_only:
        # behind the scan: the next marker that is not RSTn must be EOI (markers only: the bytes between are not decoded)
        end = pos
        while end + 1 < len(data) and not (data[end] == 0xFF and data[end + 1] != 0 and not 0xD0 <= data[end + 1] <= 0xD7):
            end = data.find(b"\xff", end + 1)
            if end < 0:
                end = len(data)
        while end + 2 < len(data) and data[end + 1] == 0xFF:
            end += 1                                                   # fill bytes in front of the marker behind the scan
        if end + 1 < len(data) and 0xD0 <= data[end + 1] <= 0xD7:
            raise ValueError(f"parse: fill bytes inside a scan (FF FF in front of RST{data[end + 1] - 0xD0} at byte {end + 1}) "
                             f"are not supported: the device readers take an RSTn marker as two bytes")
        if end + 1 < len(data) and data[end + 1] != 0xD9:
            code = data[end + 1]
            raise ValueError(f"parse: {_MARKER_NAMES.get(code, f'marker FF{code:02X}')} behind the first scan: more than "
                             f"one scan, or tables between scans")
    ids = [c[0] for c in comps]
    return dict(image_size=frame["image_size"], colorspace=_colorspace(ids, jfif, adobe), hsamp=[c[1] for c in comps],
                vsamp=[c[2] for c in comps], quants=[qt[c[3]].copy() for c in comps], dc=dc, ac=ac,
                dc_tbl=[d for _c, d, _a in sel], ac_tbl=[a for _c, _d, a in sel], restart_interval=int(dri),
                scan_offset=pos, sof=frame["sof"], component_ids=ids)


# ---- the markers of a progressive file, scan by scan ------------------------------------------------------------------------

def parse_progressive(data) -> dict:
    """The markers of a whole progressive Huffman file (SOF2, 8 bits) -> parse()'s frame fields (image_size, colorspace,
    hsamp, vsamp, quants, component_ids, sof = 0xC2) and
      scans   one dict per scan: comps (frame indices), ss, se, ah, al, dc_tbl / ac_tbl (Td / Ta per scan component),
              dc / ac (the DHT tables in effect at that SOS: DHT and DRI persist until redefined), restart_interval,
              offset (the first byte behind the SOS header), length (up to the next marker that is not RSTn)
      script  [(comps, ss, se, ah, al)]
    for the progressive route of the device scan reader (qs_hip_read_prog_device_batch).  Looks at markers only.

    Accepted: exactly the files whose script passes validate_script (with either return value).  Everything else raises
    ValueError naming what it met: SOF0 / SOF1 (parse()'s files), arithmetic, lossless and differential frames, 12 bits,
    a DQT behind the first SOS, DNL, a scan that names an undefined table (a DC refinement names none), a script
    validate_script refuses (with its scan index), no EOI behind the last scan, fill bytes in front of an RSTn (with the
    scan's index; fill bytes in front of any other marker are skipped)."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("parse_progressive: no SOI at the start")
    pos, qt, dc, ac, dri, frame, jfif, adobe, scans = 2, {}, {}, {}, 0, None, False, None, []
    while True:
        while pos + 1 < len(data) and data[pos] == 0xFF and data[pos + 1] == 0xFF:
            pos += 1                                                   # fill bytes
        if pos + 2 > len(data):
            raise ValueError("parse_progressive: the data ends without EOI" + (" behind the last scan" if scans else ""))
        if data[pos] != 0xFF:
            raise ValueError(f"parse_progressive: marker expected at byte {pos}")
        code = data[pos + 1]
        if code == 0xD9:
            if not scans:
                raise ValueError("parse_progressive: EOI in front of any scan")
            break
        if code == 0x01 or 0xD0 <= code <= 0xD7:
            pos += 2
            continue
        if pos + 4 > len(data):
            raise ValueError("parse_progressive: the data ends without EOI")
        n = struct.unpack_from(">H", data, pos + 2)[0]
        if n < 2 or pos + 2 + n > len(data):
            raise ValueError(f"parse_progressive: marker FF{code:02X} at byte {pos} runs past the data")
        body = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if code in (0xC0, 0xC1):
            raise ValueError(f"parse_progressive: a sequential frame (SOF{code - 0xC0}): parse() reads it")
        if code in _SOF_NAMES and code != 0xC2:
            raise ValueError(f"parse_progressive: {_SOF_NAMES[code]}: only progressive Huffman (SOF2)")
        if code == 0xCC:
            raise ValueError("parse_progressive: arithmetic coding (DAC)")
        if code == 0xDC:
            raise ValueError("parse_progressive: DNL")
        if code == 0xC2:
            if frame is not None:
                raise ValueError("parse_progressive: a second SOF")
            if len(body) < 6:
                raise ValueError("parse_progressive: bad SOF")
            prec, h, w, nc = struct.unpack_from(">BHHB", body, 0)
            if prec != 8:
                raise ValueError(f"parse_progressive: {prec}-bit samples: only 8")
            if h == 0:
                raise ValueError("parse_progressive: height 0 (DNL)")
            if not 1 <= nc <= 4 or len(body) != 6 + 3 * nc:
                raise ValueError(f"parse_progressive: {nc} components in the frame")
            frame = dict(image_size=(w, h), comps=[(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15,
                                                    body[8 + 3 * i]) for i in range(nc)])
        elif code == 0xDB:
            if scans:
                raise ValueError("parse_progressive: DQT behind the first SOS")
            p = 0
            while p < len(body):
                prec, idx = body[p] >> 4, body[p] & 15
                if prec > 1 or idx > 3 or p + 1 + 64 * (prec + 1) > len(body):
                    raise ValueError("parse_progressive: bad DQT")
                vals = struct.unpack_from(">64H" if prec else "64B", body, p + 1)
                q = np.zeros(64, np.uint16)
                q[ZIGZAG] = vals
                qt[idx] = q
                p += 1 + 64 * (prec + 1)
        elif code == 0xC4:
            p = 0
            while p < len(body):
                if p + 17 > len(body):
                    raise ValueError("parse_progressive: bad DHT")
                idx = body[p]
                bits = [0] + list(body[p + 1:p + 17])
                cnt = sum(bits)
                if (idx & 0xEF) > 3 or cnt > 256 or p + 17 + cnt > len(body):
                    raise ValueError("parse_progressive: bad DHT")
                (ac if idx & 0x10 else dc)[idx & 15] = (bits, list(body[p + 17:p + 17 + cnt]))
                p += 17 + cnt
        elif code == 0xDD:
            if len(body) != 2:
                raise ValueError("parse_progressive: bad DRI")
            dri = struct.unpack(">H", body)[0]
        elif code == 0xE0 and body[:5] == b"JFIF\0":
            jfif = True
        elif code == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif code == 0xDA:
            if frame is None:
                raise ValueError("parse_progressive: SOS in front of SOF")
            ids = [c[0] for c in frame["comps"]]
            ns = body[0] if body else 0
            if not 1 <= ns <= 4 or len(body) != 4 + 2 * ns:
                raise ValueError(f"parse_progressive: scan {len(scans)}: bad SOS")
            comps, td, ta = [], [], []
            for i in range(ns):
                cid = body[1 + 2 * i]
                if cid not in ids:
                    raise ValueError(f"parse_progressive: scan {len(scans)} names component id {cid}, not of the frame")
                comps.append(ids.index(cid))
                td.append(body[2 + 2 * i] >> 4)
                ta.append(body[2 + 2 * i] & 15)
            ss, se, ahal = body[1 + 2 * ns:4 + 2 * ns]
            ah, al = ahal >> 4, ahal & 15
            for i in range(ns):
                if ss == 0 and ah == 0 and td[i] not in dc:
                    raise ValueError(f"parse_progressive: scan {len(scans)}: Huffman table DC {td[i]} is used but not defined")
                if ss != 0 and ta[i] not in ac:
                    raise ValueError(f"parse_progressive: scan {len(scans)}: Huffman table AC {ta[i]} is used but not defined")
            # behind the header: up to the next marker that is not RSTn (markers only: the bytes between are not decoded)
            end = pos
            while end + 1 < len(data) and not (data[end] == 0xFF and data[end + 1] != 0 and not 0xD0 <= data[end + 1] <= 0xD7):
                end = data.find(b"\xff", end + 1)
                if end < 0:
                    end = len(data)
            if end + 1 >= len(data):
                raise ValueError(f"parse_progressive: the data ends inside scan {len(scans)}: no EOI behind the last scan")
            fill = end
            while fill + 2 < len(data) and data[fill + 1] == 0xFF:
                fill += 1                                              # fill bytes in front of the marker behind the scan
            if 0xD0 <= data[fill + 1] <= 0xD7:
                raise ValueError(f"parse_progressive: scan {len(scans)}: fill bytes inside a scan (FF FF in front of "
                                 f"RST{data[fill + 1] - 0xD0} at byte {fill + 1}) are not supported: the device readers "
                                 f"take an RSTn marker as two bytes")
            scans.append(dict(comps=comps, ss=ss, se=se, ah=ah, al=al, dc_tbl=td, ac_tbl=ta, dc=dict(dc), ac=dict(ac),
                              restart_interval=int(dri), offset=pos, length=end - pos))
            pos = end
    if frame is None:
        raise ValueError("parse_progressive: no frame header")
    comps = frame["comps"]
    for _c, _h, _v, tq in comps:
        if tq not in qt:
            raise ValueError(f"parse_progressive: quantisation table {tq} is used but not defined")
    script = [scan(s["comps"], s["ss"], s["se"], s["ah"], s["al"]) for s in scans]
    try:
        validate_script(script, len(comps))
    except ScriptError as e:
        raise ValueError(f"parse_progressive: {e}") from None
    ids = [c[0] for c in comps]
    return dict(image_size=frame["image_size"], colorspace=_colorspace(ids, jfif, adobe), hsamp=[c[1] for c in comps],
                vsamp=[c[2] for c in comps], quants=[qt[c[3]].copy() for c in comps], component_ids=ids, sof=0xC2,
                scans=scans, script=script)
