"""Seeded adversarial inputs of the plane-layer kernels (include/jpegqs_hip.h, "plane layer") and what the reference's
own block-level functions make of them.

Shared by tests/test_plane_cases.py (CPU: the oracle port against the reference on every case) and
tests/test_gpu_plane_kernels.py (GPU: every plane-layer call against the same expectations).  Both suites build the
same bytes from the same seeds, so the reference calls of the GPU suite are exactly those of the CPU suite and their
digests are recorded in tests/golden/reference_calls.json.gz (oracle.RecordedReference).

Every input is a state a job can reach: coefficients are dequantised values inside the interval of a multiple of their
quantiser that passes the range check (q * m in [-0x800, 0x7ff], reference quantsmooth.h:2598-2602), interval ends
included; the pixel plane pass B reads is the plane pass A writes for those coefficients.  One exception is a kernel
contract beyond the driver's reach: all-ones tables (the driver skips its iterations, :2500).  Tables with entries of
0x800 and more (the driver stops before its passes, :2501-2503) reach only the dequantisation and, on the CPU, the
oracle port's block function.

Numpy restatements of the reference's plane-driver steps cite the reference lines they restate.
"""
from __future__ import annotations

import numpy as np

QS_APRON_X = 16   # csrc/qs_device.h: pixel (x, y) of a product plane is at row_offset(y) + QS_APRON_X + x

# JPEG Annex K luminance table, natural order
STD_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.uint16)

F_DIAG, F_JOINT, F_LOWQ, F_NOREB = 1, 2, 8, 16


def table(name: str) -> np.ndarray:
    """uint16[64] quantisation tables beyond quality scaling"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "std":
        return STD_LUMA.copy()
    if name == "ones":          # every k takes the QS_REC_Q1 skip (the driver itself skips such a table, :2500)
        return np.ones(64, np.uint16)
    if name == "mixed":         # 1 next to large entries
        return np.where(rng.random(64) < 0.5, 1, rng.integers(200, 0x800, 64)).astype(np.uint16)
    if name == "zeros":         # zero entries count as 1 (:2505-2510)
        t = STD_LUMA.copy()
        t[rng.choice(64, 16, replace=False)] = 0
        t[0] = 0
        return t
    if name == "huge":          # 0x800..65535: interval() in its shift form, a 0 may walk to +-32767 (the driver stops, :2503)
        t = rng.integers(0x800, 0x10000, 64).astype(np.uint16)
        t[[0, 1, 8, 9, 27, 63]] = 65535
        t[[2, 16]] = 0x800
        return t
    if name == "max":           # large entries up to 0x7ff, the largest a job smooths with: interval() with shifts of 4..0
        t = rng.integers(0x400, 0x800, 64).astype(np.uint16)
        t[[0, 1, 8, 9, 27, 63]] = 0x7ff
        t[[2, 16, 40]] = 1
        return t
    if name == "camera":        # non-monotonic
        t = rng.integers(2, 40, 64).astype(np.uint16)
        t[rng.choice(64, 6, replace=False)] = 1
        return t
    raise KeyError(name)


def eff(q) -> np.ndarray:
    """the quantiser the recovery uses: 0 -> 1 (reference :2505-2510)"""
    q = np.asarray(q, dtype=np.int64)
    return np.where(q == 0, 1, q).astype(np.uint16)


def _multiples(qe):
    """the allowed multiples m of each quantiser: q * m in [-0x800, 0x7ff]"""
    qe = qe.astype(np.int64)
    return -(0x800 // qe), 0x7ff // qe


def _interval(a, qe):
    """the values that quantise to a (reference :1552-1557)"""
    qe = qe.astype(np.int64)
    d0, d1 = (qe - 1) >> 1, qe >> 1
    return a - np.where(a > 0, d1, d0), a + np.where(a < 0, d1, d0)


def _dct_matrix():
    n = np.arange(8)
    m = np.cos((2 * n[None, :] + 1) * n[:, None] * np.pi / 16) * np.sqrt(2 / 8)
    m[0] /= np.sqrt(2)
    return m


KINDS = ("random", "ends", "saturate", "checker", "single", "sparse", "flat")


def coefficients(rng, q, hblk, wblk, kinds) -> np.ndarray:
    """dequantised int16 [hblk, wblk, 64]; block kinds drawn from `kinds` (a per-block pattern)"""
    qe = eff(q).astype(np.int64)
    mlo, mhi = _multiples(qe)
    nb = hblk * wblk
    kind = rng.choice(len(kinds), nb)
    m = np.zeros((nb, 64), np.int64)
    pos = np.zeros((nb, 64), np.int64)   # 0: the multiple itself, 1: low end, 2: high end, 3: anywhere in the interval
    # random / sparse / flat: small multiples mostly, the extreme ones sometimes
    small = np.clip(np.rint(rng.normal(0, 3, (nb, 64))), mlo, mhi).astype(np.int64)
    extreme = np.where(rng.random((nb, 64)) < 0.5, mlo, mhi)
    pick = rng.random((nb, 64))
    rand = np.where(pick < 0.1, extreme, np.where(pick < 0.2, rng.integers(mlo, mhi + 1, (nb, 64)), small))
    cm = _dct_matrix()
    for b in range(nb):
        k = kinds[kind[b]]
        if k in ("random", "ends"):
            m[b] = rand[b]
            pos[b] = rng.integers(1, 3, 64) if k == "ends" else 3
        elif k == "saturate":
            m[b] = extreme[b]
            pos[b] = np.where(m[b] < 0, 1, 2)
        elif k == "checker":   # a 0/255 checkerboard (or stripes): every neighbour difference is large
            yy, xx = np.mgrid[0:8, 0:8]
            pat = [(xx + yy) & 1, xx & 1, yy & 1][b % 3] * 255.0 - 128.0
            f = (cm @ pat @ cm.T).ravel()
            m[b] = np.clip(np.rint(f / qe), mlo, mhi)
            pos[b] = rng.integers(0, 4, 64)
        elif k == "single":    # one coefficient, at each of the 64 positions in turn
            j = b % 64
            m[b, j] = extreme[b, j] if extreme[b, j] else mhi[j]
            pos[b, j] = rng.integers(0, 3)
        elif k == "sparse":
            keep = rng.random(64) < 0.1
            m[b] = np.where(keep, rand[b], 0)
            pos[b] = np.where(keep, 3, 0)
        elif k == "flat":
            m[b, 0] = rand[b, 0]
        else:
            raise KeyError(k)
    a = m * qe
    lo, hi = _interval(a, qe)
    anywhere = lo + np.floor(rng.random((nb, 64)) * (hi - lo + 1)).astype(np.int64)
    v = np.select([pos == 1, pos == 2, pos == 3], [lo, hi, anywhere], a)
    assert v.min() >= -32768 and v.max() <= 32767
    return v.astype(np.int16).reshape(hblk, wblk, 64)


# ---- cases ---------------------------------------------------------------------------------------------------------
# (name, table, hblk, wblk, kinds, seed); odd sizes, every kind next to every other
PASS_B_CASES = [
    ("std-mixed-kinds", "std", 7, 9, KINDS, 1),
    ("ones-random", "ones", 5, 6, ("random", "ends", "saturate"), 2),
    ("mixed-table", "mixed", 6, 7, KINDS, 3),
    ("zeros-table", "zeros", 5, 9, KINDS, 4),
    ("max-table", "max", 4, 5, ("random", "ends", "saturate", "sparse"), 5),
    ("camera-checker", "camera", 6, 6, ("checker", "saturate"), 6),
    ("std-single-64", "std", 8, 8, ("single",), 7),
    ("camera-sparse", "camera", 5, 7, ("sparse",), 8),
    ("std-flat", "std", 4, 9, ("flat",), 9),
]


# Tables with entries of 0x800 and more never reach pass B in a job (the driver stops, :2501-2503).  The oracle port
# follows the reference's block function there too (CPU suite only); the product's recovery kernels do not claim to.
UNREACHABLE_B_CASES = [("huge-table", "huge", 4, 5, ("random", "ends", "saturate", "sparse"), 5)]


def pass_b_case(name):
    for c in PASS_B_CASES + UNREACHABLE_B_CASES:
        if c[0] == name:
            _, t, hb, wb, kinds, seed = c
            q = table(t)
            return q, coefficients(np.random.default_rng(seed), q, hb, wb, kinds)
    raise KeyError(name)


def raw_int16_case(seed, hblk=6, wblk=7) -> np.ndarray:
    """pass A (first = 0) on coefficients covering the whole int16 range: the IDCT's __mul24 operands
    (csrc/qs_kernels.hip) must fit in 24 bits for every such input"""
    rng = np.random.default_rng(seed)
    c = rng.integers(-32768, 32768, (hblk, wblk, 64))
    c[0, 0], c[0, 1], c[1, 0] = 32767, -32768, 0
    c[1, 1] = np.where(np.arange(64) % 2, 32767, -32768)
    c[2, 2] = np.where(np.arange(64) % 2, -32768, 32767)
    c[2, 3] = 0; c[2, 3, 0] = -32768
    c[3, 3] = 0; c[3, 3, 63] = 32767
    return c.astype(np.int16)


# first = 1 (dequantise + range check): quantised coefficients whose products sit on either side of the stop
STATUS_CASES = [
    # (name, expect stop)
    ("edges-pass", False),     # products exactly 0x7ff and -0x800
    ("trip-high", True),       # one product 0x800
    ("trip-low", True),        # one product -0x801
    ("trip-wrap", True),       # a product that wraps in int16 to a small value
    ("zero-table-big", False), # a 0 quantiser leaves +-32767 untouched (0 * c == 0)
]


def status_case(name):
    """-> (raw quant, quantised int16 [hb, wb, 64]) for qs_hip_idct_plane(first = 1)"""
    q = STD_LUMA.copy()
    q[5], q[6], q[9] = 1, 0x7ff, 3
    rng = np.random.default_rng(11)
    qi = q.astype(np.int64)
    c = np.clip(rng.integers(-3, 4, (5, 6, 64)), -2048 // qi, 0x7ff // qi)
    c[:, :, 6] = np.clip(c[:, :, 6], -1, 1)
    c[1, 2, 5], c[3, 4, 5], c[0, 5, 6], c[4, 0, 6] = 0x7ff, -0x800, 1, -1
    if name == "trip-high":
        c[2, 3, 5] = 0x800
    elif name == "trip-low":
        c[4, 5, 5] = -0x801
    elif name == "trip-wrap":
        q[20] = 2
        c[1, 1, 20] = 16384 + 1            # 32770 -> wraps to -32766
    elif name == "zero-table-big":
        q[30] = 0
        c[0, 0, 30], c[1, 0, 30] = 32767, -32768
    return q, c.astype(np.int16)


def dequant_wrap(q, c) -> np.ndarray:
    """c * q in int, stored into int16 (wraps) -- reference :2597-2599, :2563"""
    return (c.astype(np.int64) * q.astype(np.int64)).astype(np.int16)


def stops(q, c) -> bool:
    """reference :2598-2602: any product outside [-0x800, 0x7ff]"""
    p = c.astype(np.int64) * q.astype(np.int64)
    return bool(((p < -0x800) | (p > 0x7ff)).any())


# ---- reference-built planes and expectations ------------------------------------------------------------------------
def pixels(ref, coefs) -> np.ndarray:
    """idct_islow of every block -> uint8 [hblk * 8, wblk * 8]"""
    hb, wb = coefs.shape[:2]
    px = ref.idct_blocks(coefs.reshape(-1, 64))
    return px.reshape(hb, wb, 8, 8).transpose(0, 2, 1, 3).reshape(hb * 8, wb * 8)


def apron(px) -> np.ndarray:
    """the clamp-to-edge apron of reference quantsmooth.h:2612-2619: columns -1 and w copy 0 and w - 1, then rows -1
    and h copy rows 0 and h - 1 (apron columns included) -> uint8 [h + 2, w + 2]"""
    h, w = px.shape
    p = np.empty((h + 2, w + 2), np.uint8)
    p[1:-1, 1:-1] = px
    p[1:-1, 0] = px[:, 0]
    p[1:-1, -1] = px[:, -1]
    p[0] = p[1]
    p[-1] = p[-2]
    return p


def ref_plane(ref, coefs) -> np.ndarray:
    """the plane pass A leaves for `coefs` (rows -1..h, columns -1..w)"""
    return apron(pixels(ref, coefs))


def all_positions(hb, wb):
    return [(bx, by) for by in range(hb) for bx in range(wb)]


def sample_positions(hb, wb, n, seed):
    """every edge and corner block plus n seeded interior ones"""
    rng = np.random.default_rng(seed)
    pos = {(bx, by) for bx in range(wb) for by in (0, hb - 1)} | {(bx, by) for by in range(hb) for bx in (0, wb - 1)}
    while len(pos) < 2 * (wb + hb) - 4 + n:
        pos.add((int(rng.integers(1, wb - 1)), int(rng.integers(1, hb - 1))))
    return sorted(pos, key=lambda p: (p[1], p[0]))


def rebalance_on(flags, luma):
    """reference :1567-1568"""
    return not (flags & F_NOREB) and (luma or not (flags & 32))


def c_roundf(x) -> np.ndarray:
    """C roundf: nearest, ties away from zero (numpy's round takes ties to even)"""
    x = np.asarray(x, dtype=np.float32)
    t = np.trunc(x)
    return np.where(np.abs(x - t) >= np.float32(0.5), t + np.sign(x), t).astype(np.float32)   # x - t is exact


def fdct_expected(ref, px_blocks) -> np.ndarray:
    """reference :2740-2749: fdct_float of (pixel - 128), then roundf into a JCOEF.  px_blocks: uint8 [n, 64]"""
    f = ref.fdct_blocks(px_blocks.astype(np.float32) - 128.0)
    return c_roundf(f).astype(np.int64).astype(np.int16)


def downsample_expected(luma_px, lw, lh, ws, hs) -> np.ndarray:
    """reference :2753-2815 restated: box mean (sum + n/2) / n over the luma pixels of each cell (cells cut at the luma
    plane's edge), then replicated out to the low-res plane's edge and apron -> uint8 [lh + 2, lw + 2] (rows / columns
    -1..lh / -1..lw).  luma_px: uint8 [yh, yw] without apron"""
    yh, yw = luma_px.shape
    w1, h1 = (yw + ws - 1) // ws, (yh + hs - 1) // hs
    out = np.zeros((lh + 2, lw + 2), np.uint8)
    for y in range(h1):
        for x in range(w1):
            cell = luma_px[y * hs:min(y * hs + hs, yh), x * ws:min(x * ws + ws, yw)].astype(np.int64)
            out[y + 1, x + 1] = (cell.sum() + cell.size // 2) // cell.size
    out[1:h1 + 1, 0] = out[1:h1 + 1, 1]
    out[1:h1 + 1, w1 + 1:] = out[1:h1 + 1, w1:w1 + 1]
    out[0] = out[1]
    out[h1 + 1:] = out[h1]
    return out


# chroma upsampling geometries: (image width, image height, ws, hs)
UPSAMPLE_CASES = [(w, h, ws, hs) for ws in (1, 2, 4) for hs in (1, 2)
                  for (w, h) in ((61, 45), (88, 72))] + [(203, 139, 2, 2), (37, 150, 4, 1)]


def upsample_geometry(w, h, ws, hs):
    """the blocks of a real job of this size: luma ceil(w / 8) x ceil(h / 8), chroma ceil(ceil(w / ws) / 8) ..."""
    w1, h1 = (w + ws - 1) // ws, (h + hs - 1) // hs
    ywb, yhb = (w + 7) // 8, (h + 7) // 8
    cwb, chb = (w1 + 7) // 8, (h1 + 7) // 8
    st = ((w1 + 8) & -8) * ws
    return dict(w1=w1, h1=h1, ywb=ywb, yhb=yhb, cwb=cwb, chb=chb, ww=ywb * 8, hh=yhb * 8, st=st,
                rows=((h1 + 8) & -8) * hs)


def upsample_inputs(ref, w, h, ws, hs, seed):
    """pass-A planes of a real job of this geometry: full-res luma, its low-res (downsampled) copy and the chroma
    plane, each with its apron; the luma rows get padding columns so the strips' reads past the row (they land in
    output columns beyond ww, which nothing reads) stay inside the array"""
    g = upsample_geometry(w, h, ws, hs)
    rng = np.random.default_rng(seed)
    yq, cq = table("std"), table("camera")
    ycoef = coefficients(rng, yq, g["yhb"], g["ywb"], ("random", "sparse", "flat", "checker"))
    ccoef = coefficients(rng, cq, g["chb"], g["cwb"], ("random", "sparse", "flat", "saturate"))
    ypx = pixels(ref, ycoef)
    luma = np.zeros((g["hh"] + 2, g["ww"] + 2 + 8 * ws + 8), np.uint8)
    luma[:, :g["ww"] + 2] = apron(ypx)
    lowres = downsample_expected(ypx, g["cwb"] * 8, g["chb"] * 8, ws, hs) if (ws, hs) != (1, 1) else apron(ypx)
    chroma = ref_plane(ref, ccoef)
    assert lowres.shape == chroma.shape
    return g, ycoef, ccoef, luma, lowres, chroma


def upsample_expected(ref, g, luma, lowres, chroma, ws, hs, first_rows=None):
    """the reference's upsampler (:2724-2730): upsample_row per 8-row strip, the bottom replicate of :2729-2730.
    first_rows = f (a band's view, qs_hip_upsample_rows): the right-edge replicate (:2390-2393) on the first f low-res
    rows only -- every strip computed without it (the strip seen as a later one), then the replicate restated here.
    -> uint8 [rows, st]; columns >= ww are not part of the contract"""
    w1, h1, ww, hh, st = g["w1"], g["h1"], g["ww"], g["hh"], g["st"]
    strips = [(y, min(y + 8, h1), 0 if first_rows is None else 8) for y in range(0, h1, 8)]
    mem = ref.upsample_strips(chroma, lowres, luma, w1, ww, g["rows"], st, ws, hs, strips)
    if first_rows is not None:
        mem[:first_rows * hs, w1 * ws:ww] = mem[:first_rows * hs, w1 * ws - 1:w1 * ws]
    mem[h1 * hs:hh] = mem[h1 * hs - 1]
    return mem


# ---- pass B expectations ----------------------------------------------------------------------------------------------
PASS_B_FLAGS = (0, F_DIAG, F_NOREB, F_DIAG | F_NOREB)


def pass_b_expected(ref, name, flags, luma):
    """block() of every block of the case, reading the reference-built plane"""
    q, c = pass_b_case(name)
    plane = ref_plane(ref, c)
    return ref.blocks(c, eff(q), plane, all_positions(*c.shape[:2]), flags, luma)


def joint_inputs(ref, name):
    """a chroma case and the luma plane its JOINT_YUV predictor reads (4:4:4: the luma plane itself, :2761): the pass-A
    plane of other coefficients of the same geometry"""
    q, c = pass_b_case(name)
    lq = table("std")
    lc = coefficients(np.random.default_rng(100 + len(name)), lq, c.shape[0], c.shape[1], ("random", "checker", "flat"))
    return q, c, ref_plane(ref, c), ref_plane(ref, lc)


def joint_expected(ref, name, flags):
    q, c, plane, plane2 = joint_inputs(ref, name)
    return ref.blocks(c, eff(q), plane, all_positions(*c.shape[:2]), flags | F_JOINT, 0, plane2)


def lowq_expected(ref, name, flags, luma, with_plane2):
    q, c, plane, plane2 = joint_inputs(ref, name)
    return ref.blocks(c, eff(q), plane, all_positions(*c.shape[:2]), flags | F_LOWQ, luma,
                      plane2 if with_plane2 else None)


# ---- large planes: every pass-B kernel form ---------------------------------------------------------------------------
# qs_dp_waves (csrc/qs_kernels.hip): <= 768 groups of 64 blocks -> 4 waves, <= 1536 -> 2 waves, more -> a block per lane
LARGE_CASES = [("dp2", 200, 256, 21), ("lane", 321, 320, 22)]   # (name, hblk, wblk, seed): 800 and 1606 groups


def large_case(name):
    for n, hb, wb, seed in LARGE_CASES:
        if n == name:
            rng = np.random.default_rng(seed)
            q = table("camera")
            # a tile of mixed adversarial blocks repeated over the plane, rolled per tile row so that neighbours vary
            tile = coefficients(rng, q, 16, 16, KINDS)
            reps = np.tile(tile, ((hb + 15) // 16, (wb + 15) // 16, 1))[:hb, :wb]
            shift = rng.integers(0, wb, hb)
            return q, np.stack([np.roll(reps[y], shift[y], axis=0) for y in range(hb)])
    raise KeyError(name)


def large_sample_expected(ref, oracle, name, flags):
    """the sampled blocks of a large case against the reference; the plane comes from the oracle's pass A (too many
    blocks for one call each), itself checked against the reference over the sampled blocks' 3x3 neighbourhoods"""
    q, c = large_case(name)
    hb, wb = c.shape[:2]
    plane = oracle_plane(oracle, q, c)
    pos = sample_positions(hb, wb, 24, hb + wb)
    return ref.blocks(c, eff(q), apron_view(plane, wb, hb), pos, flags, 1), pos


def pass_b_expected_plain(ref, q, c, flags, luma=1):
    """block() of every block of c on its reference-built plane -> int16 [hblk, wblk, 64]"""
    return ref.blocks(c, eff(q), ref_plane(ref, c), all_positions(*c.shape[:2]), flags, luma).reshape(c.shape)


def oracle_plane(oracle, q, c, first=0):
    """pass A of the oracle port in the product layout (oracle.qso_band_idct) -> (plane bytes, pitch)"""
    import ctypes as C
    hb, wb = c.shape[:2]
    pitch = ((wb * 8 + QS_APRON_X + 1) + 63) & ~63
    plane = np.zeros((hb * 8 + 2) * pitch, np.uint8)
    cc = np.ascontiguousarray(c).copy()
    bad = C.c_int(0)
    f = oracle.fn("band_idct", None)
    f(cc.ctypes.data_as(C.c_void_p), C.c_int(wb), C.c_int(hb), np.ascontiguousarray(q, np.uint16).ctypes.data_as(C.c_void_p),
      C.c_int(first), plane.ctypes.data_as(C.c_void_p), C.c_int(pitch), C.c_int(QS_APRON_X), C.c_int(1), C.c_int(1),
      C.byref(bad))
    return plane, pitch


def apron_view(plane_pitch, wb, hb) -> np.ndarray:
    """rows -1..h, columns -1..w of a product-layout plane -> uint8 [h + 2, w + 2]"""
    plane, pitch = plane_pitch
    return np.ascontiguousarray(plane.reshape(-1, pitch)[:hb * 8 + 2, QS_APRON_X - 1:QS_APRON_X + wb * 8 + 1])


def oracle_band_smooth(oracle, q, c, plane_pitch, flags, luma=1, final_clamp=0, row0=None, row1=None):
    import ctypes as C
    hb, wb = c.shape[:2]
    plane, pitch = plane_pitch
    cc = np.ascontiguousarray(c).copy()
    f = oracle.fn("band_smooth_rows", None)
    f(cc.ctypes.data_as(C.c_void_p), C.c_int(wb), C.c_int(hb), np.ascontiguousarray(q, np.uint16).ctypes.data_as(C.c_void_p),
      plane.ctypes.data_as(C.c_void_p), C.c_int(pitch), C.c_int(QS_APRON_X), C.c_int(flags), C.c_int(luma),
      C.c_int(final_clamp), C.c_int(0 if row0 is None else row0), C.c_int(hb if row1 is None else row1))
    return cc


def first_diff(got, want, what):
    """a message naming the first differing block and index"""
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(got != want)
    if not len(bad):
        return None
    i = tuple(int(v) for v in bad[0])
    return f"{what}: {len(bad)} values differ; first at {i}: got {got[i]}, want {want[i]}"


def first_rows_list(h1):
    """qs_hip_upsample_rows first_rows: 0, 1..7 and 8 (capped at the rows there are)"""
    return sorted({min(f, h1) for f in range(9)})


def fdct_case(hblk=6, wblk=9, seed=31):
    """an upsampled pixel buffer (any bytes are reachable there): random, flat 0 / 255, checkerboards, ramps;
    -> uint8 [hblk * 8, wblk * 8]"""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (hblk * 8, wblk * 8))
    yy, xx = np.mgrid[0:8, 0:8]
    tiles = [np.zeros((8, 8)), np.full((8, 8), 255), ((xx + yy) & 1) * 255, (xx & 1) * 255, xx * 36, yy * 36 + 3]
    for i, t in enumerate(tiles):
        by, bx = divmod(i * 5 % (hblk * wblk), wblk)
        px[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = t
    return px.astype(np.uint8)


def fdct_blocks_of(px):
    h, w = px.shape
    return px.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


def dequant_case(seed=41):
    """quantised coefficients over the whole int16 range under tables whose products wrap -> (q, c)"""
    rng = np.random.default_rng(seed)
    q = table("huge").copy()
    q[3:40] = table("std")[3:40]
    q[40:44] = 0
    c = rng.integers(-32768, 32768, (5, 7, 64))
    c[0, :, :] = rng.integers(-3, 4, (7, 64))
    return q, c.astype(np.int16)
