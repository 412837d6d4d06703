"""Case builders of the device decode's edge tests (tests/test_decode_cases.py on the CPU, tests/test_gpu_decode_edges.py
on the GPU): numpy only, seeded; and the host build of the product's decode arithmetic.  What each case is for:

  bound_blocks / bound_images  blocks on both sides of QS_DEC_FAST_BOUND whose signs are those of the DCT basis, so that
                               one pass-1 output is the L1 sum the bound is derived for; fast and slow blocks in one wave
  chunk_batch                  more jobs than one launch chunk holds, neighbours with different tile counts
  padded                       block arrays larger than the image needs (row stride != blocks needed)
  edge_sizes                   widths and heights around the 64 x 16 output tile, a 1 x 1 image in every layout
  colour_grid[_420]            every (Cb, Cr) pair at luma values that meet both clamps of every channel
"""
import ast
import re
from pathlib import Path

import numpy as np

from decode_oracle import blocks_needed, synth_image
from host_tools import Tool, build
from wire import pack_blocks

HERE = Path(__file__).resolve().parent
DECODE_H = HERE.parent / "jpeg-quantsmooth_amd" / "csrc" / "qs_decode.h"
TILE_W, TILE_H = 64, 16                                    # the kernel's output tile, in pixels


def header_constant(name):
    """#define NAME <integer> of csrc/qs_decode.h, read from its text"""
    m = re.search(rf"^#define\s+{name}\s+(\d+)\b", DECODE_H.read_text(), re.M)
    assert m, f"{name} not found in {DECODE_H}"
    return int(m.group(1))


def layouts():
    """LAYOUTS of tests/test_gpu_decode.py, read from its text (importing that module needs torch)"""
    m = re.search(r"^LAYOUTS = (\[.*?\])\n\n", (HERE / "test_gpu_decode.py").read_text(), re.M | re.S)
    assert m, "LAYOUTS not found in tests/test_gpu_decode.py"
    return ast.literal_eval(m.group(1))


# ---- pass-1 bound ---------------------------------------------------------------------------------------------------

# the IDCT each luma sampling sends its chroma through, and the points of that IDCT's column pass (pass 1)
KIND_OF = {(1, 1): "islow", (2, 2): "16x16", (2, 1): "16x8", (1, 2): "8x16", (4, 1): "16x8"}
PASS1_POINTS = {"islow": 8, "16x8": 8, "16x16": 16, "8x16": 16}
BOUND = 16384                                              # the issue's value of QS_DEC_FAST_BOUND (asserted in the tests)
# a single populated column avoids 0 and 4: pass 2 multiplies those by 2^13 in the 8-point row pass, so an error of a
# multiple of 2^21 in them vanishes modulo 2^28, the only bits of pass 2 that reach a sample
ONE_COLS = (1, 2, 3, 5, 6, 7)
HOT_COL = 1                                                # the column of the 35081 table that holds 35081


def basis_signs(points, i):
    """sign(cos((2i+1) k pi / (2 points))), k = 0..7: the signs of output i of a `points`-point inverse DCT"""
    c = np.cos((2 * i + 1) * np.arange(8) * np.pi / (2 * points))
    assert (np.abs(c) > 1e-3).all()
    return np.sign(c).astype(np.int64)


def _aligned(points, mag, cols_of, what):
    """for every pass-1 output row i and both signs: block[k*8+c] = +-s_i[k] * mag[k*8+c] in the columns cols_of(i)"""
    blocks, labels = [], []
    for i in range(points):
        s = basis_signs(points, i)
        for sgn in (1, -1):
            b = np.zeros((8, 8), np.int64)
            for c in cols_of(i):
                b[:, c] = sgn * s * mag.reshape(8, 8)[:, c]
            blocks.append(b.reshape(64))
            labels.append(f"{what}, row i={i}, sign {'+' if sgn > 0 else '-'}")
    return blocks, labels


def bound_blocks(kind):
    """-> list of groups, one per quant table: dict(table (64,) uint16, coefs (n, 64) int16, labels [n], mx (n,) =
    max|coef * table| of each block).  Sign-aligned blocks for every pass-1 output row and both signs, with all eight
    columns and with one column populated, at amplitudes around 16384 (the bound), 26292/26293 (the exact limit of a
    32-bit 16-point pass 1) and 35081/35082 (that of the 8-point one), up to 65535; and random-sign blocks."""
    points = PASS1_POINTS[kind]
    rng = np.random.default_rng(1000 + points + 7 * len(kind))
    ones = np.ones(64, np.int64)
    hot = ones.copy().reshape(8, 8)
    hot[:, HOT_COL] = 35081
    hot = hot.reshape(64)
    specs = [   # (table, [(coefficient magnitude, which columns are populated)])
        (ones, [(a, w) for a in (8192, 16383, 16384, 16385, 20000, 26292, 26293, 32767) for w in ("all", "one")]),
        (2 * ones, [(a, w) for a in (17541, 8192, 8193, 4096) for w in ("all", "one")]),
        (3 * ones, [(a, w) for a in (21845, 5461, 5462, 2731) for w in ("all", "one")]),
        (hot, [(1, "hot1"), (16384, "hotall"), (16384, "cold"), (8192, "cold")]),
    ]
    groups = []
    for table, amps in specs:
        blocks, labels = [], []
        for a, which in amps:
            mag = np.full(64, a, np.int64)
            if which in ("hot1", "hotall"):
                mag.reshape(8, 8)[:, HOT_COL] = 1
            amp = int((mag * table).max())
            if which == "all" or which == "hotall":
                cols = lambda i: range(8)
            elif which == "one":
                cols = lambda i: (ONE_COLS[i % 6],)
            elif which == "hot1":
                cols = lambda i: (HOT_COL,)
            else:                                          # every column but the hot one
                cols = lambda i: [c for c in range(8) if c != HOT_COL]
                amp = a
            b, lab = _aligned(points, mag, cols, f"{kind} amplitude {amp} ({which} columns, table {int(table.max())})")
            blocks += b
            labels += lab
        if table is ones:
            for lo, hi, n in ((8192, 32767, 48), (8192, 16384, 16)):
                m = rng.integers(lo, hi + 1, (n, 64)) * rng.choice(np.array([-1, 1]), (n, 64))
                blocks += list(m)
                labels += [f"{kind} random signs, magnitudes {lo}..{hi}, block {j}" for j in range(n)]
        coefs = np.array(blocks, np.int64)
        assert np.abs(coefs).max() <= 32767
        groups.append(dict(table=table.astype(np.uint16), coefs=coefs.astype(np.int16), labels=labels,
                           mx=np.abs(coefs * table).max(axis=1)))
    return groups


def bound_layout(mx, hb, wb, rng):
    """-> (hb, wb) block indices: fast blocks (mx <= BOUND) and slow ones, each shuffled, on the two colours of a
    checkerboard, every block at least once: any two horizontal neighbours lie on different sides of the bound"""
    fast, slow = np.flatnonzero(mx <= BOUND), np.flatnonzero(mx > BOUND)
    assert len(fast) and len(slow) and (hb * wb) // 2 >= max(len(fast), len(slow))
    rng.shuffle(fast)
    rng.shuffle(slow)
    y, x = np.divmod(np.arange(hb * wb), wb)
    even = (x + y) % 2 == 0
    idx = np.empty(hb * wb, np.int64)
    idx[even] = fast[np.arange(even.sum()) % len(fast)]
    idx[~even] = slow[np.arange((~even).sum()) % len(slow)]
    return idx.reshape(hb, wb)


def bound_images(hs, vs):
    """one RGB (no colour transform) image per quant table for luma sampling hs x vs: component 0 holds
    bound_blocks("islow"), the two chroma components that sampling's kind, laid out by bound_layout.  Each image carries
    kinds[ci], index[ci] (the block of the group at each array position) and groups[ci] besides the decode's arguments."""
    kind = KIND_OF[(hs, vs)]
    rng = np.random.default_rng(hs * 16 + vs)
    images = []
    for gl, gc in zip(bound_blocks("islow"), bound_blocks(kind)):
        assert np.array_equal(gl["table"], gc["table"])
        per_tile = [(TILE_W // 8) * (TILE_H // 8), (TILE_W // (8 * hs)) * (TILE_H // (8 * vs))]
        need = [2 * max(int((g["mx"] <= BOUND).sum()), int((g["mx"] > BOUND).sum())) for g in (gl, gc)]
        tiles = max(-(-n // p) for n, p in zip(need, per_tile))
        size = (4 * TILE_W, TILE_H * -(-tiles // 4))
        coefs, index, groups = [], [], [gl, gc, gc]
        for ci, g in enumerate(groups):
            hb, wb = blocks_needed(size, [hs, 1, 1], [vs, 1, 1], ci)
            idx = bound_layout(g["mx"], hb, wb, rng)
            index.append(idx)
            coefs.append(g["coefs"][idx])
        images.append(dict(coefs=coefs, quants=[g["table"] for g in groups], hsamp=[hs, 1, 1], vsamp=[vs, 1, 1],
                           colorspace=2, image_size=size, kinds=["islow", kind, kind], index=index, groups=groups))
    return images


def bound_expected(lj9, im):
    """the image's samples from libjpeg 9's own IDCT functions, block by block (4:1:1: _16x8 and 2x replication)"""
    planes = []
    w, h = im["image_size"]
    for ci, (g, idx) in enumerate(zip(im["groups"], im["index"])):
        out = lj9.blocks(im["kinds"][ci], g["coefs"], np.broadcast_to(g["table"], g["coefs"].shape))
        if ci and im["hsamp"][0] == 4:
            out = np.repeat(out, 2, axis=2)
        hb, wb = idx.shape
        r, c = out.shape[1:]
        planes.append(out[idx].transpose(0, 2, 1, 3).reshape(hb * r, wb * c)[:h, :w])
    return np.stack(planes, axis=2)


def bound_blame(im, got, want):
    """which block the first differing sample belongs to: its component, kind, amplitude and row i"""
    bad = np.argwhere(got != want)
    if not len(bad):
        return ""
    y, x, ci = (int(v) for v in bad[0])
    ph, pw = (8 * im["vsamp"][0], 8 * im["hsamp"][0]) if ci else (8, 8)
    k = int(im["index"][ci][y // ph, x // pw])
    return (f"{len(bad)} samples differ, first at (y, x, component) = ({y}, {x}, {ci}): got {got[y, x, ci]}, libjpeg "
            f"{want[y, x, ci]}; block: {im['groups'][ci]['labels'][k]}, max|dq| {int(im['groups'][ci]['mx'][k])}")


def small_image(rng, image_size, hsamp, vsamp, colorspace, amp=60, qmax=255):
    """decode_oracle.synth_image's in-range arrays and random tables, drawn block by block (no pool: cheap for the
    many small images of chunk_batch and edge_sizes)"""
    coefs, quants = [], []
    for ci in range(len(hsamp)):
        hb, wb = blocks_needed(image_size, hsamp, vsamp, ci)
        q = rng.integers(1, qmax + 1, 64).astype(np.uint16)
        blk = np.zeros((hb, wb, 64), np.int16)
        blk[:, :, 0] = rng.integers(-127, 128, (hb, wb)) * 8 // max(1, int(q[0]) // 8)
        ac = rng.integers(-amp, amp + 1, (hb, wb, 63)) // np.maximum(1, q[1:] // 4)
        ac[rng.random((hb, wb, 63)) < 0.6] = 0
        blk[:, :, 1:] = ac
        coefs.append(blk)
        quants.append(q)
    return dict(coefs=coefs, quants=quants, hsamp=list(hsamp), vsamp=list(vsamp), colorspace=colorspace,
                image_size=tuple(image_size))


# ---- launch chunks --------------------------------------------------------------------------------------------------

def tile_count(size):
    return -(-size[0] // TILE_W) * -(-size[1] // TILE_H)


def chunk_batch(n):
    """n images of 1 x 1 to 40 x 40 pixels that cycle through the ten layouts; the heights walk through the bands
    1..16, 17..32, 33..40, so no two neighbours have the same number of tiles"""
    rng = np.random.default_rng(4400 + n)
    lay = layouts()
    bands = [(1, 16), (17, 32), (33, 40)]
    ims = []
    for k in range(n):
        lo, hi = bands[k % 3]
        size = (int(rng.integers(1, 41)), int(rng.integers(lo, hi + 1)))
        if k == 0:
            size = (1, 1)
        elif k % 30 == 2:
            size = (40, 40)
        hs, vs, cs = lay[k % len(lay)]
        ims.append(small_image(rng, size, hs, vs, cs))
    return ims


# ---- array stride ---------------------------------------------------------------------------------------------------

def mcu_extra(im):
    """per component (extra_w, extra_h): what pads its block array to whole MCUs, as libjpeg allocates it"""
    ex = []
    for ci in range(len(im["coefs"])):
        hb, wb = blocks_needed(im["image_size"], im["hsamp"], im["vsamp"], ci)
        hs, vs = (im["hsamp"][ci], im["vsamp"][ci]) if len(im["coefs"]) > 1 else (1, 1)
        ex.append((-(-wb // hs) * hs - wb, -(-hb // vs) * vs - hb))
    return ex


def padded(im, extra_w, extra_h, poison=32767):
    """the image with each array embedded at the top left of one with extra_w more block columns and extra_h more block
    rows (ints, or one per component); every coefficient of the extra blocks is +-poison"""
    rng = np.random.default_rng(poison + 1)
    n = len(im["coefs"])
    ew = [extra_w] * n if np.isscalar(extra_w) else list(extra_w)
    eh = [extra_h] * n if np.isscalar(extra_h) else list(extra_h)
    coefs = []
    for c, dw, dh in zip(im["coefs"], ew, eh):
        hb, wb = c.shape[:2]
        big = (rng.choice(np.array([-poison, poison]), (hb + dh, wb + dw, 64))).astype(np.int16)
        big[:hb, :wb] = c
        coefs.append(big)
    return dict(im, coefs=coefs)


# ---- tile edges -----------------------------------------------------------------------------------------------------

EDGE_WIDTHS = (1, 7, 63, 64, 65, 127, 128, 129)
EDGE_HEIGHTS = (1, 15, 16, 17, 31, 32, 33)


def edge_sizes():
    """eight images per layout: a 1 x 1 image, and every other width with heights that rotate with the layout, so that
    each layout meets every width and every height"""
    rng = np.random.default_rng(6416)
    ims = []
    for li, (hs, vs, cs) in enumerate(layouts()):
        sizes = [(1, 1)] + [(EDGE_WIDTHS[j], EDGE_HEIGHTS[1 + (j - 1 + li) % 6]) for j in range(1, 8)]
        ims += [small_image(rng, s, hs, vs, cs) for s in sizes]
    return ims


# ---- colour conversion ----------------------------------------------------------------------------------------------

GRID_Y = (0, 1, 127, 128, 254, 255)


def _dc_table():
    q = np.full(64, 16, np.uint16)
    q[0] = 8                                               # a DC-only block of coefficient c is the flat sample 128 + c
    return q


def colour_grid(y):
    """a 4:4:4 YCbCr image of 256 x 256 DC-only blocks: luma y everywhere, Cb = block column, Cr = block row"""
    coefs = [np.zeros((256, 256, 64), np.int16) for _ in range(3)]
    coefs[0][:, :, 0] = y - 128
    coefs[1][:, :, 0] = np.arange(256)[None, :] - 128
    coefs[2][:, :, 0] = np.arange(256)[:, None] - 128
    return dict(coefs=coefs, quants=[_dc_table() for _ in range(3)], hsamp=[1, 1, 1], vsamp=[1, 1, 1], colorspace=3,
                image_size=(2048, 2048))


def colour_grid_420():
    """the 4:2:0 variant: 256 x 256 DC-only chroma blocks (Cb = column, Cr = row) under 512 x 512 DC-only luma blocks
    that walk through GRID_Y, so that each chroma block lies under several luma values"""
    by, bx = np.divmod(np.arange(512 * 512), 512)
    ysel = np.array(GRID_Y)[((by % 2) * 2 + bx % 2 + by // 2 + 5 * (bx // 2)) % len(GRID_Y)]
    coefs = [np.zeros((512, 512, 64), np.int16)] + [np.zeros((256, 256, 64), np.int16) for _ in range(2)]
    coefs[0][:, :, 0] = ysel.reshape(512, 512) - 128
    coefs[1][:, :, 0] = np.arange(256)[None, :] - 128
    coefs[2][:, :, 0] = np.arange(256)[:, None] - 128
    return dict(coefs=coefs, quants=[_dc_table() for _ in range(3)], hsamp=[2, 1, 1], vsamp=[2, 1, 1], colorspace=3,
                image_size=(4096, 4096))


# ---- the product's decode arithmetic on the host --------------------------------------------------------------------

class DecodeHost(Tool):
    """tests/decode_host.cpp (csrc/qs_decode.h compiled for the host), built on demand; a failed build fails the test"""

    def __init__(self, workdir):
        super().__init__(build("decode_host.cpp", flags=["-O1"]), workdir)

    def info(self):
        return {k: int(v) for k, v in (line.split("=") for line in self._run("info").stdout.split())}

    def blocks(self, kind, coefs, tables):
        """qd_idct_block of `kind` (islow, 16x16, 16x8, 8x16, 32x8) on each block -> (n, rows, cols) uint8"""
        n, data = pack_blocks(coefs, tables)
        src, out = self.tmp(".bin"), self.tmp(".out")
        src.write_bytes(data)
        self._run("block", kind, src, out)
        r, c = {"islow": (8, 8), "16x16": (16, 16), "16x8": (8, 16), "8x16": (16, 8), "32x8": (8, 32)}[kind]
        return np.fromfile(out, np.uint8).reshape(n, r, c)

    def ycc_rgb(self, ycc):
        """qd_ycc_rgb on (n, 3) uint8 (Y, Cb, Cr) -> (n, 3) uint8 (R, G, B)"""
        src, out = self.tmp(".bin"), self.tmp(".out")
        src.write_bytes(np.ascontiguousarray(ycc, np.uint8).tobytes())
        self._run("ycc", src, out)
        return np.fromfile(out, np.uint8).reshape(-1, 3)
