"""libjpeg 9 as the oracle of the device decode at reduced sizes (tests/libjpeg9_decode_scaled.c, compiled on demand
against the libjpeg 9 the rest of the suite links): whole-image decodes with scale_num / scale_denom = 1 / N, and its
exported reduced IDCTs on single blocks; the host build of the product's arithmetic (tests/decode_scaled_host.cpp); and
the seeded case builders the CPU and GPU tests share.  If a helper cannot be built, the tests that need it fail."""
import struct

import numpy as np

from decode_cases import DECODE_H, padded, small_image  # noqa: F401
from host_tools import Tool, build
from wire import pack_blocks, pack_image
KINDS = ("4x4", "2x2", "1x1", "8x4", "4x2", "2x1", "4x8", "2x4", "1x2")        # width x height
DENOMS = (2, 4, 8)
TILE_W, TILE_H = 64, 16
# (luma hs, luma vs, colorspace): gray, YCbCr 1x1, 2x1, 1x2, 2x2, 4x1, RGB-kept 2x2
LAYOUTS = [(1, 1, 1), (1, 1, 3), (2, 1, 3), (1, 2, 3), (2, 2, 3), (4, 1, 3), (2, 2, 2)]
BOUND4 = 141869            # QS_DEC_FAST_BOUND4: floor((2^31 - 1 - 2^10) / 15137), 15137 the 4-point pass 1's L1 norm
L1_4 = 15137


def scaled_size(image_size, denom):
    m = 8 // denom
    return -(-image_size[0] * m // 8), -(-image_size[1] * m // 8)


def kind_of(hs, vs, denom):
    """the IDCT (width x height) and the horizontal replication of a chroma component under hs x vs luma at 1 / denom"""
    m = 8 // denom
    return f"{m * min(hs, 2)}x{m * vs}", 2 if hs == 4 else 1


class _Helper(Tool):
    """a program that takes `decode in out DENOM` and `block KIND in out`"""

    def decode(self, im, denom):
        """the image's samples at 1 / denom -> uint8 (H', W', C); the size is asserted to be ceil(W * M / 8) x ceil(H * M / 8)"""
        src, out = self.tmp(".bin"), self.tmp(".raw")
        src.write_bytes(pack_image(im))
        self._run("decode", src, out, denom)
        b = out.read_bytes()
        w, h, c = struct.unpack_from("<3i", b, 0)
        assert (w, h) == scaled_size(im["image_size"], denom), (self.exe.name, (w, h), im["image_size"], denom)
        src.unlink()
        out.unlink()
        return np.frombuffer(b, np.uint8, w * h * c, 12).reshape(h, w, c).copy()

    def blocks(self, kind, coefs, tables):
        """jpeg_idct_<kind> on each block: coefs (n, 64) int16, tables (n, 64) or (64,) uint16 -> (n, height, width) uint8"""
        n, data = pack_blocks(coefs, tables)
        src, out = self.tmp(".bin"), self.tmp(".out")
        src.write_bytes(data)
        self._run("block", kind, src, out)
        w, h = int(kind[0]), int(kind[2])
        return np.fromfile(out, np.uint8).reshape(n, h, w)


class LibJpeg9Scaled(_Helper):
    """tests/libjpeg9_decode_scaled.c: the libjpeg 9 oracle of the reduced sizes"""

    def __init__(self, workdir):
        super().__init__(build("libjpeg9_decode_scaled.c", libjpeg=True), workdir)


class ScaledHost(_Helper):
    """csrc/qs_decode.h's reduced sizes compiled for the host (tests/decode_scaled_host.cpp); sanitize=True: with
    -fsanitize=address,undefined (a stand-alone program: nothing is loaded into Python)"""

    def __init__(self, workdir, sanitize=False):
        # (C++20 under the sanitizers: the 64-bit pass 1 shared with the full size shifts negative values left, which
        # every compiler of this code defines as two's complement and the language does from C++20 on)
        super().__init__(build("decode_scaled_host.cpp", flags=["-std=c++20"] if sanitize else ["-O1"], sanitize=sanitize),
                         workdir)

    def info(self):
        return {k: int(v) for k, v in (line.split("=") for line in self._run("info").stdout.split())}


# ---- blocks -----------------------------------------------------------------------------------------------------------

def _factor(t):
    """(coef, q) with coef * q == t, |coef| <= 32767, 1 <= q <= 65535; None if there is none"""
    for q in range(1, 65536):
        if t % q == 0 and t // q <= 32767:
            return t // q, q
    return None


def random_blocks(seed, n=192):
    """(coefs, tables): thirds of in-range values, full-range coefficients with small tables, full range of both"""
    rng = np.random.default_rng(seed)
    c = np.concatenate([rng.integers(-1024, 1024, (n // 3, 64)), rng.integers(-32768, 32768, (n // 3, 64)),
                        rng.integers(-32768, 32768, (n - 2 * (n // 3), 64))])
    t = np.concatenate([rng.integers(1, 256, (n // 3, 64)), rng.integers(0, 17, (n // 3, 64)),
                        rng.integers(0, 65536, (n - 2 * (n // 3), 64))])
    return c.astype(np.int16), t.astype(np.uint16)


def extreme_blocks(seed):
    """blocks of +-32767 and -32768 (constant, checkerboards, random signs) against tables 0, 1, 255, 32768, 65535, a
    ramp over 0 .. 65535 and random ones"""
    rng = np.random.default_rng(seed)
    i = np.arange(64)
    chk = np.where((i // 8 + i % 8) % 2 == 0, 1, -1)
    pats = [np.full(64, 32767), np.full(64, -32768), np.full(64, -32767), 32767 * chk, -32767 * chk,
            np.where(chk > 0, 32767, -32768), np.where(chk > 0, -32768, 32767),
            np.where(i % 2 == 0, 32767, -32768), np.where(i // 8 % 2 == 0, 32767, -32768)]
    pats += [np.where(rng.random(64) < 0.5, 32767, -32768) for _ in range(8)]
    tabs = [np.full(64, v) for v in (0, 1, 255, 32768, 65535)] + [(i * 65535) // 63, 65535 - (i * 65535) // 63]
    tabs += [rng.integers(0, 65536, 64) for _ in range(4)]
    c = np.array([p for p in pats for _ in tabs], np.int64)
    t = np.array([t for _ in pats for t in tabs], np.int64)
    return c.astype(np.int16), t.astype(np.uint16)


def bound_groups(kind):
    """-> list of dict(table (64,), coefs (n, 64), fast (n,)), one per quant table, each with blocks on both sides of its
    bound.  For the kinds whose pass 1 is the 4-point column with its own descale (4x4, 8x4): rows 1 and 3 carry the
    sign patterns of that pass's two matrix rows, (10703, 4433) and (4433, -10704), both signs, in every column or in
    one, at |coef * q| = 141868 (q 116), 141869 = QS_DEC_FAST_BOUND4 (q 7) and 141870 (q 10) -- just below, at and just
    above -- and further out on both sides, up to 32767 * 65535.  For 4x8 (the 8-point pass 1): the DCT basis signs of
    each of the eight outputs at amplitudes around QS_DEC_FAST_BOUND = 16384 and around 35081, where 32 bits wrap."""
    w, h = int(kind[0]), int(kind[2])
    groups = []
    if h == 4 and w >= 4:
        assert (2 ** 31 - 1 - 1024) // L1_4 == BOUND4 and 20267 * 7 == BOUND4
        for q, cs in ((7, (20266, 20267, 20268, 32767)), (116, (1223, 1224, 612)), (10, (14186, 14187, 7000)),
                      (65535, (2, 3, 32767))):
            blocks, fast = [], []
            for coef in cs:
                for s1, s3 in ((1, 1), (1, -1), (-1, -1), (-1, 1)):
                    for cols in (range(w), (1,), (w - 1,)):
                        b = np.zeros((8, 8), np.int64)
                        for c in cols:
                            b[1, c], b[3, c] = s1 * coef, s3 * coef
                            b[0, c], b[2, c] = 3, -2
                        blocks.append(b.reshape(64))
                        fast.append(coef * q <= BOUND4)
            groups.append(dict(table=np.full(64, q, np.uint16), coefs=np.array(blocks).astype(np.int16), fast=np.array(fast)))
    elif kind == "4x8":
        for q, cs in ((1, (16383, 16384, 16385, 26292, 32767)), (2, (8192, 8193, 17540, 17541))):
            blocks, fast = [], []
            for coef in cs:
                for i in range(8):
                    s = np.sign(np.cos((2 * i + 1) * np.arange(8) * np.pi / 16)).astype(np.int64)
                    for sgn in (1, -1):
                        for cols in (range(4), (1,), (3,)):
                            b = np.zeros((8, 8), np.int64)
                            for c in cols:
                                b[:, c] = sgn * s * coef
                            blocks.append(b.reshape(64))
                            fast.append(coef * q <= 16384)
            groups.append(dict(table=np.full(64, q, np.uint16), coefs=np.array(blocks).astype(np.int16), fast=np.array(fast)))
    else:
        return None
    assert all(g["fast"].any() and (~g["fast"]).any() for g in groups)
    return groups


def bound_blocks(kind):
    """bound_groups in one: (coefs, tables, fast)"""
    gs = bound_groups(kind)
    return (np.concatenate([g["coefs"] for g in gs]), np.concatenate([np.broadcast_to(g["table"], g["coefs"].shape) for g in gs]),
            np.concatenate([g["fast"] for g in gs]))


def extreme_group(seed, table):
    """full-range coefficients, most of them +-32767 / -32768, under one table"""
    rng = np.random.default_rng(seed)
    c = rng.integers(-32768, 32768, (96, 64)).astype(np.int16)
    ext = rng.random(c.shape) < 0.7
    c[ext] = rng.choice(np.array([32767, -32768], np.int16), int(ext.sum()))
    return dict(table=np.asarray(table, np.uint16), coefs=c, fast=np.zeros(len(c), bool))


def block_image(hs, vs, groups):
    """an RGB-kept image (no colour transform: every IDCT's samples go straight out) for luma sampling hs x vs whose
    component ci holds groups[ci]'s blocks, every block at least once, blocks within and beyond their bound on the two
    colours of a checkerboard where the group has both: neighbouring lanes take different passes.  16 chroma blocks
    per row: several output tiles at 1/2.  Carries index[ci] (the group's block at each array position)."""
    coefs, index = [], []
    need = [2 * max(int(g["fast"].sum()), int((~g["fast"]).sum())) for g in groups]      # (each colour holds one side)
    chb = max(-(-need[ci] // (16 * (1 if ci else hs * vs))) for ci in range(3))
    for ci, g in enumerate(groups):
        hb, wb = (chb, 16) if ci else (chb * vs, 16 * hs)
        y, x = np.divmod(np.arange(hb * wb), wb)
        fast, slow = np.flatnonzero(g["fast"]), np.flatnonzero(~g["fast"])
        if len(fast) and len(slow):
            even = (x + y) % 2 == 0
            idx = np.empty(hb * wb, np.int64)
            idx[even] = fast[np.arange(even.sum()) % len(fast)]
            idx[~even] = slow[np.arange((~even).sum()) % len(slow)]
            assert even.sum() >= len(fast) and (~even).sum() >= len(slow)
        else:
            idx = np.arange(hb * wb) % len(g["coefs"])
        index.append(idx.reshape(hb, wb))
        coefs.append(g["coefs"][index[-1]])
    return dict(coefs=coefs, quants=[g["table"] for g in groups], hsamp=[hs, 1, 1], vsamp=[vs, 1, 1], colorspace=2,
                image_size=(8 * 16 * hs, 8 * chb * vs), index=index, groups=groups)


def block_expected(lj9, im, denom):
    """the image's samples at 1 / denom from libjpeg 9's own IDCT functions, block by block"""
    hs, vs = im["hsamp"][0], im["vsamp"][0]
    planes = []
    for ci, (g, idx) in enumerate(zip(im["groups"], im["index"])):
        kind, rep = kind_of(hs, vs, denom) if ci else kind_of(1, 1, denom)
        assert kind in KINDS
        out = np.repeat(lj9.blocks(kind, g["coefs"], g["table"]), rep, axis=2)
        hb, wb = idx.shape
        r, c = out.shape[1:]
        planes.append(out[idx].transpose(0, 2, 1, 3).reshape(hb * r, wb * c))
    w, h = scaled_size(im["image_size"], denom)
    assert all(p.shape == (h, w) for p in planes)
    return np.stack(planes, axis=2)


# ---- whole images -----------------------------------------------------------------------------------------------------

def sizes(denom):
    """the small sizes, and every width with every height at the edges of a 64 x 16 output tile's input footprint at
    1 / denom; the largest is 513 x 129"""
    base = [(1, 1), (7, 7), (8, 8), (9, 9), (15, 17), (141, 93)]
    return base + [(w, h) for w in (64 * denom - 1, 64 * denom, 64 * denom + 1)
                   for h in (16 * denom - 1, 16 * denom, 16 * denom + 1)]


def image_cases(denom):
    """[(label, image)]: every layout at every size of sizes(denom); arrays wider and taller than the image needs, with
    junk (+-32767) outside the geometry"""
    out = []
    for li, (hs, vs, cs) in enumerate(LAYOUTS):
        for si, size in enumerate(sizes(denom)):
            rng = np.random.default_rng(denom * 1000 + li * 37 + si)
            n = 1 if cs == 1 else 3
            im = small_image(rng, size, [hs] + [1] * (n - 1), [vs] + [1] * (n - 1), cs)
            im = padded(im, 1 + (li + si) % 3, 1 + si % 2)
            out.append((f"{hs}x{vs} cs{cs} {size[0]}x{size[1]} /{denom}", im))
    return out


def expected_images(lj9, denom):
    return [(label, im, lj9.decode(im, denom)) for label, im in image_cases(denom)]
