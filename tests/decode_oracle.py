"""libjpeg 9 as the oracle of the device decode (tests/libjpeg9_decode.c, compiled on demand against the libjpeg 9 the
rest of the suite links): whole-image decodes of coefficient arrays, and its exported IDCTs on single blocks.  No code of
this project or of the reference is involved.  If the helper cannot be built, the tests that need it fail."""
import numpy as np

from host_tools import HERE, JPEGINC, JPEGLIB, Tool, build  # noqa: F401
from wire import MAGIC, pack_blocks, pack_image, parse_image  # noqa: F401

GOLD = HERE / "golden" / "cli"
KIND_SHAPE = {"islow": (8, 8), "16x16": (16, 16), "16x8": (8, 16), "8x16": (16, 8)}   # (rows, cols) out


class LibJpeg9(Tool):
    def __init__(self, workdir):
        super().__init__(build("libjpeg9_decode.c", libjpeg=True), workdir)

    def read(self, jpeg_path):
        """-> dict(coefs, quants, hsamp, vsamp, colorspace, image_size) of a JPEG file (jpeg_read_coefficients)"""
        out = self.tmp(".bin")
        self._run("read", jpeg_path, out)
        return parse_image(out.read_bytes())

    def decode(self, coefs, quants, hsamp, vsamp, colorspace, image_size):
        """libjpeg 9's pixels for these arrays: written with jpeg_write_coefficients, read back with jpeg_read_scanlines
        (JDCT_ISLOW, defaults) -> uint8 (H, W, C)"""
        src, out = self.tmp(".bin"), self.tmp(".raw")
        src.write_bytes(pack_image(dict(coefs=coefs, quants=quants, hsamp=hsamp, vsamp=vsamp, colorspace=colorspace,
                                        image_size=image_size)))
        self._run("decode", src, out)
        px = np.fromfile(out, np.uint8)
        w, h = image_size
        return px.reshape(h, w, px.size // (w * h))

    def blocks(self, kind, coefs, tables):
        """jpeg_idct_<kind> on each block: coefs (n, 64) int16, tables (n, 64) uint16 -> (n, rows, cols) uint8"""
        n, data = pack_blocks(coefs, tables)
        src, out = self.tmp(".bin"), self.tmp(".out")
        src.write_bytes(data)
        self._run("block", kind, src, out)
        r, c = KIND_SHAPE[kind]
        return np.fromfile(out, np.uint8).reshape(n, r, c)


def blocks_needed(image_size, hsamp, vsamp, ci):
    """libjpeg's width_in_blocks / height_in_blocks of component ci"""
    w, h = image_size
    mh, mv = max(hsamp), max(vsamp)
    return -(-h * vsamp[ci] // (8 * mv)), -(-w * hsamp[ci] // (8 * mh))


def synth_image(rng, image_size, hsamp, vsamp, colorspace, amp=60, qmax=255):
    """in-range coefficient arrays (|AC| within libjpeg's 10-bit limit after the tables) and random tables"""
    coefs, quants = [], []
    for ci in range(len(hsamp)):
        hb, wb = blocks_needed(image_size, hsamp, vsamp, ci)
        q = rng.integers(1, qmax + 1, 64).astype(np.uint16)
        pool = np.zeros((4096, 64), np.int16)             # blocks drawn from a pool: large images stay cheap
        pool[:, 0] = rng.integers(-127, 128, 4096) * 8 // max(1, int(q[0]) // 8)   # (DC differences within 11 bits)
        ac = rng.integers(-amp, amp + 1, (4096, 63)) // np.maximum(1, q[1:] // 4)
        ac[rng.random((4096, 63)) < 0.6] = 0
        pool[:, 1:] = ac
        coefs.append(pool[rng.integers(0, 4096, (hb, wb))])
        quants.append(q)
    return dict(coefs=coefs, quants=quants, hsamp=list(hsamp), vsamp=list(vsamp), colorspace=colorspace,
                image_size=tuple(image_size))
