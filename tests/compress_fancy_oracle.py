"""libjpeg 9 as the oracle of the device compress with its default DCT-scaled chroma downsampling
(tests/libjpeg9_compress_fancy.c, compiled on demand): whole images through jpeg_write_scanlines with
do_fancy_downsampling TRUE, and its exported jpeg_fdct_16x16 / _16x8 / _8x16 on single blocks.  Also the host build of
both modes' arithmetic (tests/compress_fancy_host.cpp over csrc/qs_compress.h) and the cases the CPU and the GPU tests
share.  The grid, the pixels, the tables and the comparison are those of compress_oracle.py."""
import struct

import numpy as np

from compress_oracle import LAYOUTS, SIZES, Compress9, assert_same_arrays, pack, pixels, tables  # noqa: F401
from host_tools import build

FANCY_SIZES = SIZES + [(31, 15), (17, 31), (63, 33)]
KINDS = ["ones", "q50", "edge"]
SHAPES = {"16x16": (16, 16), "16x8": (16, 8), "8x16": (8, 16)}       # name -> (samples wide, samples high)
SUBSAMPLED = [l for l in LAYOUTS if l[1][0] * l[2][0] > 1]


def extreme_blocks(w, h):
    """blocks whose samples are 0 / 255 by the sign of cos((2x+1) k pi / 32) (16 samples; / 16 for 8) for every k and both
    signs: in rows, in columns and in both (the product's sign) -- the inputs that reach each pass's L1 norm"""
    def signs(n):
        x = np.arange(n)
        return [np.cos((2 * x + 1) * k * np.pi / (2 * n)) >= 0 for k in range(8)]
    rows, cols = signs(w), signs(h)
    out = []
    for k in range(8):
        for flip in (False, True):
            out.append(np.broadcast_to(rows[k][None, :] ^ flip, (h, w)))
            out.append(np.broadcast_to(cols[k][:, None] ^ flip, (h, w)))
    for kr in range(8):
        for kc in range(8):
            for flip in (False, True):
                out.append((rows[kr][None, :] == cols[kc][:, None]) ^ flip)
    return (np.stack(out).astype(np.uint8) * 255).reshape(len(out), h * w)


def extreme_image(rng, shape, size):
    """a gray plane of `size` = (width, height) tiled with the extreme blocks of `shape`, every other block plain"""
    w, h = SHAPES[shape]
    ext = extreme_blocks(w, h)
    W, H = size
    plane = rng.integers(0, 256, (H + h, W + w)).astype(np.uint8)
    i = 0
    for by in range(0, H, h):
        for bx in range(0, W, w):
            if (by // h + bx // w) & 1:
                plane[by:by + h, bx:bx + w] = ext[i % len(ext)].reshape(h, w)
                i += 1
    return plane[:H, :W]


class CompressFancy9(Compress9):
    """Compress9 with do_fancy_downsampling TRUE: .libjpeg() is libjpeg 9's default, .host(..., mode=) the host build
    of either mode, .fdct16() the three scaled block functions; .box is the Compress9 of the box mode"""

    def __init__(self, workdir):
        super().__init__(workdir)
        self.box_exe = self.exe
        self.exe = build("libjpeg9_compress_fancy.c", libjpeg=True)
        self.fancy_host_exe = self.build_fancy_host("compress_fancy_host", [])

    def build_fancy_host(self, name, extra):
        return self.build_host(name, extra, "compress_fancy_host.cpp")

    def libjpeg_box(self, px, quants, hsamp, vsamp, colorspace):
        """libjpeg 9 with do_fancy_downsampling FALSE on the same input"""
        fancy, self.exe = self.exe, self.box_exe
        try:
            return self.libjpeg(px, quants, hsamp, vsamp, colorspace)
        finally:
            self.exe = fancy

    def host(self, px, quants, hsamp, vsamp, colorspace, exe=None, mode="dct"):
        return self._image(exe or self.fancy_host_exe, px, quants, hsamp, vsamp, colorspace, mode)

    def fdct16(self, which, shape, blocks, exe=None):
        """jpeg_fdct_<shape> ('libjpeg') or the host build's block function ('host') on blocks (n, H * W) uint8 ->
        (n, 64) int32"""
        w, h = SHAPES[shape]
        blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, w * h)
        src, out = self.tmp(".bin"), self.tmp(".out")
        src.write_bytes(struct.pack("<i", len(blocks)) + blocks.tobytes())
        self._run(self.exe if which == "libjpeg" else (exe or self.fancy_host_exe), "block", shape, src, out)
        r = np.fromfile(out, np.int32).reshape(len(blocks), 64)
        src.unlink()
        out.unlink()
        return r

    def norms(self):
        return {k: int(v) for k, v in (l.split("=") for l in self._run(self.fancy_host_exe, "norms").split())}
