"""libjpeg 9 as the oracle of the device compress (tests/libjpeg9_compress.c, compiled on demand against the libjpeg 9
the rest of the suite links): whole images through jpeg_write_scanlines (JDCT_ISLOW, smoothing_factor 0,
do_fancy_downsampling FALSE, one given table per component), read back with `libjpeg9_decode read`, and its exported
jpeg_fdct_islow on single blocks.  Also the host build of the compress's own arithmetic (tests/compress_host.cpp over
csrc/qs_compress.h) and the case grid the CPU and the GPU tests share.  If a helper cannot be built, the tests that
need it fail."""
import struct

import numpy as np

from decode_oracle import LibJpeg9
from host_tools import Tool, build, run
from wire import header, parse_image

# (name, hsamp, vsamp, colour space): every supported layout
LAYOUTS = [("gray", [1], [1], 1)] + \
          [(f"{'ycc' if cs == 3 else 'rgb'}{h}x{v}", [h, 1, 1], [v, 1, 1], cs)
           for cs in (3, 2) for h, v in ((1, 1), (2, 1), (1, 2), (2, 2), (4, 1))]
# (width, height): 18, 20 and 66 rows are where clamping pixels instead of downsampled rows goes wrong
SIZES = [(1, 1), (7, 9), (8, 8), (16, 17), (33, 18), (33, 20), (65, 66), (70, 50)]
EDGE_VALUES = [1, 2, 3, 255, 256, 32767, 65535]


def tables(kind, n, synth, rng=None):
    """n tables: 'ones', 'q50' (libjpeg's quality 50: luminance for component 0, chrominance for the others), or
    'edge' (per-coefficient values drawn from EDGE_VALUES)"""
    if kind == "ones":
        return [np.ones(64, np.uint16) for _ in range(n)]
    if kind == "q50":
        return [synth.quality_table(synth.STD_LUMA if ci == 0 else synth.STD_CHROMA, 50) for ci in range(n)]
    return [rng.choice(np.array(EDGE_VALUES, np.uint16), 64) for _ in range(n)]


def pixels(rng, size, nin):
    """random samples with a smooth part, so that every quantiser sees zero and non-zero outputs"""
    w, h = size
    y, x = np.mgrid[0:h, 0:w]
    base = 128 + 90 * np.sin(x / 5.0 + rng.random() * 6)[..., None] * np.cos(y / 7.0 + rng.random() * 6)[..., None]
    px = base + rng.integers(-40, 41, (h, w, nin))
    return np.clip(px, 0, 255).astype(np.uint8)


def all_colours():
    """4096 x 4096 RGB: each of the 2^24 colours once"""
    v = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8)


def pack(px, quants, hsamp, vsamp, colorspace):
    h, w, n = px.shape
    parts = [header(n, w, h, colorspace)]
    for ci in range(n):
        parts.append(struct.pack("<2i", hsamp[ci], vsamp[ci]))
        parts.append(np.asarray(quants[ci], np.uint16).tobytes())
    parts.append(np.ascontiguousarray(px).tobytes())
    return b"".join(parts)


class Compress9(Tool):
    def __init__(self, workdir):
        super().__init__(build("libjpeg9_compress.c", libjpeg=True), workdir)
        self.lj9 = LibJpeg9(self.dir)
        self.host_exe = self.build_host("compress_host", [])

    def build_host(self, name, extra, source="compress_host.cpp"):
        """tests/compress_host.cpp as a stand-alone program (extra: e.g. the sanitizer flags; name: what the caller
        calls the variant)"""
        return build(source, flags=["-g", *extra])

    @staticmethod
    def _run(exe, *args):
        """(the program is an argument here: an object of this class runs two or four of them)"""
        return run(exe, *args).stdout

    def _image(self, exe, px, quants, hsamp, vsamp, colorspace, *mode):
        """`image [mode] in out` of a host build -> the image dict its output holds"""
        src, out = self.tmp(".bin"), self.tmp(".out")
        src.write_bytes(pack(px, quants, hsamp, vsamp, colorspace))
        self._run(exe, "image", *mode, src, out)
        b = out.read_bytes()
        src.unlink()
        out.unlink()
        return parse_image(b, with_quants=False)

    def libjpeg(self, px, quants, hsamp, vsamp, colorspace, keep_file=False):
        """libjpeg 9's arrays for these pixels -> the image dict of LibJpeg9.read (with 'file': the JPEG's path)"""
        src, jpg = self.tmp(".bin"), self.tmp(".jpg")
        src.write_bytes(pack(px, quants, hsamp, vsamp, colorspace))
        self._run(self.exe, "image", src, jpg)
        im = self.lj9.read(jpg)
        src.unlink()
        if keep_file:
            im["file"] = jpg
        else:
            jpg.unlink()
        return im

    def host(self, px, quants, hsamp, vsamp, colorspace, exe=None):
        """the host build of csrc/qs_compress.h on the same input -> the same dict"""
        return self._image(exe or self.host_exe, px, quants, hsamp, vsamp, colorspace)

    def fdct(self, which, blocks, exe=None):
        """jpeg_fdct_islow ('libjpeg') or qc_fdct_row + qc_fdct_col ('host') on blocks (n, 64) uint8 -> (n, 64) int32"""
        blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 64)
        src, out = self.tmp(".bin"), self.tmp(".out")
        src.write_bytes(struct.pack("<i", len(blocks)) + blocks.tobytes())
        self._run(self.exe if which == "libjpeg" else (exe or self.host_exe), "block", src, out)
        return np.fromfile(out, np.int32).reshape(len(blocks), 64)


def assert_same_arrays(got, want, what=""):
    assert len(got) == len(want), f"{what}: {len(got)} components, expected {len(want)}"
    for ci, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, f"{what}: component {ci} has shape {a.shape}, expected {b.shape}"
        bad = np.argwhere(a != b)
        assert not len(bad), f"{what}: component {ci}: {len(bad)} coefficients differ, first at (by, bx, k) = " \
                             f"{tuple(bad[0])}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}"
