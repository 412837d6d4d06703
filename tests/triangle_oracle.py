"""What the tests of the decode's triangle mode share (upsampling="triangle": libjpeg-turbo's chroma upsampling,
DESIGN.md section 12.1): the recorded fixtures of tests/golden/triangle (made by tests/golden/make_triangle_golden.py from
libjpeg-turbo as Pillow runs it), the host build of the filter (tests/decode_triangle_host.cpp), Pillow in a child
process with and without turbo's SIMD code, and the arrays-with-junk variant of an image."""
import os
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np

from host_tools import HERE, Tool, build
from wire import MAGIC, pack_image  # noqa: F401

FIXDIR = HERE / "golden" / "triangle"

# the sizes of the mode's contract: both sides of the Wc <= 2 rule, the 64 x 16 tile and its neighbours, a halo that
# crosses tile corners in both directions, and the suite's odd size
SIZES = [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (15, 15), (16, 16), (17, 17), (63, 15), (64, 16), (65, 17),
         (129, 33), (130, 34), (141, 93)]
# (name, hsamp, vsamp, colorspace)
LAYOUTS = [("gray", [1], [1], 1), ("ycc11", [1, 1, 1], [1, 1, 1], 3), ("ycc21", [2, 1, 1], [1, 1, 1], 3),
           ("ycc12", [1, 1, 1], [2, 1, 1], 3), ("ycc22", [2, 1, 1], [2, 1, 1], 3), ("ycc41", [4, 1, 1], [1, 1, 1], 3),
           ("rgb22", [2, 1, 1], [2, 1, 1], 2), ("rgb21", [2, 1, 1], [1, 1, 1], 2), ("rgb12", [1, 1, 1], [2, 1, 1], 2)]


def kw(im):
    return dict(hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"], image_size=im["image_size"])


def load_fixtures():
    """-> [dict(name, im: the image dict decode takes (numpy arrays), pixels: turbo's output (H, W, C), ycc: turbo's
    upsampled components before colour conversion (H, W, 3) or None)] from every file of tests/golden/triangle"""
    out = []
    for path in sorted(FIXDIR.glob("*.npz")):
        d = np.load(path)
        coefs, quants, pixels, ycc = d["coefs"], d["quants"], d["pixels"], d["ycc"]
        at = dict(c=0, q=0, p=0, y=0)

        def take(arr, key, n):
            at[key] += n
            return arr[at[key] - n:at[key]]

        for name, m in zip(d["names"], d["meta"].tolist()):
            n, cs, w, h, has_ycc = m[:5]
            shapes = [(m[11 + 2 * ci], m[12 + 2 * ci]) for ci in range(n)]
            im = dict(coefs=[take(coefs, "c", hb * wb * 64).reshape(hb, wb, 64) for hb, wb in shapes],
                      quants=[take(quants, "q", 1)[0] for _ in range(n)], hsamp=m[5:5 + n], vsamp=m[8:8 + n],
                      colorspace=cs, image_size=(w, h))
            c = 1 if n == 1 else 3
            out.append(dict(name=str(name), im=im, pixels=take(pixels, "p", w * h * c).reshape(h, w, c),
                            ycc=take(ycc, "y", w * h * 3).reshape(h, w, 3) if has_ycc else None))
        assert (at["c"], at["q"], at["p"], at["y"]) == (coefs.size, len(quants), pixels.size, ycc.size), path
    return out


def with_junk(im, extra_w=2, extra_h=1, seed=5):
    """the image with every array extra_w block columns wider and extra_h block rows taller than libjpeg's geometry,
    and with junk (large coefficients of both signs) in every block outside that geometry"""
    rng = np.random.default_rng(seed)
    coefs = []
    for c in im["coefs"]:
        hb, wb = c.shape[:2]
        big = rng.choice(np.array([-1200, -300, 250, 1100], np.int16), (hb + extra_h, wb + extra_w, 64))
        big[:hb, :wb] = c
        coefs.append(np.ascontiguousarray(big))
    return dict(im, coefs=coefs)


def pack_case(im, planes=False) -> bytes:
    return struct.pack("<i", 1 if planes else 0) + pack_image(im)


class TriHost(Tool):
    """tests/decode_triangle_host.cpp: the triangle mode of csrc/qs_decode.h on the host, tile by tile as the kernel"""
    SILENT = True

    def __init__(self, workdir, sanitize=False):
        super().__init__(build("decode_triangle_host.cpp", sanitize=sanitize), workdir)

    def run(self, ims, planes=False):
        """-> one uint8 (H, W, C) per image: the pixels, or with planes the upsampled components without colour
        conversion; fails on a non-zero exit or anything on stderr (a sanitizer report)"""
        src, dst = self.tmp(".bin"), self.tmp(".out")
        src.write_bytes(struct.pack("<i", len(ims)) + b"".join(pack_case(im, planes) for im in ims))
        self._run("run", src, dst)
        b = np.fromfile(dst, np.uint8)
        src.unlink()
        dst.unlink()
        out, off = [], 0
        for im in ims:
            w, h = im["image_size"]
            c = 1 if len(im["coefs"]) == 1 else 3
            out.append(b[off:off + w * h * c].reshape(h, w, c))
            off += w * h * c
        assert off == b.size
        return out


PILLOW_CHILD = r"""
import io, sys
import numpy as np
from PIL import Image
out = {}
names = sys.argv[2:]
for k, path in enumerate(names):
    data = open(path, "rb").read()
    im = Image.open(io.BytesIO(data))
    px = np.asarray(im)
    out[f"p{k}"] = px if px.ndim == 3 else px[:, :, None]
    if im.mode == "RGB" and b"Adobe" not in data[:400]:
        im = Image.open(io.BytesIO(data))
        im.draft("YCbCr", im.size)
        assert im.mode == "YCbCr", im.mode
        out[f"y{k}"] = np.asarray(im)
np.savez(sys.argv[1], **out)
"""


def have_pillow() -> bool:
    try:
        from PIL import features
    except ImportError:
        return False
    return bool(features.check_feature("libjpeg_turbo"))


def pillow_decode(files, workdir: Path, simd=True):
    """libjpeg-turbo's decode of each JPEG file (bytes) in a fresh Python process -- with JSIMD_FORCENONE=1 when simd is
    False: turbo's C code -> [(pixels (H, W, C), the upsampled YCbCr components (H, W, 3) or None)]"""
    workdir = Path(workdir)
    paths = []
    for k, data in enumerate(files):
        p = workdir / f"pil{os.getpid()}_{k}.jpg"
        p.write_bytes(data)
        paths.append(p)
    res = workdir / f"pil{os.getpid()}.npz"
    env = dict(os.environ)
    env.pop("JSIMD_FORCENONE", None)
    if not simd:
        env["JSIMD_FORCENONE"] = "1"
    r = subprocess.run([sys.executable, "-c", PILLOW_CHILD, str(res), *map(str, paths)], capture_output=True, text=True,
                       env=env)
    assert r.returncode == 0, f"the Pillow child process failed:\n{r.stderr[-4000:]}"
    d = np.load(res)
    out = [(d[f"p{k}"], d[f"y{k}"] if f"y{k}" in d.files else None) for k in range(len(files))]
    for p in paths + [res]:
        p.unlink()
    return out
