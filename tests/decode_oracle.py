"""libjpeg 9 as the oracle of the device decode (tests/libjpeg9_decode.c, compiled on demand against the libjpeg 9 the
rest of the suite links): whole-image decodes of coefficient arrays, and its exported IDCTs on single blocks.  No code of
this project or of the reference is involved.  If the helper cannot be built, the tests that need it fail."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
GOLD = HERE / "golden" / "cli"
JPEGINC = Path("/opt/conda/include")
JPEGLIB = Path("/opt/conda/lib/libjpeg.so.9")
MAGIC = 0x51534A43
KIND_SHAPE = {"islow": (8, 8), "16x16": (16, 16), "16x8": (8, 16), "8x16": (16, 8)}   # (rows, cols) out


class LibJpeg9:
    def __init__(self, workdir: Path):
        self.dir = Path(workdir)
        self.exe = self.dir / "libjpeg9_decode"
        cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc")
        r = subprocess.run([cc or "gcc", "-O2", "-Wall", f"-I{JPEGINC}", "-o", str(self.exe), str(HERE / "libjpeg9_decode.c"),
                            str(JPEGLIB), f"-Wl,-rpath,{JPEGLIB.parent}"], capture_output=True, text=True)
        if r.returncode or not self.exe.exists():
            pytest.fail(f"the libjpeg 9 oracle (tests/libjpeg9_decode.c) did not build:\n{r.stderr}")
        self.n = 0

    def _tmp(self, ext):
        self.n += 1
        return self.dir / f"t{os.getpid()}_{self.n}{ext}"

    def _run(self, *args):
        r = subprocess.run([str(self.exe), *map(str, args)], capture_output=True, text=True)
        if r.returncode:
            pytest.fail(f"libjpeg9_decode {args[0]} failed: {r.stderr}")

    def read(self, jpeg_path):
        """-> dict(coefs, quants, hsamp, vsamp, colorspace, image_size) of a JPEG file (jpeg_read_coefficients)"""
        out = self._tmp(".bin")
        self._run("read", jpeg_path, out)
        b = out.read_bytes()
        _, n, w, h, cs = struct.unpack_from("<5i", b, 0)
        off, geo = 20, []
        for _c in range(n):
            g = struct.unpack_from("<5i", b, off)
            q = np.frombuffer(b, np.uint16, 64, off + 20).copy()
            geo.append((g, q))
            off += 20 + 128
        coefs = []
        for (wb, hb, _hs, _vs, _hq), _q in geo:
            coefs.append(np.frombuffer(b, np.int16, wb * hb * 64, off).reshape(hb, wb, 64).copy())
            off += wb * hb * 128
        return dict(coefs=coefs, quants=[q if g[4] else None for g, q in geo], hsamp=[g[2] for g, _ in geo],
                    vsamp=[g[3] for g, _ in geo], colorspace=cs, image_size=(w, h))

    def decode(self, coefs, quants, hsamp, vsamp, colorspace, image_size):
        """libjpeg 9's pixels for these arrays: written with jpeg_write_coefficients, read back with jpeg_read_scanlines
        (JDCT_ISLOW, defaults) -> uint8 (H, W, C)"""
        n = len(coefs)
        parts = [struct.pack("<5i", MAGIC, n, image_size[0], image_size[1], colorspace)]
        for ci in range(n):
            c = coefs[ci]
            q = np.ones(64, np.uint16) if quants[ci] is None else np.asarray(quants[ci], np.uint16)
            parts.append(struct.pack("<5i", c.shape[1], c.shape[0], hsamp[ci], vsamp[ci], 1))
            parts.append(q.tobytes())
        for c in coefs:
            parts.append(np.ascontiguousarray(c, np.int16).tobytes())
        src, out = self._tmp(".bin"), self._tmp(".raw")
        src.write_bytes(b"".join(parts))
        self._run("decode", src, out)
        px = np.fromfile(out, np.uint8)
        w, h = image_size
        return px.reshape(h, w, px.size // (w * h))

    def blocks(self, kind, coefs, tables):
        """jpeg_idct_<kind> on each block: coefs (n, 64) int16, tables (n, 64) uint16 -> (n, rows, cols) uint8"""
        coefs = np.asarray(coefs, np.int16).reshape(-1, 64)
        tables = np.asarray(tables, np.uint16).reshape(-1, 64)
        src, out = self._tmp(".bin"), self._tmp(".out")
        rec = np.concatenate([coefs.view(np.uint16), tables], axis=1)
        src.write_bytes(struct.pack("<i", len(coefs)) + rec.astype(np.uint16).tobytes())
        self._run("block", kind, src, out)
        r, c = KIND_SHAPE[kind]
        return np.fromfile(out, np.uint8).reshape(len(coefs), r, c)


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
