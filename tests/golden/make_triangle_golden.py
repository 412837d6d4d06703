"""Generate tests/golden/triangle/*.npz: what libjpeg-turbo, as Pillow runs it, decodes from small JPEG files, for the
decode's triangle mode (upsampling="triangle").  Needs Pillow with libjpeg-turbo and the libjpeg 9
the suite links (the files are written by tests/libjpeg9_encode.c from coefficient arrays):

    python tests/golden/make_triangle_golden.py            # write the fixtures
    python tests/golden/make_triangle_golden.py --check    # also: the host build of the filter on every layout x size

Every file is decoded twice, each time in a fresh Python process: with turbo's SIMD code and with JSIMD_FORCENONE=1 (its
C code).  The two must agree on every sample of every case -- the contract's domain is where they do -- or nothing is
written.  Each .npz holds, per case (triangle_oracle.load_fixtures reads them), the coefficient arrays, tables, sampling, colour space, size, turbo's pixels and (for
YCbCr files of up to 65 x 17 pixels, and the saturating cases) its upsampled components before colour conversion: data
only, replayable without Pillow.  (The components of the larger cases are compared in --check and live in the CPU test,
not stored: the directory stays near 400 KB.)
"""
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import jpegqs_pkg  # noqa: E402
from encode_oracle import LibJpeg9Enc  # noqa: E402
from triangle_oracle import FIXDIR, LAYOUTS, SIZES, TriHost, have_pillow, pillow_decode  # noqa: E402

synth = jpegqs_pkg.load().synth

# what is stored: the three filtered layouts at every size (141 x 93 for 2x2 only), the others where a tile or a filter
# condition changes
MOST = [s for s in SIZES if s != (141, 93)]
FEW = [(1, 1), (5, 5), (17, 17), (65, 17)]
STORED = {"ycc22": SIZES, "ycc21": MOST, "ycc12": MOST, "gray": FEW, "ycc11": FEW, "ycc41": FEW + [(130, 34)],
          "rgb22": [(3, 3), (6, 6), (17, 17), (65, 17), (129, 33)], "rgb21": [(5, 5), (65, 17), (129, 33)],
          "rgb12": [(5, 5), (65, 17), (129, 33)]}
FILE_OF = {"ycc22": "ycc22", "ycc21": "ycc21", "ycc12": "ycc12"}          # everything else: other.npz


def busy_chroma(coefs, seed):
    """random low-frequency AC terms on the chroma arrays: the samples of a block differ from their neighbours, and the
    IDCT's own columns and rows beyond the downsampled size differ from the last one inside it"""
    rng = np.random.default_rng(seed)
    low = [1, 8, 9, 2, 16, 10, 17, 3, 24]
    for c in coefs[1:]:
        c[..., low] += rng.integers(-3, 4, c.shape[:2] + (len(low),)).astype(np.int16)
    return coefs


def make_image(layout, size, seed):
    name, hs, vs, cs = layout
    w, h = size
    if len(hs) == 1:
        coef, q = synth.synth_gray(w, h, 75, seed)
        return dict(coefs=[coef], quants=[q], hsamp=hs, vsamp=vs, colorspace=cs, image_size=size)
    y = synth.synth_ycc(w, h, hs[0], vs[0], quality=75, seed=seed)
    return dict(coefs=busy_chroma([c.copy() for c in y["coefs"]], seed + 1), quants=y["quants"], hsamp=hs, vsamp=vs,
                colorspace=cs, image_size=size)


YCC_PIXELS = 65 * 17          # the components before colour conversion are stored up to this size (the file budget)


def saturating(hs, vs, size=(66, 18)):
    """chroma blocks that alternate between far below 0 and far above 255 with strong first harmonics: the range limit
    clips on both sides inside a block and across block borders, right where the filter mixes neighbours"""
    im = make_image(("sat", [hs, 1, 1], [vs, 1, 1], 3), size, 4242)
    for ci in (1, 2):
        c, q = im["coefs"][ci], im["quants"][ci]
        hb, wb = c.shape[:2]
        sign = np.where((np.arange(hb)[:, None] + np.arange(wb)[None, :] + ci) % 2 == 0, 1, -1)
        c[..., 0] = sign * (900 // int(q[0]))
        c[..., 1] = -sign * (700 // int(q[1]))
        c[..., 8] = sign * (600 // int(q[8]))
    return im


def cases(stored_only):
    out, seed = {}, 100
    for layout in LAYOUTS:
        for size in SIZES:
            seed += 1
            if stored_only and size not in STORED[layout[0]]:
                continue
            out[f"{layout[0]}_{size[0]}x{size[1]}"] = make_image(layout, size, seed)
    for hs, vs in ((2, 2), (2, 1), (1, 2)):
        out[f"sat{hs}{vs}_66x18"] = saturating(hs, vs)
    return out


def turbo(ims, work):
    """turbo's pixels and components for every image, asserted equal between its SIMD and its C code"""
    enc = LibJpeg9Enc(work)
    files = [enc.write(im) for im in ims.values()]
    simd, plain = pillow_decode(files, work, simd=True), pillow_decode(files, work, simd=False)
    bad = []
    for name, (p1, y1), (p2, y2) in zip(ims, simd, plain):
        if not np.array_equal(p1, p2) or (y1 is None) != (y2 is None) or (y1 is not None and not np.array_equal(y1, y2)):
            bad.append(name)
    assert not bad, f"turbo's SIMD and C decodes disagree on {bad}: outside the contract's domain, pick other inputs"
    return dict(zip(ims, simd))


def main():
    assert have_pillow(), "Pillow with libjpeg-turbo is needed to make these fixtures"
    check = "--check" in sys.argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        work = Path(tmp)
        ims = cases(stored_only=not check)
        want = turbo(ims, work)
        for name, im in ims.items():
            w, h = im["image_size"]
            assert want[name][0].shape == (h, w, 1 if len(im["coefs"]) == 1 else 3), name
        if check:
            host = TriHost(work)
            got = host.run(list(ims.values()))
            comp = host.run(list(ims.values()), planes=True)
            nbad = 0
            for name, g, c in zip(ims, got, comp):
                px, ycc = want[name]
                d = int((g != px).sum()) + (0 if ycc is None else int((c != ycc).sum()))
                if d:
                    nbad += 1
                    print(f"MISMATCH {name}: {d} samples")
            print(f"host build against turbo: {len(ims)} cases, {nbad} with a mismatch")
            assert nbad == 0
    FIXDIR.mkdir(exist_ok=True)
    files = {}
    for name, im in ims.items():
        layout = name.split("_")[0]
        size = im["image_size"]
        if layout in STORED and size not in STORED[layout]:
            continue
        d = files.setdefault(FILE_OF.get(layout, "other"), dict(names=[], meta=[], coefs=[], quants=[], pixels=[], ycc=[]))
        px, ycc = want[name]
        keep_ycc = ycc is not None and size[0] * size[1] <= max(YCC_PIXELS, 66 * 18 * name.startswith("sat"))
        n = len(im["coefs"])
        shapes = [v for c in im["coefs"] for v in c.shape[:2]] + [0] * (6 - 2 * n)
        d["names"].append(name)
        d["meta"].append([n, im["colorspace"], size[0], size[1], int(keep_ycc)] + list(im["hsamp"]) + [0] * (3 - n)
                         + list(im["vsamp"]) + [0] * (3 - n) + shapes)
        d["coefs"] += [np.asarray(c, np.int16).reshape(-1) for c in im["coefs"]]
        d["quants"] += [np.asarray(q, np.uint16).reshape(64) for q in im["quants"]]
        d["pixels"].append(px.reshape(-1))
        if keep_ycc:
            d["ycc"].append(ycc.reshape(-1))
    total = 0
    for stem, d in files.items():
        path = FIXDIR / f"{stem}.npz"
        # a handful of flat arrays per file (a zip entry per case and field would cost more than the data)
        np.savez_compressed(path, names=np.array(d["names"]), meta=np.array(d["meta"], np.int32),
                            coefs=np.concatenate(d["coefs"]), quants=np.stack(d["quants"]),
                            pixels=np.concatenate(d["pixels"]), ycc=np.concatenate(d["ycc"] or [np.zeros(0, np.uint8)]))
        total += path.stat().st_size
        print(f"{path.name}: {len(d['names'])} cases, {path.stat().st_size} bytes")
        assert path.stat().st_size < 256 * 1024, path
    print(f"total {total} bytes")


if __name__ == "__main__":
    main()
