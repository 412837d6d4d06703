"""shared helpers for the parity tests"""
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"


def golden_names():
    return sorted(p.stem for p in GOLDEN.glob("*.npz"))


def load_golden(name):
    d = np.load(GOLDEN / f"{name}.npz")
    n = int(d["ncomp"])
    job = dict(
        coefs=[d[f"in{ci}"] for ci in range(n)],
        quants=[d[f"q{ci}"] for ci in range(n)],
        flags=int(d["flags"]), niter=int(d["niter"]),
        kw=dict(hsamp=[int(v) for v in d["hsamp"]], vsamp=[int(v) for v in d["vsamp"]],
                colorspace=int(d["colorspace"]), image_size=tuple(int(v) for v in d["image_size"])),
    )
    want = dict(ret=int(d["ret"]), up=bool(int(d["up"])), hsamp0=int(d["hsamp0"]), vsamp0=int(d["vsamp0"]),
                coefs=[d[f"out{ci}"] for ci in range(n)], quants=[d[f"qout{ci}"] for ci in range(n)])
    return job, want


def assert_same_result(got, want, what=""):
    assert got["ret"] == want["ret"], f"{what}: return value {got['ret']} != {want['ret']}"
    assert bool(got["up"]) == bool(want["up"]), f"{what}: upsample flag"
    assert (got["hsamp0"], got["vsamp0"]) == (want["hsamp0"], want["vsamp0"]), f"{what}: sampling factors"
    for ci, (a, b) in enumerate(zip(got["coefs"], want["coefs"])):
        assert a.shape == b.shape, f"{what}: component {ci} shape {a.shape} != {b.shape}"
        nbad = int((a != b).sum())
        if nbad:
            blocks = np.argwhere((a != b).any(axis=2))
            raise AssertionError(f"{what}: component {ci}: {nbad} coefficients differ in "
                                 f"{len(blocks)} blocks, first at (by,bx)={tuple(blocks[0])}")
    for ci, (a, b) in enumerate(zip(got["quants"], want["quants"])):
        if a is None or b is None:
            assert a is None and b is None
        else:
            assert np.array_equal(a, b), f"{what}: component {ci} quant table"


# flag bits the GPU job layer does not implement (none left)
GPU_FLAG_MASK_UNSUPPORTED = 0


def inject_extreme_blocks(j, seed=7):
    """blocks whose dequantised DC lies beyond +-1023 with strong low AC terms: their IDCT
    depends on whether the +-1023 clamp has happened yet"""
    rng = np.random.default_rng(seed)
    coefs = [c.copy() for c in j["coefs"]]
    for ci, (c, q) in enumerate(zip(coefs, j["quants"])):
        hb, wb = c.shape[:2]
        for _ in range(max(2, hb * wb // 6)):
            by, bx = rng.integers(0, hb), rng.integers(0, wb)
            sgn = 1 if rng.integers(0, 2) else -1
            c[by, bx, 0] = sgn * (int(rng.integers(1200, 2000)) // int(q[0]))
            for k in (1, 8, 9, 2, 16):
                c[by, bx, k] = -sgn * (int(rng.integers(300, 1500)) // int(q[k])) * (1 if rng.integers(0, 2) else -1)
    return dict(j, coefs=coefs)


def fuzz_generators():
    """tools/fuzz_gpu.py's seeded job generators (trial_jobs, stop_trial_jobs, jobs_of, digest, kwargs, ...), without
    running its command line: the part of the file above `if mode == "gen":`"""
    import sys
    root = GOLDEN.parent.parent
    src = (root / "tools" / "fuzz_gpu.py").read_text().split('if mode == "gen":')[0]
    ns = {"__file__": str(root / "tools" / "fuzz_gpu.py")}
    argv = sys.argv
    sys.argv = ["fuzz_gpu.py", "import-only", "-"]
    try:
        exec(compile(src, "fuzz_gpu_generators", "exec"), ns)
    finally:
        sys.argv = argv
    return ns


def stop_corpus():
    """tests/golden/fuzz_stops.jsonl: one dict per trial"""
    import json
    with open(GOLDEN / "fuzz_stops.jsonl") as f:
        return [json.loads(line) for line in f]


# products beyond int16 in a 4:2:0 job: (component, block row, block column, coefficient index, coefficient, quantiser).
# Component 0 trips (the reference stops there: int16(c * q), then the +-1023 clamp); component 1 comes after the stop
# and is only dequantised (int16(c * q), no clamp); component 2 holds one product inside the range.
WRAP_PLANTS = [(0, 0, 0, 0, 20000, 2), (0, 3, 5, 9, -20000, 2), (0, 4, 4, 63, 11000, 3), (0, 5, 7, 1, -16385, 2),
               (1, 0, 0, 0, 30000, 3), (1, 2, 1, 17, -30000, 3), (1, 2, 2, 8, 16384, 2), (2, 1, 1, 5, -2048, 1)]


def wrap_job(synth):
    """a 4:2:0 job whose range check trips in luma with products beyond +-32767 (WRAP_PLANTS)"""
    y = synth.synth_ycc(120, 96, 2, 2, quality=50, seed=77)
    coefs = [c.copy() for c in y["coefs"]]
    quants = [q.copy() for q in y["quants"]]
    for ci, by, bx, e, c, q in WRAP_PLANTS:
        coefs[ci][by, bx, e] = c
        quants[ci][e] = q
    return dict(coefs=coefs, quants=quants, hsamp=y["hsamp"], vsamp=y["vsamp"], colorspace=3, image_size=(120, 96))


def wrap_expected(ci, c, q):
    """what the reference leaves for one WRAP_PLANTS entry after stopping at component 0"""
    v = int(np.int16(np.int32(c) * np.int32(q)))             # JCOEF arithmetic: the product wraps to int16
    return max(-1023, min(1023, v)) if ci == 0 else v


MARGIN = 4096


class Guarded:
    """a device buffer of n elements between two sentinel margins of MARGIN bytes (GPU tests: needs torch)"""

    def __init__(self, n, dtype=None):
        import torch
        dtype = torch.uint8 if dtype is None else dtype
        self.item = torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((2 * MARGIN + n * self.item,), 0xA5, dtype=torch.uint8, device="cuda")
        self.view = self.raw[MARGIN:MARGIN + n * self.item].view(dtype)

    def check(self, untouched_from=None):
        host = self.raw.cpu().numpy()
        assert (host[:MARGIN] == 0xA5).all() and (host[len(host) - MARGIN:] == 0xA5).all(), "a sentinel margin changed"
        if untouched_from is not None:
            assert (host[MARGIN + untouched_from:] == 0xA5).all(), "bytes at or beyond the capacity changed"
