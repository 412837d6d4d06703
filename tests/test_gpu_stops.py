"""MI355X tests of the range-check stop (reference quantsmooth.h:2596-2610) on every route.

1. tests/golden/fuzz_stops.jsonl -- jobs built to trip, with digests from the compiled reference
   (tests/test_stop_corpus.py re-derives it) -- through the host job layer (single calls and batches), its banded
   planes, the sharded route, and the device-resident route one job per call and in batches.
2. Exact, hand-written cases for the device route's precheck and fix-up kernels (csrc/qs_kernels_device.hip): the
   boundary products at every coefficient index (every lane of the quantiser mapping) at the edges of precheck and
   fix-up workgroups, a captured batch replayed with the first tripping component moving, and products that wrap in
   int16 before the clamp."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import test_gpu_device_batch as devb
import test_gpu_device_job as devj
from helpers import WRAP_PLANTS, assert_same_result, fuzz_generators, stop_corpus, wrap_expected, wrap_job

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CORPUS = "tests/golden/fuzz_stops.jsonl"


@pytest.fixture(scope="module")
def tq(gpu):
    import torch
    from jpeg_quantsmooth_amd import torch_qs
    assert torch.cuda.is_available()
    return torch, torch_qs


@pytest.fixture(scope="module")
def gens():
    return fuzz_generators()


# ---- 1. the stop corpus on every route ------------------------------------------------------------------------------

@pytest.mark.parametrize("env", [{}, {"QS_HIP_SPLIT_BLOCKS": "60", "QS_HIP_BAND_BLOCKS": "40"},
                                 {"QS_HIP_DEVICES": "0,0,0", "QS_HIP_SHARD_MIN_BLOCKS": "1"}],
                         ids=["job layer", "banded planes", "three logical devices"])
def test_stop_corpus_through_the_host_routes(env):
    """tools/fuzz_gpu.py run: every single trial through qs_hip_do_quantsmooth, every batch trial through
    qs_hip_do_quantsmooth_batch"""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz_gpu.py"), "run", str(ROOT / CORPUS)],
                       capture_output=True, text=True, timeout=600, cwd=str(ROOT), env=dict(os.environ, **env))
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_stop_corpus_through_the_device_route(tq, gens):
    """torch_qs.quantsmooth_ on every single trial"""
    fails, done = [], 0
    for rec in stop_corpus():
        if rec["batch"]:
            continue
        made, flags, niter, _ = gens["jobs_of"](rec)
        (j, desc), = made
        got = devj.run_device(tq, j["coefs"], j["quants"], flags, niter, **gens["kwargs"](j))
        done += 1
        if not gens["matches"](gens["digest"](got), rec["expect"][0]):
            fails.append(f"({rec['trial']}) {desc} flags={flags} niter={niter}")
    assert done > 100 and not fails, f"{len(fails)} of {done} failed: {fails[:5]}"


def test_stop_corpus_through_device_batches(tq, gens):
    """torch_qs.quantsmooth_batch_ on every batch trial (up to 50 jobs, up to three chunks of records): each job's
    digest is the reference's and each job equals quantsmooth_ on a copy, in-place arrays included"""
    fails, nbatch, njobs = [], 0, 0
    for rec in stop_corpus():
        if not rec["batch"]:
            continue
        made, flags, niter, _ = gens["jobs_of"](rec)
        jobs = [devb._as_job(gens, j) for j, _ in made]
        got = devb.check_against_single(tq, jobs, flags, niter, f"trial {rec['trial']}")
        nbatch += 1
        for i, (g, (_, desc)) in enumerate(zip(got, made)):
            njobs += 1
            if not gens["matches"](gens["digest"](g), rec["expect"][i]):
                fails.append(f"({rec['trial']}) job {i} {desc} flags={flags} niter={niter}")
    assert nbatch > 50 and njobs > 600 and not fails, f"{len(fails)} of {njobs} failed: {fails[:5]}"


# ---- 2. exact cases of the device route's kernels -------------------------------------------------------------------

BOUNDARY = {0x7ff: 0, 0x800: 1, -0x800: 0, -0x801: 1}      # product -> the reference's stop (val |= p + 0x800; val >> 12)


@pytest.mark.parametrize("hb,wb,where", [(3, 5, "first"), (3, 5, "last"), (8, 16, "last"), (3, 43, "last"),
                                         (32, 32, "last"), (25, 41, "last")],
                         ids=["first block", "last block", "128 blocks", "129 blocks", "1024 blocks", "1025 blocks"])
def test_boundary_products_at_every_index(tq, hip, synth, pkg, hb, wb, where):
    """64 gray jobs in one batch; job e plants the product at coefficient index e under quantiser 1, in the first or the
    last block of a component whose last block ends or starts a precheck workgroup (128 blocks) or a fix-up workgroup
    (1024 blocks).  Each job's stop is the reference's formula and its result the host job layer's"""
    flags, niter = pkg.flags_for_quality(3), 1
    coef, quant = synth.synth_gray(wb * 8, hb * 8, 50, seed=hb * 100 + wb)
    assert coef.shape[:2] == (hb, wb)
    by, bx = (0, 0) if where == "first" else (hb - 1, wb - 1)
    for product, stop in BOUNDARY.items():
        jobs = []
        for e in range(64):
            c, q = coef.copy(), quant.copy()
            q[e] = 1
            c[by, bx, e] = product
            jobs.append(dict(coefs=[c], quants=[q]))
        got = devb.run_batch(tq, jobs, flags, niter)
        want = hip.do_quantsmooth_batch(jobs, flags, niter)
        assert [g["ret"] for g in got] == [stop] * 64, hex(product)
        for e, (g, w) in enumerate(zip(got, want)):
            assert_same_result(g, w, f"product {product:#x} at index {e}")


def _cmyk(synth, seed, w=160, h=120):
    planes = [synth.synth_gray(w, h, 40 + 10 * k, seed=seed + k) for k in range(4)]
    return dict(coefs=[p[0] for p in planes], quants=[p[1] for p in planes], hsamp=[1] * 4, vsamp=[1] * 4, colorspace=4,
                image_size=(w, h))


def _trip(j, plants):
    """plants: (component, last block or not, coefficient index): 0x7ff * q >= 0x800 for any q >= 2"""
    coefs = [c.copy() for c in j["coefs"]]
    for ci, last, e in plants:
        hb, wb = coefs[ci].shape[:2]
        by, bx = (hb - 1, wb - 1) if last else (hb // 2, 1)
        assert j["quants"][ci][e] >= 2
        coefs[ci][by, bx, e] = 0x7ff
    return dict(j, coefs=coefs)


def test_first_tripping_component_moves_across_graph_replays(tq, hip, synth, pkg):
    """one batch captured under the --quality 6 flags: a four-component job (plane-set route), a 4:2:0 job (coupled
    route) and a 4:2:0 job with a ones-with-a-zero chroma table (sequential route; when luma trips, the reference
    leaves that chroma untouched, not dequantised); replayed with the first tripping component
    of the four-component job at 3, 0, 2, none, and with two trips in one job -- stops and results equal the host job
    layer after every replay"""
    torch, torch_qs = tq
    flags, niter = pkg.flags_for_quality(6), 2
    base = [_cmyk(synth, 300), devb._ycc(synth, 310, 176, 136), devb._ycc(synth, 320, 176, 136)]
    ones_zero = np.ones(64, np.uint16)
    ones_zero[0] = 0                                         # (dequantising it zeroes the DC: restoring it does not)
    base[2]["quants"] = [base[2]["quants"][0], ones_zero, base[2]["quants"][2]]
    rounds = [
        [[(3, True, 63)], [], [(0, False, 0)]],
        [[(0, True, 7)], [(2, True, 56)], []],
        [[(2, False, 33), (3, True, 1)], [(0, True, 2)], [(2, True, 8)]],
        [[], [], []],
        [[(1, True, 62), (3, False, 0)], [(1, False, 4), (2, True, 63)], [(0, True, 9), (2, False, 1)]],
    ]
    kws = [devb._kw(j) for j in base]
    static = [devb._tensors(torch, j["coefs"]) for j in base]
    images = [dict(coefs=ts, quants=j["quants"], **kw) for ts, j, kw in zip(static, base, kws)]
    warm = torch_qs.quantsmooth_batch_(images, flags, niter)   # prepares the workspace
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = torch_qs.quantsmooth_batch_(images, flags, niter, workspace=warm["workspace"])
    for r, plants in enumerate(rounds):
        jobs = [_trip(j, p) for j, p in zip(base, plants)]
        for ts, j in zip(static, jobs):
            for t, c in zip(ts, j["coefs"]):
                t.copy_(torch.from_numpy(c))
        g.replay()
        torch.cuda.synchronize()
        stops = res["stop"].cpu().numpy().tolist()
        assert stops == [int(bool(p)) for p in plants], (r, stops)
        for k, (ts, j, kw) in enumerate(zip(static, jobs, kws)):
            got = devb._result(torch, ts, stops[k], res["images"][k], kw)
            want = hip.do_quantsmooth(j["coefs"], j["quants"], flags, niter, **kw)
            assert_same_result(got, want, f"replay {r} job {k}")


@pytest.mark.parametrize("quality", [3, 6])
def test_int16_wrap_before_the_clamp(tq, reference, synth, pkg, quality):
    """products beyond +-32767: the tripped component holds clamp(int16(c * q)), the component after it int16(c * q)
    (no clamp) -- as the reference leaves them (tests/test_stop_corpus.py checks the same on the reference), one job per
    call and in a batch"""
    flags, niter = pkg.flags_for_quality(quality), 2
    j = wrap_job(synth)
    kw = devb._kw(j)
    want = reference.do_quantsmooth(j["coefs"], j["quants"], flags, niter, **kw)
    single = devj.run_device(tq, j["coefs"], j["quants"], flags, niter, **kw)
    batch = devb.run_batch(tq, [j, devb._ycc(synth, 330)], flags, niter)
    for what, got in (("quantsmooth_", single), ("quantsmooth_batch_", batch[0])):
        assert got["ret"] == 1, what
        for ci, by, bx, e, c, q in WRAP_PLANTS[:-1]:
            assert int(got["coefs"][ci][by, bx, e]) == wrap_expected(ci, c, q), (what, ci, by, bx, e)
        assert_same_result(got, want, what)
    assert batch[1]["ret"] == 0
