"""MI355X tests of the device-resident batch route (qs_hip_do_quantsmooth_device_batch through
torch_qs.quantsmooth_batch_): each job of a batch must give exactly what quantsmooth_ gives on a copy of the same input
-- coefficients, replacement chroma, quant tables, sampling factors and stop -- and, where stated, what the goldens,
the reference (fuzz corpus digests, range-check stops) or the host job layer give."""
import json
from pathlib import Path

import numpy as np
import pytest

from helpers import assert_same_result, golden_names, load_golden

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KW = ("hsamp", "vsamp", "colorspace", "image_size")


@pytest.fixture(scope="module")
def tq(gpu):
    import torch
    from jpeg_quantsmooth_amd import torch_qs
    assert torch.cuda.is_available()
    return torch, torch_qs


def _kw(j):
    return {k: j[k] for k in KW if j.get(k) is not None}


def _result(torch, ts, stop, out, kw):
    """the job layer's result dict of one job from its tensors, its stop and its entry of what the call returned"""
    coefs = [t.cpu().numpy() for t in ts]
    up = out["coef_up"] is not None and stop == 0
    if up:
        coefs[1], coefs[2] = out["coef_up"][0].cpu().numpy(), out["coef_up"][1].cpu().numpy()
    if stop == 0:
        hs, vs = out["hsamp0"], out["vsamp0"]
    else:                                                    # the reference drops the replacement chroma (:2835)
        hs, vs = (kw.get("hsamp") or [1])[0], (kw.get("vsamp") or [1])[0]
    return dict(ret=stop, up=up, hsamp0=hs, vsamp0=vs, coefs=coefs, quants=out["quants"],
                inplace=[t.cpu().numpy() for t in ts])


def _tensors(torch, coefs):
    return [torch.from_numpy(np.ascontiguousarray(c, dtype=np.int16)).cuda() for c in coefs]


def run_batch(tq, jobs, flags, niter):
    """jobs: dicts with coefs, quants and the keyword arguments -> one result dict per job"""
    torch, torch_qs = tq
    images = [dict(coefs=_tensors(torch, j["coefs"]), quants=j["quants"], **_kw(j)) for j in jobs]
    res = torch_qs.quantsmooth_batch_(images, flags, niter)
    stops = res["stop"].cpu().numpy().tolist()
    assert len(stops) == len(jobs)
    return [_result(torch, im["coefs"], int(s), out, _kw(j)) for im, s, out, j in zip(images, stops, res["images"], jobs)]


def run_single(tq, j, flags, niter):
    torch, torch_qs = tq
    ts = _tensors(torch, j["coefs"])
    res = torch_qs.quantsmooth_(ts, j["quants"], flags, niter, **_kw(j))
    return _result(torch, ts, int(res["stop"].item()), res, _kw(j))


def assert_same_as_single(got, want, what):
    assert_same_result(got, want, what)
    for ci, (a, b) in enumerate(zip(got["inplace"], want["inplace"])):
        assert np.array_equal(a, b), f"{what}: component {ci} in place"


def check_against_single(tq, jobs, flags, niter, what):
    got = run_batch(tq, jobs, flags, niter)
    for i, (g, j) in enumerate(zip(got, jobs)):
        assert_same_as_single(g, run_single(tq, j, flags, niter), f"{what}: job {i}")
    return got


def _golden_job(name):
    j, want = load_golden(name)
    return dict(coefs=j["coefs"], quants=j["quants"], **j["kw"]), j, want


# ---- 1. the goldens, grouped by flags / niter ---------------------------------------------------------------------

def test_goldens_in_mixed_geometry_batches(tq):
    groups = {}
    for name in golden_names():
        job, j, want = _golden_job(name)
        groups.setdefault((j["flags"], j["niter"]), []).append((name, job, want))
    assert any(len(g) > 3 for g in groups.values())
    for (flags, niter), members in sorted(groups.items()):
        got = check_against_single(tq, [m[1] for m in members], flags, niter, f"flags {flags} niter {niter}")
        for g, (name, _, want) in zip(got, members):
            assert_same_result(g, want, name)


# ---- 2. the committed fuzz corpus ---------------------------------------------------------------------------------

def _fuzz_generators():
    """tools/fuzz_gpu.py's seeded job generators (trial_jobs, digest, kwargs), without running its command line"""
    import sys
    src = (ROOT / "tools" / "fuzz_gpu.py").read_text().split('if mode == "gen":')[0]
    ns = {"__file__": str(ROOT / "tools" / "fuzz_gpu.py")}
    argv = sys.argv
    sys.argv = ["fuzz_gpu.py", "import-only", "-"]
    try:
        exec(compile(src, "fuzz_gpu_generators", "exec"), ns)
    finally:
        sys.argv = argv
    return ns


def _as_job(ns, j):
    return dict(coefs=j["coefs"], quants=j["quants"], **ns["kwargs"](j))


def test_fuzz_corpus_batches(tq):
    """every batch trial of tests/golden/fuzz_s2.jsonl as one batch, and the single-job trials packed into batches of
    up to 16 jobs of one flags / niter setting: each job's digest equals the reference's"""
    ns = _fuzz_generators()
    fails, nbatch, single = [], 0, {}
    for line in open(ROOT / "tests" / "golden" / "fuzz_s2.jsonl"):
        rec = json.loads(line)
        made, flags, niter, _ = ns["trial_jobs"](rec["seed0"], rec["trial"])
        if not rec["batch"]:
            single.setdefault((flags, niter), []).append((made[0], rec))
            continue
        nbatch += 1
        got = run_batch(tq, [_as_job(ns, j) for j, _ in made], flags, niter)
        for i, (g, (_, desc)) in enumerate(zip(got, made)):
            if ns["digest"](g) != rec["expect"][i]:
                fails.append(f"batch ({rec['seed0']},{rec['trial']}) job {i} {desc} flags={flags} niter={niter}")
    nsingle = 0
    for (flags, niter), members in sorted(single.items()):
        for k in range(0, len(members), 16):
            part = members[k:k + 16]
            got = run_batch(tq, [_as_job(ns, j) for (j, _), _ in part], flags, niter)
            nsingle += len(part)
            for g, ((_, desc), rec) in zip(got, part):
                if ns["digest"](g) != rec["expect"][0]:
                    fails.append(f"single ({rec['seed0']},{rec['trial']}) {desc} flags={flags} niter={niter}")
    assert nbatch == 100 and nsingle == 300 and not fails, f"{len(fails)} failed: {fails[:5]}"


# ---- 3. more planes than one set holds ----------------------------------------------------------------------------

@pytest.mark.parametrize("quality,njobs", [(3, 40), (6, 30)])
def test_more_than_56_planes_per_pass(tq, synth, pkg, quality, njobs):
    jobs = []
    for k in range(njobs):
        y = synth.synth_ycc(48 + 16 * (k % 5), 32 + 8 * (k % 7), 2, 2, quality=40 + k, seed=100 + k)
        jobs.append(dict(coefs=y["coefs"], quants=y["quants"], hsamp=y["hsamp"], vsamp=y["vsamp"], colorspace=3))
    check_against_single(tq, jobs, pkg.flags_for_quality(quality), 2, f"{njobs} jobs q{quality}")


# ---- 4. per-job stop isolation ------------------------------------------------------------------------------------

def _ycc(synth, seed, w=96, h=80):
    y = synth.synth_ycc(w, h, 2, 2, quality=50, seed=seed)
    return dict(coefs=y["coefs"], quants=y["quants"], hsamp=y["hsamp"], vsamp=y["vsamp"], colorspace=3, image_size=(w, h))


def _bad_in(j, ci):
    c = [a.copy() for a in j["coefs"]]
    c[ci][1, 2, 0] = 0x7ff                                   # 0x7ff * q >= 0x800 for any q >= 2
    return dict(j, coefs=c)


def _big_quant(j, ci):
    q = [a.copy() for a in j["quants"]]
    q[ci][63] = 0x800
    return dict(j, quants=q)


@pytest.mark.parametrize("quality", [3, 6])
def test_stop_is_decided_per_job(tq, hip, synth, pkg, quality):
    """job 2 trips luma's range check, job 5 chroma's, job 7 has a quantiser >= 0x800: each equals the host job layer
    (the reference's stop semantics); every other job has stop 0 and its full result"""
    flags, niter = pkg.flags_for_quality(quality), 2
    jobs = [_ycc(synth, 40 + k) for k in range(9)]
    jobs[2], jobs[5], jobs[7] = _bad_in(jobs[2], 0), _bad_in(jobs[5], 1), _big_quant(jobs[7], 2)
    got = check_against_single(tq, jobs, flags, niter, f"stops q{quality}")
    for i, (g, j) in enumerate(zip(got, jobs)):
        want = hip.do_quantsmooth(j["coefs"], j["quants"], flags, niter, **_kw(j))
        assert_same_result(g, want, f"q{quality} job {i}")
        assert g["ret"] == (1 if i in (2, 5, 7) else 0), i


# ---- 5. every route in one batch ----------------------------------------------------------------------------------

def test_mixed_routes_under_q6(tq, synth, pkg):
    """coupled 4:2:0, 4:4:4 and 4:2:2, a grey image (independent sets) and a job with an all-ones table (the single-job
    sequence) in one batch"""
    jobs = []
    for hs, vs, seed in ((2, 2, 61), (1, 1, 62), (2, 1, 63)):
        y = synth.synth_ycc(88, 72, hs, vs, quality=55, seed=seed)
        jobs.append(dict(coefs=y["coefs"], quants=y["quants"], hsamp=y["hsamp"], vsamp=y["vsamp"], colorspace=3))
    coef, quant = synth.synth_gray(80, 56, 60)
    jobs.append(dict(coefs=[coef], quants=[quant]))
    ones = _ycc(synth, 64)
    ones["quants"] = [ones["quants"][0], np.ones(64, np.uint16), ones["quants"][2]]
    jobs.append(ones)
    jobs.append(_ycc(synth, 65, 120, 64))
    got = check_against_single(tq, jobs, pkg.flags_for_quality(6), 3, "mixed routes")
    assert [g["up"] for g in got[:4]] == [True, False, True, False] and got[5]["up"]


# ---- 6. graph capture ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("quality", [3, 6])
def test_graph_capture_replays_reset_the_words(tq, hip, synth, pkg, quality):
    """one batch call captured on one stream, replayed three times with new inputs copied into the same tensors: clean,
    two jobs tripping, clean again -- stops and results after each replay.  Jobs 5 and 6 take the sequential route: a
    quantiser >= 0x800 decides job 5's stop, job 6 has an all-ones chroma table (and trips in the second round)"""
    torch, torch_qs = tq
    flags, niter = pkg.flags_for_quality(quality), 2
    rounds = [[_ycc(synth, 70 + 10 * r + k) for k in range(7)] for r in range(3)]
    rounds[0][5] = _big_quant(rounds[0][5], 2)
    rounds[0][6]["quants"] = [rounds[0][6]["quants"][0], np.ones(64, np.uint16), rounds[0][6]["quants"][2]]
    for r in rounds[1:]:
        for k, j in enumerate(r):
            j["quants"] = rounds[0][k]["quants"]
    rounds[1][3] = _bad_in(rounds[1][3], 0)
    rounds[1][6] = _bad_in(rounds[1][6], 0)
    static = [_tensors(torch, j["coefs"]) for j in rounds[0]]
    images = [dict(coefs=ts, quants=j["quants"], **_kw(j)) for ts, j in zip(static, rounds[0])]
    warm = torch_qs.quantsmooth_batch_(images, flags, niter)  # prepares the workspace
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = torch_qs.quantsmooth_batch_(images, flags, niter, workspace=warm["workspace"])
    for r, jobs in enumerate(rounds):
        for ts, j in zip(static, jobs):
            for t, c in zip(ts, j["coefs"]):
                t.copy_(torch.from_numpy(c))
        g.replay()
        torch.cuda.synchronize()
        stops = res["stop"].cpu().numpy().tolist()
        assert stops == [1 if k == 5 or (r == 1 and k in (3, 6)) else 0 for k in range(7)], (r, stops)
        for k, (ts, j) in enumerate(zip(static, jobs)):
            got = _result(torch, ts, stops[k], res["images"][k], _kw(j))
            want = hip.do_quantsmooth(j["coefs"], j["quants"], flags, niter, **_kw(j))
            assert_same_result(got, want, f"replay {r} job {k}")


# ---- 7. full-size images against the host batch route -------------------------------------------------------------

@pytest.mark.parametrize("quality", [3, 6])
def test_sixteen_1080p_equal_the_host_batch(tq, hip, synth, pkg, quality):
    flags, niter = pkg.flags_for_quality(quality), 3
    base = [_ycc(synth, 5 + k, 1920, 1080) for k in range(4)]
    jobs = [base[k % 4] for k in range(16)]                  # (each job still has tensors of its own)
    got = run_batch(tq, jobs, flags, niter)
    want = hip.do_quantsmooth_batch([dict(coefs=j["coefs"], quants=j["quants"], **_kw(j)) for j in jobs], flags, niter)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same_result(g, w, f"1080p q{quality} job {i}")


# ---- 8. one job ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ycc420_141x93_q6_n2", "gray64_q3_n3", "gray64_badcoef_q3_n2"])
def test_one_job_equals_quantsmooth_(tq, name):
    job, j, want = _golden_job(name)
    got = check_against_single(tq, [job], j["flags"], j["niter"], name)
    assert_same_result(got[0], want, name)


def test_a_tensor_twice_is_refused(tq):
    torch, torch_qs = tq
    job, j, _ = _golden_job("gray64_q3_n3")
    t = _tensors(torch, job["coefs"])
    with pytest.raises(ValueError, match="appears earlier"):
        torch_qs.quantsmooth_batch_([dict(coefs=t, quants=job["quants"])] * 2, j["flags"], j["niter"])
