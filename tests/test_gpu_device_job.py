"""MI355X tests of the device-resident job route (qs_hip_do_quantsmooth_device through torch_qs.quantsmooth_):
coefficients live in torch device tensors, the job runs on the current stream, `stop` is read from the device word.
Pinned to the goldens, the committed fuzz corpus, the compiled reference (range-check stops) and the job layer
(full-size images), and captured into a single-stream torch.cuda.graph."""
import json
from pathlib import Path

import numpy as np
import pytest

from helpers import assert_same_result, golden_names, load_golden

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


# the compiled reference's answers for this file's own inputs, for checkouts where oracle/_ref cannot be built
RECORDED = ROOT / "tests" / "golden" / "device_job_reference.json.gz"


@pytest.fixture(scope="module")
def reference():
    """the compiled unmodified reference (oracle/_ref) where it was built; elsewhere the oracle port, checked call by call
    against digests of the compiled reference's results for these tests' inputs (RECORDED, written by
    QS_RECORD_REFERENCE=1 with oracle/_ref built) -- tests/conftest.py's fixture of the same name, on its own file"""
    import os
    from oracle import oracle as om
    if not om.have_ref("none"):
        om.build_ref()
    if not om.have_ref("none"):
        yield om.RecordedReference(path=RECORDED)
    elif os.environ.get("QS_RECORD_REFERENCE") == "1":
        rec = om.RecordedReference(live=om.Reference("none"), path=RECORDED)
        yield rec
        rec.save()
    else:
        yield om.Reference("none")


@pytest.fixture(scope="module")
def tq(gpu):
    import torch
    from jpeg_quantsmooth_amd import torch_qs
    assert torch.cuda.is_available()
    return torch, torch_qs


def _result(torch, ts, res, kw):
    """the job layer's result dict from the tensors and what quantsmooth_ returned (reads the device stop word)"""
    stop = int(res["stop"].item())
    coefs = [t.cpu().numpy() for t in ts]
    up = res["coef_up"] is not None and stop == 0
    if up:
        coefs[1], coefs[2] = res["coef_up"][0].cpu().numpy(), res["coef_up"][1].cpu().numpy()
    if stop == 0:
        hs, vs = res["hsamp0"], res["vsamp0"]
    else:                                                    # the reference drops the replacement chroma (:2835)
        hs, vs = (kw.get("hsamp") or [1])[0], (kw.get("vsamp") or [1])[0]
    return dict(ret=stop, up=up, hsamp0=hs, vsamp0=vs, coefs=coefs, quants=res["quants"])


def run_device(tq, coefs, quants, flags, niter, **kw):
    torch, torch_qs = tq
    ts = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.int16)).cuda() for c in coefs]
    res = torch_qs.quantsmooth_(ts, quants, flags, niter, **kw)
    return _result(torch, ts, res, kw)


@pytest.mark.parametrize("name", golden_names())
def test_golden_through_the_device_route(tq, name):
    j, want = load_golden(name)
    got = run_device(tq, j["coefs"], j["quants"], j["flags"], j["niter"], **j["kw"])
    assert_same_result(got, want, name)


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


def test_fuzz_corpus_through_the_device_route(tq):
    """tests/golden/fuzz_s2.jsonl (expected digests from the reference), every non-batch trial"""
    ns = _fuzz_generators()
    fails, done = [], 0
    for line in open(ROOT / "tests" / "golden" / "fuzz_s2.jsonl"):
        rec = json.loads(line)
        if rec["batch"]:
            continue
        made, flags, niter, _ = ns["trial_jobs"](rec["seed0"], rec["trial"])
        (j, desc), = made
        got = run_device(tq, j["coefs"], j["quants"], flags, niter, **ns["kwargs"](j))
        done += 1
        if ns["digest"](got) != rec["expect"][0]:
            fails.append(f"({rec['seed0']},{rec['trial']}) {desc} flags={flags} niter={niter}")
    assert done > 200 and not fails, f"{len(fails)} of {done} failed: {fails[:5]}"


# ---- the reference's range-check stop, decided on the device ------------------------------------------------------

def stop_cases(synth, flags_for_quality):
    """(name, job kwargs, flags, niter): one bad block in component 0, 1, 2 of a 4:2:0 q6 and a q3 job; a quantiser
    >= 0x800 in component 1; bad blocks next to an all-ones table (and one with a zero quantiser)"""
    y = synth.synth_ycc(96, 80, 2, 2, quality=50, seed=21)
    base = dict(coefs=y["coefs"], quants=y["quants"], hsamp=y["hsamp"], vsamp=y["vsamp"], colorspace=3, image_size=(96, 80))
    out = []

    def bad_in(j, ci, by=1, bx=2):
        c = [a.copy() for a in j["coefs"]]
        c[ci][by, bx, 0] = 0x7ff                             # 0x7ff * q >= 0x800 for any q >= 2
        return dict(j, coefs=c)

    def with_quant(j, ci, q):
        qs = [a.copy() for a in j["quants"]]
        qs[ci] = np.asarray(q, dtype=np.uint16)
        return dict(j, quants=qs)

    ones = np.ones(64, np.uint16)
    ones_zero = ones.copy()
    ones_zero[5] = 0
    big = y["quants"][1].copy()
    big[63] = 0x800
    for quality in (6, 3):
        fl = flags_for_quality(quality)
        for ci in range(3):
            out.append((f"q{quality}_bad{ci}", bad_in(base, ci), fl, 2))
        out.append((f"q{quality}_bigquant1", with_quant(base, 1, big), fl, 2))
        out.append((f"q{quality}_bigquant1_bad0", with_quant(bad_in(base, 0), 1, big), fl, 2))
        out.append((f"q{quality}_ones1_bad0", with_quant(bad_in(base, 0), 1, ones), fl, 2))
        out.append((f"q{quality}_ones1_bad2", with_quant(bad_in(base, 2), 1, ones), fl, 2))
        out.append((f"q{quality}_oneszero1_bad0", with_quant(bad_in(base, 0), 1, ones_zero), fl, 2))
    return out


def reference_run(reference, j, flags, niter):
    kw = {k: j[k] for k in ("hsamp", "vsamp", "colorspace", "image_size")}
    return reference.do_quantsmooth(j["coefs"], j["quants"], flags, niter, **kw)


def test_range_check_stop_equals_the_reference(tq, reference, synth, pkg):
    for name, j, flags, niter in stop_cases(synth, pkg.flags_for_quality):
        want = reference_run(reference, j, flags, niter)
        assert want["ret"] == 1, name
        kw = {k: j[k] for k in ("hsamp", "vsamp", "colorspace", "image_size")}
        got = run_device(tq, j["coefs"], j["quants"], flags, niter, **kw)
        assert_same_result(got, want, name)


# ---- full-size images against the job layer -----------------------------------------------------------------------

@pytest.mark.parametrize("quality", [3, 4])
def test_8192_luma_equals_the_job_layer(tq, hip, big_plane, pkg, quality):
    coef, quant = big_plane
    flags = pkg.flags_for_quality(quality)
    want = hip.do_quantsmooth([coef], [quant], flags, 3)
    got = run_device(tq, [coef], [quant], flags, 3)
    assert_same_result(got, want, f"8192^2 q{quality}")


@pytest.fixture(scope="module")
def hd420(synth):
    y = synth.synth_ycc(1920, 1080, 2, 2, quality=50, seed=5)
    return dict(coefs=y["coefs"], quants=y["quants"], hsamp=y["hsamp"], vsamp=y["vsamp"], colorspace=3,
                image_size=(1920, 1080))


@pytest.mark.parametrize("quality", [3, 5, 6])
def test_1080p_420_equals_the_job_layer(tq, hip, hd420, pkg, quality):
    j = hd420
    kw = {k: j[k] for k in ("hsamp", "vsamp", "colorspace", "image_size")}
    flags = pkg.flags_for_quality(quality)
    want = hip.do_quantsmooth(j["coefs"], j["quants"], flags, 3, **kw)
    got = run_device(tq, j["coefs"], j["quants"], flags, 3, **kw)
    assert_same_result(got, want, f"1080p 4:2:0 q{quality}")


# ---- graph capture ------------------------------------------------------------------------------------------------

def capture_inputs(synth):
    """two different 1080p 4:2:0 inputs with the same geometry and tables"""
    a = synth.synth_ycc(1920, 1080, 2, 2, quality=50, seed=31)
    b = synth.synth_ycc(1920, 1080, 2, 2, quality=50, seed=32)
    assert all(np.array_equal(p, q) for p, q in zip(a["quants"], b["quants"]))
    return [dict(coefs=x["coefs"], quants=x["quants"], hsamp=x["hsamp"], vsamp=x["vsamp"], colorspace=3,
                 image_size=(1920, 1080)) for x in (a, b)]


@pytest.mark.parametrize("quality", [3, 6])
def test_single_stream_graph_capture_replays_exactly(tq, hip, reference, synth, pkg, quality):
    """one job captured on one stream (a linear graph: the route uses no other stream, no host synchronisation, no
    allocation outside torch's graph pool); four replays with different inputs copied into the static tensors: two
    clean ones, one whose range check trips, a clean one again.  Then a niter-0 job replayed: its stop comes from
    the fix-up kernel inside the graph"""
    torch, torch_qs = tq
    flags, niter = pkg.flags_for_quality(quality), 2
    inputs = capture_inputs(synth)
    bad = dict(inputs[0], coefs=[c.copy() for c in inputs[0]["coefs"]])
    bad["coefs"][0][1, 2, 0] = 0x7ff                         # 0x7ff * q >= 0x800 for any q >= 2
    kw = {k: inputs[0][k] for k in ("hsamp", "vsamp", "colorspace", "image_size")}
    static = [torch.from_numpy(c).cuda() for c in inputs[0]["coefs"]]
    warm = torch_qs.quantsmooth_(static, inputs[0]["quants"], flags, niter, **kw)     # prepares the workspace
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = torch_qs.quantsmooth_(static, inputs[0]["quants"], flags, niter, workspace=warm["workspace"], **kw)
    for r, x in enumerate(inputs + [bad, inputs[1]]):
        for t, c in zip(static, x["coefs"]):
            t.copy_(torch.from_numpy(c))
        g.replay()
        torch.cuda.synchronize()
        got = _result(torch, static, res, kw)
        assert got["ret"] == (1 if r == 2 else 0), r
        want = hip.do_quantsmooth(x["coefs"], x["quants"], flags, niter, **kw)
        assert_same_result(got, want, f"graph replay {r} q{quality}")
        if r < 2:
            assert_same_result(got, reference_run(reference, x, flags, niter), f"graph replay {r} q{quality}")

    warm = torch_qs.quantsmooth_(static, inputs[0]["quants"], flags, 0, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = torch_qs.quantsmooth_(static, inputs[0]["quants"], flags, 0, workspace=warm["workspace"], **kw)
    x = inputs[1]
    for t, c in zip(static, x["coefs"]):
        t.copy_(torch.from_numpy(c))
    res["stop"].fill_(7)
    g.replay()
    torch.cuda.synchronize()
    got = _result(torch, static, res, kw)
    assert got["ret"] == 0
    assert_same_result(got, hip.do_quantsmooth(x["coefs"], x["quants"], flags, 0, **kw), f"graph replay niter 0 q{quality}")
