#!/usr/bin/env python3
"""Randomised GPU-vs-oracle campaign: larger images than the test suite affords, every
flag combination, extreme blocks, sparse planes, single calls and batches.

The scalar oracle is the slow side, so the campaign is split: `gen` runs ONLY the oracle
(anywhere, no GPU) and writes one JSON line per job with the hashes of the expected
outputs; `run` regenerates the same seeded inputs on the GPU box, runs the product and
compares hashes -- hundreds of jobs in a minute of GPU time.

    python tools/fuzz_gpu.py gen <file.jsonl> <trials> [seed=1] [generator=trials]   # CPU only
    python tools/fuzz_gpu.py run <file.jsonl>                                         # GPU box

Generators (GENERATORS): `trials` (trial_jobs, tests/golden/fuzz_s2.jsonl) and `stops` (stop_trial_jobs: jobs built
to trip the range check, tests/golden/fuzz_stops.jsonl).  A record names its generator under "gen"; records without
the key come from `trials`.
"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import jpegqs_pkg  # noqa: E402
from helpers import inject_extreme_blocks  # noqa: E402

import hashlib  # noqa: E402
import json  # noqa: E402

mode, path = sys.argv[1], Path(sys.argv[2])
pkg = jpegqs_pkg.load()
synth = pkg.synth
LAYOUTS = [(1, 1), (2, 2), (2, 1), (1, 2), (4, 1), (2, 2), (2, 2)]


def make_job(rng, trial, big):
    hi = 1400 if big else 260
    w, h = int(rng.integers(8, hi)), int(rng.integers(8, hi * 3 // 4))
    qual = int(rng.choice([1, 5, 20, 35, 50, 65, 80, 95, 100]))
    if rng.random() < 0.3:
        coef, quant = synth.synth_gray(w, h, qual, seed=trial)
        if rng.random() < 0.3:
            coef = (coef * (rng.random(coef.shape[:2]) < 0.3)[:, :, None]).astype(np.int16)
        j = dict(coefs=[coef], quants=[quant])
        desc = f"gray {w}x{h} q{qual}"
    else:
        hs, vs = LAYOUTS[int(rng.integers(0, len(LAYOUTS)))]
        y = synth.synth_ycc(w, h, hs, vs, quality=qual, seed=trial)
        if rng.random() < 0.5 and qual >= 20:
            y = inject_extreme_blocks(y, seed=trial)
        j = dict(coefs=y["coefs"], quants=y["quants"], hsamp=y["hsamp"], vsamp=y["vsamp"], colorspace=3, image_size=(w, h))
        desc = f"ycc {w}x{h} {hs}x{vs} q{qual}"
    return j, desc


def digest(res):
    h = lambda x: hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]
    return dict(ret=int(res["ret"]), up=bool(res["up"]), samp=[int(res["hsamp0"]), int(res["vsamp0"])],
                coefs=[[list(c.shape), h(c)] for c in res["coefs"]],
                quants=[None if q is None else h(q) for q in res["quants"]])


def trial_jobs(seed0, trial):
    """the jobs of one trial: ([(job, desc)], flags, niter, is_batch) -- a pure function of the seeds"""
    rng = np.random.default_rng([seed0, trial])
    flags = int(rng.integers(0, 128))
    niter = int(rng.choice([0, 1, 2, 3, 3, 3, 5]))
    if trial % 4 == 0:                                   # a batch of small / medium jobs
        n = int(rng.integers(2, 12))
        return [make_job(rng, trial * 100 + k, big=False) for k in range(n)], flags, niter, True
    return [make_job(rng, trial * 100, big=trial % 4 == 1)], flags, niter, False


def kwargs(j):
    return {k: j[k] for k in ("hsamp", "vsamp", "colorspace", "image_size") if k in j}


# ---- the stop corpus: jobs built to trip the reference's range check (quantsmooth.h:2596-2610) ------------------------
#
# A trip plants one product coef * quantval outside [-0x800, 0x7ff] in a component; a near miss one just inside it (or
# a huge coefficient under a zero quantiser, whose product is 0).  `desc` names everything planted, component by
# component, in a fixed vocabulary the tests count: "trip c<ci>:<pos>[<index>]=<kind>", "near c<ci>:...", "table
# c<ci>=<kind>", "notable c<ci>", "extreme", "split64" / "split128" (a tripping job whose precheck records straddle a
# chunk of QS_DEVB_CHUNK = 64 records, see csrc/qs_device_job.h), "rec<first record>".

STOP_PRODUCTS = {"p800": 0x800, "m801": -0x801}            # exact boundary trips ...
NEAR_PRODUCTS = {"p7ff": 0x7ff, "m800": -0x800}            # ... and exact near misses


def _divisor_for(value, q):
    """the largest quantiser up to q (at least 1) that divides `value`: lowering a quantiser never makes the other
    coefficients under it trip"""
    return max(d for d in range(1, max(q, 1) + 1) if value % d == 0)


def _plant(rng, coefs, quants, ci, pos, kind, used):
    """writes one coefficient (and where needed its quantiser) of component ci -> the desc token.  used: the
    (component, index) pairs planted so far, whose quantisers stay as they are"""
    c, q = coefs[ci], quants[ci]
    hb, wb = c.shape[:2]
    by, bx = {"first": (0, 0), "last": (hb - 1, wb - 1)}.get(pos, (int(rng.integers(0, hb)), int(rng.integers(0, wb))))
    e = int(rng.integers(0, 64))
    while (ci, e) in used:
        e = (e + 1) % 64
    used.add((ci, e))
    if kind in STOP_PRODUCTS or kind in NEAR_PRODUCTS:
        v = {**STOP_PRODUCTS, **NEAR_PRODUCTS}[kind]
        q[e] = _divisor_for(abs(v), int(q[e]))
        c[by, bx, e] = v // int(q[e])
    elif kind == "zeroq":                                    # coefficient +-32767, quantiser 0: the product is 0
        q[e] = 0
        c[by, bx, e] = 32767 if rng.integers(0, 2) else -32767
    elif kind == "large":                                    # 0x800 < |product| <= 32767
        q[e] = max(1, min(int(q[e]), 64))
        lo, hi = -(-0x801 // int(q[e])), 32767 // int(q[e])
        c[by, bx, e] = int(rng.integers(lo, hi + 1)) * (1 if rng.integers(0, 2) else -1)
    else:                                                    # "wrap": |product| > 32767, int16 wraps before the clamp
        q[e] = max(2, min(int(q[e]), 64))
        lo = 32768 // int(q[e]) + 1
        c[by, bx, e] = int(rng.integers(lo, 32768)) * (1 if rng.integers(0, 2) else -1)
    return f"c{ci}:{pos}[{e}]={kind}"


def _stop_base(rng, seed, flags, big, tiny):
    """an unplanted job: gray, YCbCr in a layout of LAYOUTS, RGB or four components -> (job, desc)"""
    hi = 1400 if big else 64 if tiny else 300
    w, h = int(rng.integers(8, hi)), int(rng.integers(8, max(9, hi * 3 // 4)))
    qual = int(rng.choice([5, 20, 35, 50, 65, 80, 95]))
    shape = rng.choice(["gray", "ycc", "ycc", "ycc", "rgb", "cmyk"] if not tiny else ["gray", "ycc", "ycc", "ycc", "cmyk",
                                                                                   "cmyk", "cmyk", "cmyk"])
    if shape == "gray":
        coef, quant = synth.synth_gray(w, h, qual, seed=seed)
        return dict(coefs=[coef], quants=[quant]), f"gray {w}x{h} q{qual}"
    if shape == "cmyk":
        planes = [synth.synth_gray(w, h, max(1, qual - 10 * k), seed=seed + k) for k in range(4)]
        return (dict(coefs=[p[0] for p in planes], quants=[p[1] for p in planes], hsamp=[1] * 4, vsamp=[1] * 4,
                     colorspace=4, image_size=(w, h)), f"cmyk {w}x{h} q{qual}")
    hs, vs = (1, 1) if shape == "rgb" else LAYOUTS[int(rng.integers(0, len(LAYOUTS)))]
    y = synth.synth_ycc(w, h, hs, vs, quality=qual, seed=seed)
    j = dict(coefs=y["coefs"], quants=y["quants"], hsamp=y["hsamp"], vsamp=y["vsamp"], colorspace=2 if shape == "rgb" else 3,
             image_size=(w, h))
    desc = f"{shape} {w}x{h} {hs}x{vs} q{qual}"
    if shape == "ycc" and rng.random() < 0.5:
        j = inject_extreme_blocks(j, seed=seed)
        desc += " extreme"
    return j, desc


def make_stop_job(rng, seed, flags, *, big=False, tiny=False, trips=None, plain_tables=False):
    """one job of the stop corpus -> (job, desc).  trips: the components to trip (None: drawn here)"""
    j, desc = _stop_base(rng, seed, flags, big, tiny)
    return plant_stop_job(rng, j, desc, flags, trips, plain_tables)


def plant_stop_job(rng, j, desc, flags, trips=None, plain_tables=False):
    n = len(j["coefs"])
    coefs = [np.ascontiguousarray(c).copy() for c in j["coefs"]]
    quants = [np.asarray(q, dtype=np.uint16).copy() for q in j["quants"]]
    toks, used = [], set()
    if trips is None:
        r = rng.random()
        ntrip = 0 if r < 0.12 else 1 if r < 0.55 else 2 if r < 0.85 else 3
        trips = sorted(int(x) for x in rng.choice(n, size=min(ntrip, n), replace=False))
        if trips and rng.random() < 0.25:                    # bias towards late first trips (k = 2, 3)
            trips = [n - 1]
    tab_ci = None
    if not plain_tables and rng.random() < 0.45:             # one component's table replaced
        kind = str(rng.choice(["ones", "oneszero", "zeros", "bigq", "bigq"]))
        others = [ci for ci in range(n) if ci not in trips]
        if kind == "bigq" and others:
            tab_ci = int(rng.choice(others))                 # before or after the first tripping component
            quants[tab_ci][int(rng.integers(0, 64))] = int(rng.integers(0x800, 0x10000))
        elif kind != "bigq":
            tab_ci = int(rng.integers(0, n))
            if kind == "ones":
                quants[tab_ci][:] = 1
            elif kind == "oneszero":
                quants[tab_ci][:] = 1
                quants[tab_ci][int(rng.integers(0, 64))] = 0
            else:
                quants[tab_ci][rng.random(64) < 0.2] = 0
        if tab_ci is not None:
            toks.append(f"table c{tab_ci}={kind}")
    for ci in trips:
        pos = str(rng.choice(["first", "last", "rand"]))
        kind = str(rng.choice(["p800", "m801", "large", "wrap"]))
        toks.append("trip " + _plant(rng, coefs, quants, ci, pos, kind, used))
    for _ in range(int(rng.integers(0, 3)) if trips else int(rng.integers(1, 4))):
        ci = int(rng.integers(0, n))
        pos = str(rng.choice(["first", "last", "rand"]))
        toks.append("near " + _plant(rng, coefs, quants, ci, pos, str(rng.choice(["p7ff", "m800", "zeroq"])), used))
    if not plain_tables and n > 1 and rng.random() < 0.1:   # a component without a table
        ycc_up = j.get("colorspace") == 3 and flags & 4
        cands = [0] if ycc_up else list(range(n))            # (UPSAMPLE_UV and a missing chroma table: the reference
        ci = int(rng.choice(cands))                          # dereferences the missing replacement array)
        quants[ci] = None
        toks.append(f"notable c{ci}")
    j = dict(j, coefs=coefs, quants=quants)
    return j, " | ".join([desc] + toks)


def stop_trial_jobs(seed0, trial):
    """the jobs of one trial of the stop corpus: ([(job, desc)], flags, niter, is_batch) -- a pure function of the seeds"""
    rng = np.random.default_rng([seed0, trial, 0x57])
    flags = pkg.flags_for_quality(int(rng.integers(0, 7))) if trial % 2 else int(rng.integers(0, 128))
    niter = int(rng.choice([0, 1, 2, 3, 5]))
    seed = trial * 100
    if trial % 24 == 6:
        # 30-50 small jobs with ordinary tables and niter >= 1 (niter 0 without UPSAMPLE_UV has no records): every
        # component has one precheck record, so job k's records start at the sum of the earlier jobs' components.
        # Trips in about half the jobs before record 64 and three in four after it, and in the first component past the
        # boundary of a job that straddles one
        niter = max(niter, 1)
        made, rec = [], 0
        for k in range(int(rng.integers(40, 51))):                 # (3.25 components a job on average)
            j, d = _stop_base(rng, seed + k, flags, False, True)
            nc = len(j["coefs"])
            split = 64 if rec < 64 < rec + nc else 128 if rec < 128 < rec + nc else 0
            if split:
                trips = [split - rec]
                d += f" | split{split}"
            else:
                trips = [int(rng.integers(0, nc))] if rng.random() < (0.75 if rec >= 64 else 0.5) else []
            j, d = plant_stop_job(rng, j, d, flags, trips, plain_tables=True)
            made.append((j, d + f" | rec{rec}"))
            rec += nc
        return made, flags, niter, True
    if trial % 4 == 0:                                       # a batch of 2-12 jobs, some tripping, some clean
        n = int(rng.integers(2, 13))
        made = [make_stop_job(rng, seed + k, flags, trips=None if rng.random() < 0.8 else []) for k in range(n)]
        return made, flags, niter, True
    return [make_stop_job(rng, seed, flags, big=trial % 8 == 1)], flags, niter, False


GENERATORS = {"trials": trial_jobs, "stops": stop_trial_jobs}


def jobs_of(rec):
    """the jobs of a corpus record; records without a "gen" key come from trial_jobs"""
    return GENERATORS[rec.get("gen", "trials")](rec["seed0"], rec["trial"])


# Records of the `trials` corpus hold every job's desc and digest in full.  The others are kept small: one hash of the
# descs (they come back from the seeds), and per job the short form of its digest.
def short_digest(d):
    """'<ret><up><hsamp0><vsamp0>:<hash of the whole digest>', e.g. '1022:9c1f0e2ab3'"""
    h = hashlib.sha1(json.dumps(d, sort_keys=True).encode()).hexdigest()[:10]
    return f"{d['ret']}{int(d['up'])}{d['samp'][0]}{d['samp'][1]}:{h}"


def descs_hash(descs):
    return hashlib.sha1("\n".join(descs).encode()).hexdigest()[:10]


def record(gen, seed0, trial, flags, niter, is_batch, descs, digests):
    if gen == "trials":
        return dict(seed0=seed0, trial=trial, flags=flags, niter=niter, batch=is_batch, desc=descs, expect=digests)
    return dict(gen=gen, seed0=seed0, trial=trial, flags=flags, niter=niter, batch=is_batch, descs=descs_hash(descs),
                expect=[short_digest(d) for d in digests])


def same_trial(rec, flags, niter, is_batch, descs):
    """the generator still draws the trial the record was made from"""
    return ((flags, niter, is_batch) == (rec["flags"], rec["niter"], rec["batch"]) and
            (descs == rec["desc"] if "desc" in rec else descs_hash(descs) == rec["descs"]))


def matches(d, want):
    """a digest against a record's expectation, full or short"""
    return (d if isinstance(want, dict) else short_digest(d)) == want


if mode == "gen":
    from oracle.oracle import Oracle, RecordedReference, Reference, have_ref   # the replay side (`run`) never touches the oracle
    # FUZZ_TRUTH=ref: the expected hashes come from the COMPILED, UNMODIFIED reference (oracle/_ref/libqsref_none.so) instead
    # of the plain-C port -- slower, and how the committed corpus was re-derived in round 6 (identical file: the port is
    # pinned to the reference on CPU, this shows it on the corpus itself).  Without oracle/_ref: its recorded results
    # (the port, checked job by job against them); QS_RECORD_REFERENCE=1 records them from oracle/_ref.
    import os
    oracle = Oracle()
    if os.environ.get("FUZZ_TRUTH") == "ref":
        if not have_ref("none"):
            oracle = RecordedReference()
        elif os.environ.get("QS_RECORD_REFERENCE") == "1":
            oracle = RecordedReference(live=Reference("none"))
        else:
            oracle = Reference("none")
    print("gen: truth =", type(oracle).__name__)
    ntrials = int(sys.argv[3]); seed0 = int(sys.argv[4]) if len(sys.argv) > 4 else 1
    gen = sys.argv[5] if len(sys.argv) > 5 else "trials"
    t0 = time.time()
    with open(path, "w") as f:
        for trial in range(1, ntrials + 1):
            made, flags, niter, is_batch = GENERATORS[gen](seed0, trial)
            exp = [digest(oracle.do_quantsmooth(j["coefs"], j["quants"], flags, niter, threads=0, **kwargs(j))) for j, _ in made]
            rec = record(gen, seed0, trial, flags, niter, is_batch, [d for _, d in made], exp)
            f.write((json.dumps(rec) if gen == "trials" else json.dumps(rec, separators=(",", ":"))) + "\n")
            f.flush()
    if isinstance(oracle, RecordedReference) and oracle.live is not None:
        oracle.save()
    print(f"gen: {ntrials} trials in {time.time() - t0:.0f} s -> {path}")
    sys.exit(0)

hip = pkg.HipQS()
fails = jobs_done = blocks = trials = 0
t0 = time.time()
for line in open(path):
    rec = json.loads(line)
    made, flags, niter, is_batch = jobs_of(rec)
    assert same_trial(rec, flags, niter, is_batch, [d for _, d in made]), "generator drift"
    if is_batch:
        got = hip.do_quantsmooth_batch([m[0] for m in made], flags, niter)
    else:
        j = made[0][0]
        got = [hip.do_quantsmooth(j["coefs"], j["quants"], flags, niter, **kwargs(j))]
    trials += 1
    for (j, desc), g, want in zip(made, got, rec["expect"]):
        jobs_done += 1
        blocks += sum(c.shape[0] * c.shape[1] for c in j["coefs"])
        if not matches(digest(g), want):
            fails += 1
            print(f"FAIL seed=({rec['seed0']},{rec['trial']}) {'batch ' if is_batch else ''}{desc} flags={flags} niter={niter}", flush=True)
print(f"fuzz: {trials} trials, {jobs_done} jobs, {blocks} blocks, {fails} failures, {time.time() - t0:.0f} s", flush=True)
sys.exit(1 if fails else 0)
