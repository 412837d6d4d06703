"""The luma recovery kernel's rebalance epilogue (csrc/qs_smooth_kernel.inc) handles two coefficients per LDS dword with
24-bit multiplies and applies only the outward bound of each interval (qs_rebalance_outward, csrc/qs_devfn.h;
tests/test_rebalance_lemma.py has the arithmetic), and the coefficient update collects the two rebalance sums in
registers, one anti-diagonal at a time, before they go to the 64-bit sums in LDS.  Everything here is bit-exact against
the compiled reference (oracle/_ref/libqsref_none.so; the plain-C port where it did not travel), never against another
run of the kernel.

Shape: 9 x 8 blocks -- one full wave and one with 8 live lanes.  Each case runs three chained recovery launches (the
first is the niter = 1 result, every launch is compared), with flags 0 and DIAGONALS, once in a process with QS_HIP_DP=0
(every launch takes the block-per-lane kernel) and once with the launcher's choice (the small-plane kernel).  The cases
a job can hold also run as whole jobs (niter 1 and 3) through the plane-set launches, eager and deferred.

Each case states on the host, from the reference's own results without the rebalance step, that it reaches the regime
it is there for (which lanes rebalance, how large mul is, how large the sums are)."""
import numpy as np
import pytest

import plane_cases as pc

pytestmark = pytest.mark.gpu

HB, WB = 8, 9


def _orig(c, q):
    """nearest multiple of the quantiser, ties away from zero (exact below 0x4000)"""
    c, q = c.astype(np.int64), pc.eff(q).astype(np.int64)
    return np.sign(c) * ((np.abs(c) + (q >> 1)) // q) * q


def rebalance_muls(ref, q, c):
    """per block: (m0, m1, mul) of the reference's rebalance step (:1823-1835) for one launch on c -- the sums over the
    walk's results, which are the reference's results without the rebalance step; mul = 0 where m1 <= m0"""
    v = pc.pass_b_expected_plain(ref, q, c, pc.F_NOREB).astype(np.int64)
    orig = _orig(v, q)
    m0, m1 = (v * orig)[..., 1:].sum(-1).ravel(), (orig * orig)[..., 1:].sum(-1).ravel()
    mul = np.zeros_like(m0)
    on = m1 > m0
    mul[on] = ((m1[on] << 13) + (m0[on] >> 1)) // m0[on]
    return m0, m1, mul


def parity_table():
    """even and odd quantisers next to each other (d0 != d1 for the even ones), entries of 1 and of 255"""
    t = np.array([8, 1, 2, 3, 4, 5, 255, 254] * 8, np.uint16)
    t[[9, 27, 63]] = 1
    t[[10, 17, 62]] = 255
    return t


def case_parity(ref):
    q = parity_table()
    c = pc.coefficients(np.random.default_rng(81), q, HB, WB, ("random", "ends", "saturate", "sparse"))
    _, _, mul = rebalance_muls(ref, q, c)
    assert (mul[:64] > 0).sum() >= 16 and ((q & 1) == 0).sum() >= 16 and (q == 1).sum() >= 8 and (q == 255).sum() >= 8
    return q, c


def case_mixed_wave(ref):
    """lanes that rebalance next to lanes that do not (blocks without AC energy: m0 = m1 = 0) in ONE wave"""
    q = pc.STD_LUMA.copy()
    c = pc.coefficients(np.random.default_rng(82), q, HB, WB, ("random",))
    flat = (np.arange(HB * WB) % 3 == 1).reshape(HB, WB)
    c[flat, 1:] = 0
    c[flat, 0] = (c[flat, 0] // 16) * 16            # (DC: an exact multiple of its quantiser)
    m0, m1, mul = rebalance_muls(ref, q, c)
    assert (mul[:64] > 0).sum() >= 8 and (m1[:64] <= m0[:64]).sum() >= 8
    return q, c


def case_ratio_just_above_one(ref):
    """a few hundred in each of eight low frequencies (no pixel saturates) under quantisers of 2 and 3: where the walk
    moves anything it moves it by 1 in a few hundred, and only some of the eight -- mul lands just above 8192"""
    q = np.where(np.arange(64) & 1, 3, 2).astype(np.uint16)
    rng = np.random.default_rng(83)
    c = np.zeros((HB, WB, 64), np.int64)
    for k in (1, 2, 3, 8, 9, 10, 16, 17):
        c[..., k] = rng.choice((-1, 1), (HB, WB)) * 150 * rng.integers(1, 3, (HB, WB))
    c = ((c // q) * q).astype(np.int16)
    _, _, mul = rebalance_muls(ref, q, c)
    assert ((mul > 8192) & (mul <= 8200)).sum() >= 4, sorted(set(mul.tolist()))[:8]
    return q, c


def case_large_ratio(ref):
    """a few single multiples of a large quantiser in empty blocks: the walk pulls each to the inner end of its interval"""
    q = np.full(64, 255, np.uint16)
    rng = np.random.default_rng(84)
    m = rng.choice((-1, 0, 1), (HB, WB, 64), p=(0.02, 0.96, 0.02))
    c = (m * 255).astype(np.int16)
    c[..., 0] = 0
    _, _, mul = rebalance_muls(ref, q, c)
    assert (mul > 12000).sum() >= 8, int(mul.max())
    return q, c


def case_signs_and_zeros(ref):
    q = pc.table("camera")
    c = pc.coefficients(np.random.default_rng(85), q, HB, WB, ("sparse", "random", "ends"))
    _, _, mul = rebalance_muls(ref, q, c)
    assert (mul > 0).sum() >= 8 and (c < 0).sum() >= 500 and (c[..., 1:] == 0).sum() >= 500
    return q, c


def _all_1fff():
    sign = np.where((np.arange(64)[None, None, :] + np.arange(WB)[None, :, None] + np.arange(HB)[:, None, None]) & 1, -1, 1)
    c = (sign * 0x1fff).astype(np.int16)
    c[..., 0] = 0
    return c


def case_sums_quantiser_one(ref):
    """every AC coefficient at +-0x1fff, quantiser 1: both sums are 63 * 0x1fff^2 > 2^31"""
    q, c = np.ones(64, np.uint16), _all_1fff()
    m0, m1, _ = rebalance_muls(ref, q, c)
    assert (m1 > 2**31).all() and (m1 < 2**32).all() and np.array_equal(m0, m1)
    return q, c


def case_sums_large_quantiser(ref):
    """the same magnitudes under quantisers near 0x7ff: orig = +-4 q, sums beyond 2^31"""
    q = np.where(np.arange(64) & 1, 0x7ff, 0x7fe).astype(np.uint16)
    c = _all_1fff()
    m0, m1, mul = rebalance_muls(ref, q, c)
    assert (m1 > 2**31).all() and (m0 > 2**31).sum() >= 8 and (mul > 0).sum() >= 8
    return q, c


def case_reference_range_wave(ref):
    """one coefficient >= 0x2000 in the first wave: that wave follows the reference to the letter, the second does not"""
    q = pc.STD_LUMA.copy()
    c = pc.coefficients(np.random.default_rng(87), q, HB, WB, ("random", "ends"))
    c[0, 3, 5] = 0x2345
    assert (np.abs(c.reshape(-1, 64)[64:].astype(np.int32)) < 0x2000).all()
    _, _, mul = rebalance_muls(ref, q, c)
    assert (mul[:64] > 0).sum() >= 8 and (mul[64:] > 0).sum() >= 2
    return q, c


CASES = {f.__name__: f for f in (case_parity, case_mixed_wave, case_ratio_just_above_one, case_large_ratio, case_signs_and_zeros,
                                 case_sums_quantiser_one, case_sums_large_quantiser, case_reference_range_wave)}


def check_block_level(pkg, gpu, ref, torch):
    """three chained launches per case and flags: launch n + 1 starts from the reference's result of launch n"""
    import test_gpu_resident_differences as R
    n = 0
    for name, make in CASES.items():
        q, c0 = make(ref)
        for flags in (0, pc.F_DIAG):
            c = c0
            for it in range(3):
                c = R._block_level(gpu, torch, ref, q, c, flags, (0,), f"{name} flags={flags} launch {it + 1}")
                n += 1
    return n


def job_inputs(pkg):
    """what a job can hold: quantised planes of sensor noise, and of noise with every third block constant"""
    from test_gpu_resident_differences import _quantised
    ins = []
    for quant, seed in ((parity_table(), 91), (np.full(64, 255, np.uint16), 92)):
        px = pkg.synth.synth_pixels(WB * 8, HB * 8, seed)
        for b in range(1, HB * WB, 3):
            by, bx = divmod(b, WB)
            px[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = 100 + b
        ins.append((np.ascontiguousarray(pkg.synth.quantise_plane(px, quant), np.int16), quant))
    ins.append((_quantised(pkg, "noise", WB, HB, pc.table("camera"), 93), pc.table("camera")))
    return ins


def check_jobs(pkg, gpu, ref, torch):
    """whole jobs through the plane-set launches: niter 1 and 3, flags 0 and DIAGONALS, eager and deferred dequantisation"""
    import test_gpu_deferred_dequant as D
    import test_gpu_resident_differences as R
    n = 0
    ins = job_inputs(pkg)
    for flags in (0, pc.F_DIAG):
        for niter in (1, 3):
            n += R._run_job(D, gpu, torch, ref, ins, [False, True, False], flags, niter, f"set of three, flags {flags}, niter {niter}")
            n += R._run_job(D, gpu, torch, ref, ins[:1], [True], flags, niter, f"parity table alone, flags {flags}, niter {niter}")
    return n


CHECKS = {f.__name__: f for f in (check_block_level, check_jobs)}


@pytest.mark.parametrize("dp", ("block-per-lane", "launcher"))
@pytest.mark.parametrize("check", sorted(CHECKS))
def test_rebalance_epilogue(gpu, check, dp):
    from test_gpu_parity import _run_py
    code = rf'''
import sys, torch
sys.path.insert(0, "tests")
import jpegqs_pkg
import test_gpu_rebalance_epilogue as T
from oracle import oracle as om
ref = om.Reference("none") if om.have_ref("none") else om.Oracle()
pkg = jpegqs_pkg.load()
gpu = pkg.HipQS()
print("ok", T.CHECKS["{check}"](pkg, gpu, ref, torch))
'''
    out = _run_py(code, {"QS_HIP_DP": "0"} if dp == "block-per-lane" else {}, timeout=300)
    assert "ok" in out
