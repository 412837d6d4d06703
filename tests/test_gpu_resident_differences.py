"""The luma recovery kernel (csrc/qs_smooth_kernel.inc, one block per lane, non-DIAGONALS) holds its 112 interior and 32
edge pixel differences in registers between refreshes and no pixels; the neighbour pixels, the rebalance sums and one
stash slot live in LDS behind the coefficient columns.  Everything here is bit-exact against the compiled reference
(oracle/_ref/libqsref_none.so; the plain-C port where it did not travel) -- never against another run of the kernel --
and runs in a fresh process with QS_HIP_DP=0 (read once per process), so that every launch takes the block-per-lane
kernel, whatever the plane's size.

Shapes (wblk x hblk): 1x1; 5x3; 8x9 (72 blocks: a second wave with 8 live lanes); 65x2 (left and right neighbours in
another wave).  Every plane is small enough for every block row or column to touch the plane border somewhere, so all
four groups of edge differences matter.

Content: sensor noise (every refresh runs); a constant and a gently shaded image (whole waves skip refreshes: the
differences and the stash bookkeeping must survive them); reachable extremes of a table with entries of 1 and of
0x7ff; coefficients over the whole int16 range (quotients past int32 and 0 / 0: the NaN -> INT_MIN conversion)."""
import numpy as np
import pytest

import plane_cases as pc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (8, 9), (65, 2)]        # (wblk, hblk)
CONTENTS = ("noise", "constant", "shaded", "checker")


def _pixels(pkg, kind, wb, hb, seed):
    w, h = wb * 8, hb * 8
    if kind == "noise":
        return pkg.synth.synth_pixels(w, h, seed)
    if kind == "checker":     # 0 / 255 pixel checkerboard: every difference is 0 or 255 >= 2q, denominators of 0 (0 / 0 = NaN) within reach of a job
        x, y = np.arange(w)[None, :], np.arange(h)[:, None]
        return (((x + y) & 1) * 255).astype(np.uint8)
    if kind == "constant":
        return np.full((h, w), 137, np.uint8)
    if kind == "shaded":      # one grey level every four / seven pixels: differences of 0 and 1
        x, y = np.arange(w)[None, :], np.arange(h)[:, None]
        return (90 + x // 4 + y // 7).clip(0, 255).astype(np.uint8)
    raise KeyError(kind)


def _quantised(pkg, kind, wb, hb, quant, seed):
    coef = pkg.synth.quantise_plane(_pixels(pkg, kind, wb, hb, seed), np.asarray(quant, np.uint16))
    assert coef.shape == (hb, wb, 64)
    return np.ascontiguousarray(coef, np.int16)


def _same(got, want, what):
    msg = pc.first_diff(np.asarray(got), np.asarray(want), what)
    assert msg is None, msg


def _run_job(D, gpu, torch, ref, planes_in, defer, flags, niter, what):
    """pass A + niter recovery launches over the planes (tests/test_gpu_deferred_dequant._run_set: next-plane writes in
    every launch but the last, the +-1023 clamp in the last) against the reference's whole job, plane by plane; after
    the first launch the fused next plane against the reference's IDCT of that launch's coefficients"""
    planes = [D.Plane(gpu, torch, c, q, flags) for c, q in planes_in]

    def after_first():
        if niter > 1:
            for p in planes:
                _same(p.rows(p.plane), pc.ref_plane(ref, p.coef.cpu().numpy()), f"{what}: next plane of the first launch, plane {p.wb}x{p.hb}")
    D._run_set(gpu, torch, planes, defer, flags, niter, None, after_first)
    for p, (c, q) in zip(planes, planes_in):
        want = ref.do_quantsmooth([c], [q], flags, niter)
        assert want["ret"] == 0 and int(p.status.item()) == 0
        _same(p.coef.cpu().numpy(), want["coefs"][0], f"{what}: plane {p.wb}x{p.hb} vs the reference")
    return len(planes)


def check_contents(pkg, gpu, ref, torch):
    """every shape x content x rebalance on / off x niter 1 / 3, the eager and the deferred-dequantisation route"""
    import test_gpu_deferred_dequant as D
    quant = pkg.synth.quality_table(pkg.synth.STD_LUMA, 50)
    n = 0
    for wb, hb in SHAPES:
        for kind in CONTENTS:
            coef = _quantised(pkg, kind, wb, hb, quant, 300 + wb)
            for flags in (0, pc.F_NOREB):
                for niter in (1, 3):
                    for defer in (False, True):
                        n += _run_job(D, gpu, torch, ref, [(coef, quant)], [defer], flags, niter,
                                      f"{wb}x{hb} blocks, {kind}, flags {flags}, niter {niter}, {'deferred' if defer else 'eager'}")
    return n


def check_set_launch(pkg, gpu, ref, torch):
    """three planes with three quantiser tables in ONE launch per iteration -- one table with entries of 1, whose
    coefficients skip their term streams and still feed the rebalance sums in LDS; one plane of constant content next
    to two of noise; only the first and the last defer their dequantisation"""
    import test_gpu_deferred_dequant as D
    tables = [pkg.synth.quality_table(pkg.synth.STD_LUMA, 50), pc.table("camera"), pkg.synth.quality_table(pkg.synth.STD_LUMA, 20)]
    assert (tables[1] == 1).sum() >= 6
    ins = [(_quantised(pkg, kind, wb, hb, q, 11 + wb), np.asarray(q, np.uint16))
           for (wb, hb), kind, q in zip(((5, 3), (8, 9), (65, 2)), ("noise", "noise", "constant"), tables)]
    n = 0
    for flags in (0, pc.F_NOREB):
        for niter in (1, 3):
            n += _run_job(D, gpu, torch, ref, ins, [True, False, True], flags, niter, f"set of three, flags {flags}, niter {niter}")
    return n


def _block_level(gpu, torch, ref, q, c, flags, clamps, what):
    """qs_hip_smooth_plane_next on the reference-built plane of c: coefficients = block() of every block (clamped to
    +-1023 when the clamp rides); the next plane = the reference's IDCT of the launch's UNCLAMPED results -- the kernel
    transforms what its LDS column holds, as the reference clamps once, after its last iteration (:2668-2689), and never
    feeds a clamped value to an IDCT"""
    import test_gpu_plane_kernels as K
    dev = torch.device("cuda:0")
    hb, wb = c.shape[:2]
    want = pc.pass_b_expected_plain(ref, q, c, flags)
    B = K.Bufs(dev)
    cst, d_p = K._consts(B, gpu, q, flags), K._plane_buf(gpu, B, wb, hb, pc.ref_plane(ref, c))
    for clamp in clamps:
        d_c, d_n = K._coef_buf(B, c), K._plane_buf(gpu, B, wb, hb, fill=0xC3)
        gpu.smooth_plane_next(B.ptr(cst), B.ptr(d_c), B.ptr(d_p), B.ptr(d_n), wb, hb, flags, 1, clamp, 1, 1)
        B.check(what)
        _same(K._coefs(B, d_c, c), np.clip(want, -1023, 1023) if clamp else want, f"{what} clamp={clamp}: coefficients")
        _same(K._plane(gpu, B, d_n, wb, hb), pc.ref_plane(ref, want), f"{what} clamp={clamp}: next plane")
    return want


def check_clamp_and_next_plane(pkg, gpu, ref, torch):
    """the fused next-plane write with the +-1023 clamp riding and not riding, on results that leave +-1023"""
    n = 0
    q = pc.table("max")                             # entries up to 0x7ff and three of 1
    for (wb, hb), seed in (((5, 3), 61), ((8, 9), 62)):
        c = pc.coefficients(np.random.default_rng(seed), q, hb, wb, ("random", "ends", "saturate"))
        for flags in (0, pc.F_NOREB):
            want = _block_level(gpu, torch, ref, q, c, flags, (0, 1), f"smooth_plane_next max-table {wb}x{hb} flags={flags}")
            assert np.abs(want.astype(np.int32)).max() > 1023, "the case must make the clamp matter"
            n += 2
    return n


def check_full_range(pkg, gpu, ref, torch):
    """coefficients over the whole int16 range: quotients beyond int32 and 0 / 0 take x86's INT_MIN conversion.

    No job reaches such coefficients (its dequantised coefficients pass the +-2048 range check), and three shortcuts of
    the walk hold only below 0x4000, where the reference's reciprocal tables divide exactly (quantsmooth.h:2527):
    storing the clamped coefficient back when the rounded quotient is 0 (the reference leaves it alone, :1551 -- its
    own interval may miss it by one up there), collecting the rebalance sums during the walk (the reference forms them
    from the final, int16-wrapped coefficients, :1826-1831), and `orig` as an int (the reference keeps it as JCOEF,
    :1829).  A wave staged with a coefficient outside [-0x2000, 0x2000) follows the reference to the letter instead.
    Before that, the 8x9 case differed in 141 values with the rebalance step and 1 without (29816 -> 29817 at quantiser
    49: nearest multiple 609 by the tables, 608 exactly)."""
    n = 0
    for (wb, hb), seed in (((5, 3), 71), ((8, 9), 72), ((65, 2), 73)):
        c = pc.raw_int16_case(seed, hb, wb) if hb >= 4 and wb >= 4 else \
            np.random.default_rng(seed).integers(-32768, 32768, (hb, wb, 64)).astype(np.int16)
        for flags in (0, pc.F_NOREB):
            _block_level(gpu, torch, ref, pc.STD_LUMA, c, flags, (0,), f"smooth_plane_next int16-range {wb}x{hb} flags={flags}")
            n += 1
    return n


def check_diagonals_untouched(pkg, gpu, ref, torch):
    """one q4 job: the DIAGONALS instantiation keeps its pixels and its two stash slots"""
    import test_gpu_deferred_dequant as D
    quant = pkg.synth.quality_table(pkg.synth.STD_LUMA, 50)
    coef = _quantised(pkg, "noise", 8, 9, quant, 5)
    return _run_job(D, gpu, torch, ref, [(coef, quant)], [False], pkg.flags_for_quality(4), 3, "8x9 blocks, noise, q4, niter 3")


CHECKS = {f.__name__: f for f in (check_contents, check_set_launch, check_clamp_and_next_plane, check_full_range, check_diagonals_untouched)}


@pytest.mark.parametrize("check", sorted(CHECKS))
def test_resident_differences_block_per_lane(gpu, check):
    from test_gpu_parity import _run_py
    code = rf'''
import sys, torch
sys.path.insert(0, "tests")
import jpegqs_pkg
import test_gpu_resident_differences as T
from oracle import oracle as om
ref = om.Reference("none") if om.have_ref("none") else om.Oracle()
pkg = jpegqs_pkg.load()
gpu = pkg.HipQS()
print("ok", T.CHECKS["{check}"](pkg, gpu, ref, torch))
'''
    out = _run_py(code, {"QS_HIP_DP": "0"}, timeout=300)
    assert "ok" in out
