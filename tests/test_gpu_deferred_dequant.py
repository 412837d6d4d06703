"""Deferred dequantisation (include/jpegqs_hip.h: QS_HIP_PLANE_DEFER): the first pass A leaves the coefficients quantised
and the first recovery launch multiplies while it loads them.  Everything is bit-exact: the deferred route against the
eager route and against the compiled reference (oracle/_ref/libqsref_none.so; the plain-C port where it did not
travel), on both forms of the recovery kernel -- the small-plane form in this process, one block per lane in a fresh
process with QS_HIP_DP=0 (the switch is read once per process).

Shapes: 1x1 block; 9x5 and 65x3 (partial waves, partial 16-byte groups, a wave that crosses a block-row boundary);
129x2; a set of three planes of different sizes of which only some defer."""
import os

import numpy as np
import pytest

import plane_cases as pc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (9, 5), (65, 3), (129, 2)]      # (wblk, hblk)
DEFER = 4                                         # QS_HIP_PLANE_DEFER


def _input(pkg, wb, hb, seed):
    coef, quant = pkg.synth.synth_gray(wb * 8, hb * 8, 50, seed=seed)
    assert coef.shape == (hb, wb, 64)
    return np.ascontiguousarray(coef, np.int16), np.asarray(quant, np.uint16)


def _dequant(coef, quant):
    return (coef.astype(np.int32) * quant.astype(np.int32)[None, None, :]).astype(np.int16)


class Plane:
    """one plane on the device: coefficients, two pixel planes (filled with 0x3C), constants, status word"""

    def __init__(self, gpu, torch, coef, quant, flags, band=0):
        dev = torch.device("cuda:0")
        self.gpu, self.torch = gpu, torch
        self.hb, self.wb = coef.shape[:2]
        self.band = band
        self.cst = torch.from_numpy(gpu.consts_build(quant, flags)).to(dev)
        self.coef = torch.from_numpy(coef.copy()).to(dev)
        n = gpu.plane_bytes(self.wb, self.hb)
        self.plane = torch.full((n,), 0x3C, dtype=torch.uint8, device=dev)
        self.plane2 = torch.full((n,), 0x3C, dtype=torch.uint8, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)

    def ref(self, bits, nxt=False):
        return (self.cst.data_ptr(), self.coef.data_ptr(), self.plane.data_ptr(), self.status.data_ptr(),
                self.wb, self.hb, 1, self.band | bits, self.plane2.data_ptr() if nxt else None)

    def rows(self, t, full=False):
        """rows -1..h of a pixel plane: columns -1..w, or whole rows"""
        raw = t.cpu().numpy()
        pitch, off = self.gpu.plane_pitch(self.wb), self.gpu.plane_row_offset(self.wb, -1)
        r = raw[off:off + (self.hb * 8 + 2) * pitch].reshape(self.hb * 8 + 2, pitch)
        return r if full else r[:, pc.QS_APRON_X - 1:pc.QS_APRON_X + self.wb * 8 + 1]


def _run_set(gpu, torch, planes, defer, flags, niter, after_a=None, after_first=None):
    """the fused plane-set schedule: pass A once, niter recovery launches; defer[i]: plane i defers its dequantisation"""
    bits = [DEFER if d else 0 for d in defer]
    gpu.idct_planes(gpu.plane_refs([p.ref(b) for p, b in zip(planes, bits)]), 1)
    if after_a:
        torch.cuda.synchronize()
        after_a()
    for it in range(niter):
        nxt = it < niter - 1
        gpu.smooth_planes(gpu.plane_refs([p.ref(b if it == 0 else 0, nxt) for p, b in zip(planes, bits)]), flags, it == niter - 1)
        if nxt:
            for p in planes:
                p.plane, p.plane2 = p.plane2, p.plane
        if it == 0 and after_first:
            torch.cuda.synchronize()
            after_first()
    torch.cuda.synchronize()


def _same(got, want, what):
    msg = pc.first_diff(np.asarray(got), np.asarray(want), what)
    assert msg is None, msg


def check_shapes(pkg, gpu, ref, torch, form):
    """every shape x q3 / q4 x niter 1 / 3: deferred == eager == reference, coefficients and the next pixel plane"""
    for wb, hb in SHAPES:
        coef, quant = _input(pkg, wb, hb, 100 + wb)
        deq = _dequant(coef, quant)
        for quality in (3, 4):
            flags = pkg.flags_for_quality(quality)
            for niter in (1, 3):
                what = f"[{form}] {wb}x{hb} blocks q{quality} niter {niter}"
                want = ref.do_quantsmooth([coef], [quant], flags, niter)
                assert want["ret"] == 0
                res = {}
                for defer in (False, True):
                    p = Plane(gpu, torch, coef, quant, flags)
                    name = "deferred" if defer else "eager"

                    def after_a():
                        # the default semantics: dequantised after the eager pass A; untouched after the deferred one
                        _same(p.coef.cpu().numpy(), coef if defer else deq, f"{what}: coef after the {name} pass A")
                        _same(p.rows(p.plane), pc.ref_plane(ref, deq), f"{what}: pixel plane of the {name} pass A")

                    def after_first():
                        if niter > 1:
                            c1 = p.coef.cpu().numpy()
                            res[name, "c1"] = c1
                            res[name, "next"] = p.rows(p.plane).copy()
                            _same(res[name, "next"], pc.ref_plane(ref, c1), f"{what}: next pixel plane of the {name} route "
                                  "vs the reference's IDCT of the launch's coefficients")
                    _run_set(gpu, torch, [p], [defer], flags, niter, after_a, after_first)
                    assert int(p.status.item()) == 0
                    res[name] = p.coef.cpu().numpy()
                    _same(res[name], want["coefs"][0], f"{what}: {name} route vs the reference")
                _same(res["deferred"], res["eager"], f"{what}: deferred vs eager")
                if niter > 1:
                    _same(res["deferred", "c1"], res["eager", "c1"], f"{what}: coefficients after the first launch, deferred vs eager")
                    _same(res["deferred", "next"], res["eager", "next"], f"{what}: next pixel plane, deferred vs eager")


def check_mixed_set(pkg, gpu, ref, torch, form):
    """three planes of different sizes in one launch, only the first and the last deferred"""
    flags = pkg.flags_for_quality(3)
    ins = [_input(pkg, wb, hb, 7 + wb) for wb, hb in ((9, 5), (1, 1), (65, 3))]
    planes = [Plane(gpu, torch, c, q, flags) for c, q in ins]
    defer = [True, False, True]

    def after_a():
        for p, (c, q), d in zip(planes, ins, defer):
            _same(p.coef.cpu().numpy(), c if d else _dequant(c, q), f"[{form}] mixed set: coef after pass A (deferred={d})")
    _run_set(gpu, torch, planes, defer, flags, 3, after_a)
    for p, (c, q) in zip(planes, ins):
        want = ref.do_quantsmooth([c], [q], flags, 3)
        _same(p.coef.cpu().numpy(), want["coefs"][0], f"[{form}] mixed set: plane {p.wb}x{p.hb} vs the reference")


def _range_case(pkg):
    """a quantiser with entries 1 and entries >= 0x800, and coefficients whose products leave +-2048 (one of them past int16)"""
    coef, quant = _input(pkg, 9, 5, 31)
    quant = quant.copy()
    quant[[0, 5, 9, 63]] = 1
    quant[[1, 8, 40]] = [0x800, 0x9c4, 0xffff]
    coef = coef.copy()
    coef[:, :, [1, 8, 40]] = 0
    coef[2, 3, 1] = 1          # 2048: just outside
    coef[4, 8, 8] = -27        # wraps in int16
    coef[0, 0, 40] = 1         # 65535 -> -1
    coef[1, 1, 2] = 700        # an ordinary entry, product far outside
    return coef, quant


def check_range_stop(pkg, gpu, ref, torch, form):
    """a tripped range check: status and the final arrays of every deferred route equal the eager route's"""
    from jpeg_quantsmooth_amd import bands
    coef, quant = _range_case(pkg)
    flags = pkg.flags_for_quality(3)
    # plane-set calls
    out = {}
    for defer in (False, True):
        p = Plane(gpu, torch, coef, quant, flags)
        _run_set(gpu, torch, [p], [defer], flags, 3)
        out[defer] = (int(p.status.item()), p.coef.cpu().numpy())
    assert out[True][0] == out[False][0] == 1, f"[{form}] status words {out[True][0]} / {out[False][0]}"
    _same(out[True][1], out[False][1], f"[{form}] tripped range check, plane-set calls: deferred vs eager")
    # the band schedules (what bench.py drives), QS_BANDS_DEFER read per call
    dev = torch.device("cuda:0")
    topo = bands.BandTopology(0, 1, 0, coef.shape[0])
    old = os.environ.get("QS_BANDS_DEFER")
    try:
        for sched in ("sets", "edge_first"):
            got = {}
            for d in ("0", "1"):
                os.environ["QS_BANDS_DEFER"] = d
                e = bands.HipBandEngine(gpu, torch, torch.from_numpy(coef.copy()).to(dev), quant, flags, luma=1, device=dev)
                if sched == "sets":
                    bands.run_bands_batched_sets(gpu, [e], topo, 3, lambda: None)
                else:
                    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
                    bands.run_band_edge_first(gpu, e, topo, 3, lambda: None, main, side, torch)
                torch.cuda.synchronize()
                got[d] = (e.bad_coef(), e.coef.cpu().numpy())
            assert got["0"][0] and got["1"][0], f"[{form}] bands {sched}: the range check did not trip"
            _same(got["1"][1], got["0"][1], f"[{form}] tripped range check, bands {sched}: deferred vs eager")
            _same(got["1"][1], out[False][1], f"[{form}] tripped range check, bands {sched} vs the plane-set calls")
    finally:
        if old is None:
            os.environ.pop("QS_BANDS_DEFER", None)
        else:
            os.environ["QS_BANDS_DEFER"] = old
    # the job layer (fused route on host arrays) against the reference: return code and arrays
    want = ref.do_quantsmooth([coef], [quant], flags, 3)
    one = gpu.do_quantsmooth([coef], [quant], flags, 3)
    assert one["ret"] == want["ret"], f"[{form}] job layer: ret {one['ret']} != reference {want['ret']}"
    _same(one["coefs"][0], want["coefs"][0], f"[{form}] tripped range check, job layer vs the reference")
    _same(one["quants"][0], want["quants"][0], f"[{form}] tripped range check, job layer: quant table vs the reference")


def check_job_layer(pkg, gpu, ref, torch, form):
    """the routes of the job layer that defer (fused; batch with and without JOINT_YUV) against the reference"""
    coef, quant = _input(pkg, 65, 3, 9)
    for quality in (3, 4):
        flags = pkg.flags_for_quality(quality)
        for niter in (1, 3):
            want = ref.do_quantsmooth([coef], [quant], flags, niter)
            got = gpu.do_quantsmooth([coef], [quant], flags, niter)
            assert got["ret"] == want["ret"] == 0
            _same(got["coefs"][0], want["coefs"][0], f"[{form}] job layer q{quality} niter {niter} vs the reference")
    job = pkg.synth.synth_ycc(72, 40, 2, 2, 50)
    coefs, quants, hsamp, vsamp = job["coefs"], job["quants"], job["hsamp"], job["vsamp"]
    for quality in (3, 6):                     # 6: JOINT_YUV + UPSAMPLE_UV, whose chroma stays eager
        flags = pkg.flags_for_quality(quality)
        want = ref.do_quantsmooth(coefs, quants, flags, 2, hsamp=hsamp, vsamp=vsamp, image_size=(72, 40))
        got = gpu.do_quantsmooth(coefs, quants, flags, 2, hsamp=hsamp, vsamp=vsamp, image_size=(72, 40))
        assert got["ret"] == want["ret"] == 0
        for ci in range(3):
            _same(got["coefs"][ci], want["coefs"][ci], f"[{form}] colour job q{quality} component {ci} vs the reference")


def check_halo_and_plane_kernel(pkg, gpu, ref, torch, form):
    """a band whose apron rows are halo rows: the deferred pass A leaves them alone; and the single-plane pass A's
    deferred form (first = 1 | QS_HIP_FIRST_DEFER) writes the eager form's plane and leaves coef as it found it"""
    coef, quant = _input(pkg, 9, 5, 5)
    flags = pkg.flags_for_quality(3)
    deq = _dequant(coef, quant)
    p = Plane(gpu, torch, coef, quant, flags, band=3)
    gpu.idct_planes(gpu.plane_refs([p.ref(DEFER)]), 1)
    torch.cuda.synchronize()
    full = p.rows(p.plane, full=True)
    assert (full[0] == 0x3C).all() and (full[-1] == 0x3C).all(), f"[{form}] the deferred pass A wrote a halo apron row"
    _same(p.rows(p.plane)[1:-1], pc.ref_plane(ref, deq)[1:-1], f"[{form}] band rows of the deferred pass A")
    _same(p.coef.cpu().numpy(), coef, f"[{form}] coef after the deferred pass A of a band")
    planes = {}
    for first in (1, 3):
        s = Plane(gpu, torch, coef, quant, flags)
        gpu.idct_plane(s.cst.data_ptr(), s.coef.data_ptr(), s.plane.data_ptr(), s.wb, s.hb, first, 1, 1, s.status.data_ptr())
        torch.cuda.synchronize()
        _same(s.coef.cpu().numpy(), deq if first == 1 else coef, f"[{form}] coef after idct_plane(first={first})")
        planes[first] = s.plane.cpu().numpy()
        _same(s.rows(s.plane), pc.ref_plane(ref, deq), f"[{form}] plane of idct_plane(first={first})")
    assert np.array_equal(planes[1], planes[3])


CHECKS = [check_shapes, check_mixed_set, check_range_stop, check_job_layer, check_halo_and_plane_kernel]


@pytest.fixture(scope="module")
def truth():
    """the compiled, unmodified reference where it travelled with the tree, the plain-C port otherwise (as in test_gpu_fullsize.py)"""
    from oracle import oracle as om
    return om.Reference("none") if om.have_ref("none") else om.Oracle()


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_deferred_dequant_small_plane_form(check, pkg, gpu, truth):
    import torch
    check(pkg, gpu, truth, torch, "small-plane form")


def test_deferred_dequant_block_per_lane_form(gpu):
    """the same checks with QS_HIP_DP=0: every recovery launch takes the one-block-per-lane kernel (fresh process)"""
    from test_gpu_parity import _run_py
    code = r'''
import sys, torch
sys.path.insert(0, "tests")
import jpegqs_pkg
import test_gpu_deferred_dequant as T
from oracle import oracle as om
ref = om.Reference("none") if om.have_ref("none") else om.Oracle()
pkg = jpegqs_pkg.load()
gpu = pkg.HipQS()
for check in T.CHECKS:
    check(pkg, gpu, ref, torch, "block per lane, QS_HIP_DP=0")
print("ok", len(T.CHECKS))
'''
    out = _run_py(code, {"QS_HIP_DP": "0"}, timeout=300)
    assert "ok" in out
