"""Every plane-layer call (include/jpegqs_hip.h, "plane layer") against the reference's own block-level functions on the
seeded adversarial inputs of tests/plane_cases.py -- the same expectations tests/test_plane_cases.py checks the oracle
port against without a GPU.  Every device buffer lies between sentinel-filled margins that must survive every call.
Failures name the call, the kernel form, the case and the first differing block and index."""
import numpy as np
import pytest

import plane_cases as pc

pytestmark = pytest.mark.gpu

MARGIN = 4096          # bytes of sentinel before and after every buffer (keeps 16-byte alignment)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def dev(gpu):
    import torch
    return torch.device("cuda:0")


class Bufs:
    """device buffers with sentinel margins; check() asserts every margin is intact"""

    def __init__(self, dev):
        import torch
        self.torch, self.dev, self.all = torch, dev, []

    def alloc(self, nbytes, fill=0x3C, data=None):
        t = self.torch.full((2 * MARGIN + nbytes,), SENTINEL, dtype=self.torch.uint8, device=self.dev)
        if data is not None:
            raw = np.ascontiguousarray(data).view(np.uint8).ravel()
            assert raw.size == nbytes
            t[MARGIN:MARGIN + nbytes] = self.torch.from_numpy(raw.copy()).to(self.dev)
        else:
            t[MARGIN:MARGIN + nbytes] = fill
        self.all.append((t, nbytes))
        return t

    @staticmethod
    def ptr(t):
        return t.data_ptr() + MARGIN

    @staticmethod
    def get(t, nbytes, dtype=np.uint8):
        return t[MARGIN:MARGIN + nbytes].cpu().numpy().view(dtype)

    def check(self, what):
        self.torch.cuda.synchronize()
        for t, n in self.all:
            h = t.cpu().numpy()
            for side, m in (("before", h[:MARGIN]), ("after", h[MARGIN + n:])):
                bad = np.flatnonzero(m != SENTINEL)
                assert not len(bad), f"{what}: {len(bad)} bytes of the margin {side} a {n}-byte buffer were written " \
                                     f"(first at margin byte {int(bad[0])})"


def _coef_buf(B, c):
    return B.alloc(c.nbytes, data=np.ascontiguousarray(c, np.int16))


def _coefs(B, t, c):
    return B.get(t, c.nbytes, np.int16).reshape(c.shape).copy()


def _plane_buf(gpu, B, wb, hb, ref_plane=None, fill=0x3C):
    """a product plane; ref_plane (uint8 [h + 2, w + 2]) is written at rows -1..h, columns -1..w"""
    n = gpu.plane_bytes(wb, hb)
    if ref_plane is None:
        return B.alloc(n, fill=fill)
    raw = np.full(n, 0x5A, np.uint8)
    pitch, off = gpu.plane_pitch(wb), gpu.plane_row_offset(wb, -1)
    rows = raw[off:off + (hb * 8 + 2) * pitch].reshape(hb * 8 + 2, pitch)
    rows[:, pc.QS_APRON_X - 1:pc.QS_APRON_X + wb * 8 + 1] = ref_plane
    return B.alloc(n, data=raw)


def _plane(gpu, B, t, wb, hb, full_rows=False):
    """rows -1..h of a product plane: columns -1..w, or every byte of the row (pitch padding included)"""
    raw = B.get(t, gpu.plane_bytes(wb, hb))
    pitch, off = gpu.plane_pitch(wb), gpu.plane_row_offset(wb, -1)
    rows = raw[off:off + (hb * 8 + 2) * pitch].reshape(hb * 8 + 2, pitch)
    return rows if full_rows else rows[:, pc.QS_APRON_X - 1:pc.QS_APRON_X + wb * 8 + 1]


def _consts(B, gpu, q, flags):
    cst = gpu.consts_build(q, flags)
    return B.alloc(cst.nbytes, data=cst)


def _same(got, want, what):
    msg = pc.first_diff(got, want, what)
    assert msg is None, msg


def _same_blocks(got, want, what):
    """got / want: [..., 64] coefficient blocks; names block (bx, by) or index and coefficient"""
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(got != want)
    if len(bad):
        i = tuple(int(v) for v in bad[0])
        where = f"block (bx={i[1]}, by={i[0]}) coefficient {i[2]}" if got.ndim == 3 else f"block #{i[0]} coefficient {i[1]}"
        pytest.fail(f"{what}: {len(np.unique(bad[:, :-1], axis=0))} blocks differ; first: {where}: got {got[i]}, want {want[i]}")


def _same_plane(got, want, what):
    """plane rows -1..h, columns -1..w"""
    bad = np.argwhere(got != want)
    if len(bad):
        y, x = (int(v) - 1 for v in bad[0])
        pytest.fail(f"{what}: {len(bad)} pixels differ; first at pixel (x={x}, y={y}) = block ({x // 8}, {y // 8}): "
                    f"got {got[y + 1, x + 1]}, want {want[y + 1, x + 1]}")


def _form(nblk):
    """the pass-B kernel the launcher picks for a whole plane of nblk blocks (qs_dp_waves, csrc/qs_kernels.hip)"""
    g = (nblk + 63) // 64
    return "dp-4-waves" if g <= 768 else "dp-2-waves" if g <= 1536 else "block-per-lane"


# ---- pass A -----------------------------------------------------------------------------------------------------------
PASS_A = [("b:" + c[0]) for c in pc.PASS_B_CASES] + [f"raw-int16:{s}" for s in (51, 52, 53)]


def _pass_a_input(name):
    if name.startswith("raw-int16:"):
        return pc.STD_LUMA, pc.raw_int16_case(int(name.split(":")[1]))
    return pc.pass_b_case(name[2:])


@pytest.mark.parametrize("name", PASS_A)
def test_gpu_idct_plane_matches_reference(gpu, dev, reference, name):
    """qs_hip_idct_plane(first = 0) = idct_islow per block + the apron replicate of :2612-2619, byte for byte over rows
    -1..h and columns -1..w; with rep_top = rep_bot = 0 the apron rows -1 and h stay as they were"""
    q, c = _pass_a_input(name)
    hb, wb = c.shape[:2]
    want = pc.ref_plane(reference, c)
    B = Bufs(dev)
    cst, st = _consts(B, gpu, q, 0), B.alloc(4, fill=0)
    for rep in (1, 0):
        d_c, d_p = _coef_buf(B, c), _plane_buf(gpu, B, wb, hb, fill=0x3C)
        gpu.idct_plane(B.ptr(cst), B.ptr(d_c), B.ptr(d_p), wb, hb, 0, rep, rep, B.ptr(st))
        B.check(f"idct_plane {name} rep={rep}")
        got = _plane(gpu, B, d_p, wb, hb)
        what = f"idct_plane(first=0, rep_top=rep_bot={rep}) case {name}"
        if rep:
            _same_plane(got, want, what)
        else:
            _same_plane(got[1:-1], want[1:-1], what)
            full = _plane(gpu, B, d_p, wb, hb, full_rows=True)
            assert (full[0] == 0x3C).all() and (full[-1] == 0x3C).all(), f"{what}: a halo apron row was written"
        _same_blocks(_coefs(B, d_c, c), c, f"{what}: coefficients (first = 0 must not change them)")
    assert int(B.get(st, 4, np.int32)[0]) == 0


@pytest.mark.parametrize("name,stop", pc.STATUS_CASES)
def test_gpu_idct_plane_first_status(gpu, dev, reference, name, stop):
    """first = 1: coefficients become the int16-wrapped products c * q, *d_status is set exactly when :2598-2602 stops,
    and the plane is the IDCT of the wrapped products (interior; the apron too when nothing stops)"""
    q, c = pc.status_case(name)
    assert pc.stops(q, c) == stop
    hb, wb = c.shape[:2]
    wrapped = pc.dequant_wrap(q, c)
    want = pc.ref_plane(reference, wrapped)
    B = Bufs(dev)
    cst, st = _consts(B, gpu, q, 0), B.alloc(4, fill=0)
    d_c, d_p = _coef_buf(B, c), _plane_buf(gpu, B, wb, hb)
    gpu.idct_plane(B.ptr(cst), B.ptr(d_c), B.ptr(d_p), wb, hb, 1, 1, 1, B.ptr(st))
    B.check(f"idct_plane first=1 {name}")
    got_stop = int(B.get(st, 4, np.int32)[0])
    assert bool(got_stop & 1) == stop, f"idct_plane(first=1) case {name}: status {got_stop}, reference stops: {stop}"
    _same_blocks(_coefs(B, d_c, c), wrapped, f"idct_plane(first=1) case {name}: dequantised coefficients")
    got = _plane(gpu, B, d_p, wb, hb)
    if stop:
        _same_plane(got[1:-1, 1:-1], want[1:-1, 1:-1], f"idct_plane(first=1) case {name}: interior")
    else:
        _same_plane(got, want, f"idct_plane(first=1) case {name}")


# ---- pass B -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", pc.PASS_B_FLAGS)
@pytest.mark.parametrize("name", [c[0] for c in pc.PASS_B_CASES])
def test_gpu_smooth_plane_matches_reference(gpu, dev, reference, name, flags):
    """qs_hip_smooth_plane = block() per block on the reference-built plane (luma 0 and 1; + the +-1023 clamp);
    qs_hip_smooth_plane_next: the same coefficients and, as its next plane, the reference-built plane of them"""
    q, c = pc.pass_b_case(name)
    hb, wb = c.shape[:2]
    form = _form(hb * wb)
    plane = pc.ref_plane(reference, c)
    B = Bufs(dev)
    cst = _consts(B, gpu, q, flags)
    d_p = _plane_buf(gpu, B, wb, hb, plane)
    for luma in (1, 0):
        want = pc.pass_b_expected(reference, name, flags, luma).reshape(c.shape)
        for clamp in (0, 1):
            d_c = _coef_buf(B, c)
            gpu.smooth_plane(B.ptr(cst), B.ptr(d_c), B.ptr(d_p), wb, hb, flags, luma, clamp)
            B.check(f"smooth_plane {name}")
            w = np.clip(want, -1023, 1023) if clamp else want
            _same_blocks(_coefs(B, d_c, c), w, f"smooth_plane[{form}] case {name} flags={flags} luma={luma} clamp={clamp}")
        if luma:
            d_c, d_n = _coef_buf(B, c), _plane_buf(gpu, B, wb, hb, fill=0xC3)
            gpu.smooth_plane_next(B.ptr(cst), B.ptr(d_c), B.ptr(d_p), B.ptr(d_n), wb, hb, flags, luma, 0, 1, 1)
            B.check(f"smooth_plane_next {name}")
            what = f"smooth_plane_next[{form}] case {name} flags={flags}"
            _same_blocks(_coefs(B, d_c, c), want, what)
            _same_plane(_plane(gpu, B, d_n, wb, hb), pc.ref_plane(reference, want), what + ": next plane")
    _same_plane(_plane(gpu, B, d_p, wb, hb), plane, f"smooth_plane case {name}: the plane it reads was written")


def test_gpu_smooth_rows_leaves_other_rows(gpu, dev, reference):
    """qs_hip_smooth_rows(row0, row1): block rows [row0, row1) as smooth_plane, every other coefficient untouched"""
    name, flags = "std-mixed-kinds", 1
    q, c = pc.pass_b_case(name)
    hb, wb = c.shape[:2]
    want = pc.pass_b_expected(reference, name, flags, 1).reshape(c.shape)
    B = Bufs(dev)
    cst, d_p = _consts(B, gpu, q, flags), _plane_buf(gpu, B, wb, hb, pc.ref_plane(reference, c))
    for r0, r1 in ((0, 1), (2, 5), (hb - 1, hb), (3, 3)):
        d_c = _coef_buf(B, c)
        gpu.smooth_rows(B.ptr(cst), B.ptr(d_c), B.ptr(d_p), wb, hb, r0, r1, flags, 1, 0)
        B.check(f"smooth_rows {r0}..{r1}")
        got = _coefs(B, d_c, c)
        _same_blocks(got[r0:r1], want[r0:r1], f"smooth_rows({r0}, {r1}) case {name}: rows inside")
        outside = np.ones(hb, bool); outside[r0:r1] = False
        _same_blocks(got[outside], c[outside], f"smooth_rows({r0}, {r1}) case {name}: rows outside (block index)")


def test_gpu_plane_sets_mixed(gpu, dev, reference):
    """qs_hip_idct_planes + qs_hip_smooth_planes over every pass-B case in ONE launch each (different sizes, tables and
    luma); planes with band bits keep their halo-side apron rows, which then receive what the neighbour would send"""
    flags = pc.F_DIAG
    B = Bufs(dev)
    st = B.alloc(4 * len(pc.PASS_B_CASES), fill=0)
    items, refs = [], []
    for i, case in enumerate(pc.PASS_B_CASES):
        q, c = pc.pass_b_case(case[0])
        hb, wb = c.shape[:2]
        band, luma = i % 4, i % 2
        cst, d_c, d_p = _consts(B, gpu, q, flags), _coef_buf(B, c), _plane_buf(gpu, B, wb, hb, fill=0x3C)
        items.append((case[0], q, c, band, luma, d_c, d_p))
        refs.append((B.ptr(cst), B.ptr(d_c), B.ptr(d_p), B.ptr(st) + 4 * i, wb, hb, luma, band))
    R = gpu.plane_refs(refs)
    gpu.idct_planes(R, 0)
    B.check("idct_planes")
    for name, q, c, band, luma, d_c, d_p in items:
        hb, wb = c.shape[:2]
        want = pc.ref_plane(reference, c)
        full = _plane(gpu, B, d_p, wb, hb, full_rows=True)
        got = _plane(gpu, B, d_p, wb, hb)
        what = f"idct_planes case {name} band={band}"
        _same_plane(got[1:-1], want[1:-1], what)
        for bit, row in ((1, 0), (2, -1)):
            if band & bit:
                assert (full[row] == 0x3C).all(), f"{what}: the halo apron row {'top' if bit == 1 else 'bottom'} was written"
            else:
                _same(got[row], want[row], f"{what}: replicated apron row {row}")
        # the halo rows a neighbour sends: here the replicate of the image edge
        raw = B.get(d_p, gpu.plane_bytes(wb, hb)).copy()
        for y in (-1, hb * 8):
            o = gpu.plane_row_offset(wb, y) + pc.QS_APRON_X - 1
            raw[o:o + wb * 8 + 2] = want[y + 1]
        d_p.copy_(B.torch.from_numpy(np.concatenate([np.full(MARGIN, SENTINEL, np.uint8), raw,
                                                      np.full(MARGIN, SENTINEL, np.uint8)])).to(dev))
    gpu.smooth_planes(R, flags)
    B.check("smooth_planes")
    for name, q, c, band, luma, d_c, d_p in items:
        want = pc.pass_b_expected(reference, name, flags, luma).reshape(c.shape)
        _same_blocks(_coefs(B, d_c, c), want, f"smooth_planes case {name} band={band} luma={luma} flags={flags}")


@pytest.mark.parametrize("name", [n for n, *_ in pc.LARGE_CASES])
def test_gpu_large_planes_every_form(gpu, dev, reference, oracle, name):
    """planes large enough for the 2-wave and the block-per-lane forms of pass B: pass A against the oracle port's
    plane, every block of pass B against the oracle port, edge, corner and sampled blocks against the reference"""
    q, c = pc.large_case(name)
    hb, wb = c.shape[:2]
    form = _form(hb * wb)
    assert form == {"dp2": "dp-2-waves", "lane": "block-per-lane"}[name]
    flags = pc.F_DIAG
    B = Bufs(dev)
    cst, st = _consts(B, gpu, q, flags), B.alloc(4, fill=0)
    d_c, d_p = _coef_buf(B, c), _plane_buf(gpu, B, wb, hb)
    gpu.idct_plane(B.ptr(cst), B.ptr(d_c), B.ptr(d_p), wb, hb, 0, 1, 1, B.ptr(st))
    B.check(f"idct_plane {name}")
    oplane = pc.oracle_plane(oracle, q, c)
    _same_plane(_plane(gpu, B, d_p, wb, hb), pc.apron_view(oplane, wb, hb), f"idct_plane case {name} vs the oracle port")
    gpu.smooth_plane(B.ptr(cst), B.ptr(d_c), B.ptr(d_p), wb, hb, flags, 1, 0)
    B.check(f"smooth_plane {name}")
    got = _coefs(B, d_c, c)
    _same_blocks(got, pc.oracle_band_smooth(oracle, q, c, oplane, flags), f"smooth_plane[{form}] case {name} vs the oracle port")
    want, pos = pc.large_sample_expected(reference, oracle, name, flags)
    _same_blocks(np.stack([got[by, bx] for bx, by in pos]), want,
                 f"smooth_plane[{form}] case {name} vs the reference (sampled blocks, in (by, bx) order)")


def test_gpu_smooth_plane_block_per_lane_small(gpu):
    """QS_HIP_DP=0 (read once per process): the block-per-lane form on every small pass-B case, fresh process"""
    from test_gpu_parity import _run_py
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, "tests")
import jpegqs_pkg, plane_cases as pc
from oracle import oracle as om
ref = om.Reference("none") if om.have_ref("none") else om.RecordedReference()
gpu = jpegqs_pkg.load().HipQS()
dev = torch.device("cuda:0")
n = 0
for case in pc.PASS_B_CASES:
    q, c = pc.pass_b_case(case[0]); hb, wb = c.shape[:2]
    raw = np.zeros(gpu.plane_bytes(wb, hb), np.uint8)
    pitch, off = gpu.plane_pitch(wb), gpu.plane_row_offset(wb, -1)
    raw[off:off + (hb * 8 + 2) * pitch].reshape(hb * 8 + 2, pitch)[:, pc.QS_APRON_X - 1:pc.QS_APRON_X + wb * 8 + 1] = pc.ref_plane(ref, c)
    d_p = torch.from_numpy(raw).to(dev)
    for flags in pc.PASS_B_FLAGS:
        cst = torch.from_numpy(gpu.consts_build(q, flags)).to(dev)
        for luma in (1, 0):
            d_c = torch.from_numpy(c.copy()).to(dev)
            gpu.smooth_plane(cst.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), wb, hb, flags, luma, 0)
            got = d_c.cpu().numpy()
            want = pc.pass_b_expected(ref, case[0], flags, luma).reshape(c.shape)
            msg = pc.first_diff(got, want, f"smooth_plane[block-per-lane, QS_HIP_DP=0] case {case[0]} flags={flags} luma={luma} (by, bx, k)")
            assert msg is None, msg
            n += 1
print("ok", n)
'''
    out = _run_py(code, {"QS_HIP_DP": "0"}, timeout=300)
    assert "ok" in out


# ---- JOINT_YUV and LOW_QUALITY ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", (0, pc.F_DIAG, pc.F_NOREB))
@pytest.mark.parametrize("name", ["std-mixed-kinds", "camera-checker", "max-table", "zeros-table"])
def test_gpu_joint_and_lowq_match_reference(gpu, dev, reference, name, flags):
    """qs_hip_joint_plane + qs_hip_smooth_plane = block(plane2) under JOINT_YUV (chroma); qs_hip_lowq_plane =
    block() under LOW_QUALITY (luma 0 / 1); qs_hip_joint_plane with its rebalance = block(plane2) under LOW_QUALITY"""
    q, c, plane, plane2 = pc.joint_inputs(reference, name)
    hb, wb = c.shape[:2]
    B = Bufs(dev)
    cst = _consts(B, gpu, q, flags)
    d_p, d_l = _plane_buf(gpu, B, wb, hb, plane), _plane_buf(gpu, B, wb, hb, plane2)
    d_c = _coef_buf(B, c)
    gpu.joint_plane(B.ptr(cst), B.ptr(d_c), B.ptr(d_p), B.ptr(d_l), wb, hb, 0, 0)
    gpu.smooth_plane(B.ptr(cst), B.ptr(d_c), B.ptr(d_p), wb, hb, flags, 0, 0)
    B.check(f"joint_plane + smooth_plane {name}")
    _same_blocks(_coefs(B, d_c, c), pc.joint_expected(reference, name, flags).reshape(c.shape),
                 f"joint_plane + smooth_plane case {name} flags={flags}")
    for luma in (1, 0):
        d_c = _coef_buf(B, c)
        gpu.lowq_plane(B.ptr(cst), B.ptr(d_c), B.ptr(d_p), wb, hb, int(pc.rebalance_on(flags, luma)), 0)
        B.check(f"lowq_plane {name}")
        _same_blocks(_coefs(B, d_c, c), pc.lowq_expected(reference, name, flags, luma, False).reshape(c.shape),
                     f"lowq_plane case {name} flags={flags} luma={luma}")
    d_c = _coef_buf(B, c)
    gpu.joint_plane(B.ptr(cst), B.ptr(d_c), B.ptr(d_p), B.ptr(d_l), wb, hb, int(pc.rebalance_on(flags, 0)), 1)
    B.check(f"joint_plane lowq {name}")
    want = np.clip(pc.lowq_expected(reference, name, flags, 0, True).reshape(c.shape), -1023, 1023)
    _same_blocks(_coefs(B, d_c, c), want, f"joint_plane(LOW_QUALITY, final clamp) case {name} flags={flags}")


# ---- UPSAMPLE_UV, the low-res luma, the re-encode ---------------------------------------------------------------------
@pytest.mark.parametrize("w,h,ws,hs", pc.UPSAMPLE_CASES)
def test_gpu_upsample_matches_reference(gpu, dev, reference, w, h, ws, hs):
    """qs_hip_upsample_plane and qs_hip_upsample_rows(first_rows = 0, 1..7, 8) against upsample_row per strip plus the
    bottom replicate of :2729-2730, over the rows and columns the re-encode reads"""
    g, ycoef, ccoef, luma, lowres, chroma = pc.upsample_inputs(reference, w, h, ws, hs, seed=w * h)
    ww, hh, st = g["ww"], g["hh"], g["st"]
    assert gpu.upsample_pitch(w, ws) == st
    B = Bufs(dev)
    d_y = _plane_buf(gpu, B, g["ywb"], g["yhb"], luma[:, :ww + 2])
    d_l = _plane_buf(gpu, B, g["cwb"], g["chb"], lowres)
    d_c = _plane_buf(gpu, B, g["cwb"], g["chb"], chroma)
    nbytes = gpu.lib.qs_hip_upsample_bytes(w, h, ws, hs)
    what = f"({w}x{h}, {ws}x{hs}, w1={g['w1']}, h1={g['h1']})"
    d_px = B.alloc(nbytes, fill=0x77)
    gpu._check(gpu.lib.qs_hip_upsample_plane(B.ptr(d_c), B.ptr(d_l), g["cwb"], B.ptr(d_y), g["ywb"], g["yhb"],
                                             B.ptr(d_px), w, h, ws, hs, None))
    B.check(f"upsample_plane {what}")
    got = B.get(d_px, st * hh).reshape(hh, st)
    want = pc.upsample_expected(reference, g, luma, lowres, chroma, ws, hs)
    _same(got[:, :ww], want[:hh, :ww], f"upsample_plane {what} (row, column)")
    for f in pc.first_rows_list(g["h1"]):
        d_px = B.alloc(nbytes, fill=0x77)
        gpu.upsample_rows(B.ptr(d_c), B.ptr(d_l), g["cwb"], B.ptr(d_y), g["ywb"], g["yhb"], B.ptr(d_px), st,
                          g["w1"], g["h1"], f, ws, hs)
        B.check(f"upsample_rows {what} first_rows={f}")
        got = B.get(d_px, st * hh).reshape(hh, st)
        want = pc.upsample_expected(reference, g, luma, lowres, chroma, ws, hs, first_rows=f)
        _same(got[:, :ww], want[:hh, :ww], f"upsample_rows {what} first_rows={f} (row, column)")


@pytest.mark.parametrize("w,h,ws,hs", [c for c in pc.UPSAMPLE_CASES])
def test_gpu_downsample_matches_restatement(gpu, dev, reference, w, h, ws, hs):
    """qs_hip_downsample_plane: the box mean (sum + n/2) / n of :2753-2815, replicated to the edge and apron"""
    g, ycoef, ccoef, luma, lowres, chroma = pc.upsample_inputs(reference, w, h, ws, hs, seed=w * h)
    lw, lh = g["cwb"] * 8, g["chb"] * 8
    want = pc.downsample_expected(pc.pixels(reference, ycoef), lw, lh, ws, hs)
    B = Bufs(dev)
    d_y = _plane_buf(gpu, B, g["ywb"], g["yhb"], luma[:, :g["ww"] + 2])
    d_l = _plane_buf(gpu, B, g["cwb"], g["chb"], fill=0x3C)
    gpu.downsample_plane(B.ptr(d_y), g["ywb"], g["yhb"], B.ptr(d_l), g["cwb"], g["chb"], ws, hs)
    B.check(f"downsample_plane {w}x{h} {ws}x{hs}")
    _same_plane(_plane(gpu, B, d_l, g["cwb"], g["chb"]), want, f"downsample_plane ({w}x{h}, {ws}x{hs})")


def test_gpu_fdct_plane_matches_reference(gpu, dev, reference):
    """qs_hip_fdct_plane = fdct_float(pixel - 128), then C roundf (ties away from zero), :2740-2749"""
    px = pc.fdct_case()
    hb, wb = px.shape[0] // 8, px.shape[1] // 8
    want = pc.fdct_expected(reference, pc.fdct_blocks_of(px)).reshape(hb, wb, 64)
    B = Bufs(dev)
    for extra in (0, 24):                       # the buffer's pitch may exceed the blocks' width
        pitch = wb * 8 + extra
        buf = np.full((hb * 8, pitch), 0xEE, np.uint8)
        buf[:, :wb * 8] = px
        d_px = B.alloc(buf.nbytes, data=buf)
        d_c = B.alloc(hb * wb * 128, fill=0x11)
        gpu.fdct_plane(B.ptr(d_px), pitch, B.ptr(d_c), wb, hb)
        B.check("fdct_plane")
        _same_blocks(B.get(d_c, hb * wb * 128, np.int16).reshape(hb, wb, 64), want, f"fdct_plane pitch={pitch}")


def test_gpu_dequant_and_clamp_plane(gpu, dev):
    """qs_hip_dequant_plane: int16-wrapping c * q (:2563, zero quantisers included); qs_hip_clamp_plane: +-1023"""
    q, c = pc.dequant_case()
    hb, wb = c.shape[:2]
    B = Bufs(dev)
    cst, d_c = _consts(B, gpu, q, 0), _coef_buf(B, c)
    gpu.dequant_plane(B.ptr(cst), B.ptr(d_c), wb, hb)
    B.check("dequant_plane")
    _same_blocks(_coefs(B, d_c, c), pc.dequant_wrap(q, c), "dequant_plane")
    d_c = _coef_buf(B, c)
    gpu.clamp_plane(B.ptr(d_c), wb, hb)
    B.check("clamp_plane")
    _same_blocks(_coefs(B, d_c, c), np.clip(c, -1023, 1023), "clamp_plane")
