"""The luma recovery kernel's rebalance epilogue applies only ONE bound of a coefficient's interval
(qs_rebalance_outward, csrc/qs_devfn.h): the reference computes  clamp((c * mul + 0x1000) >> 13, lo, hi)  with
mul = round(8192 * m1 / m0) >= 8192, and scaling by at least one moves a coefficient away from zero, so only the bound
on the far side of zero can bind.  Checked here exhaustively, on the CPU, against the project's own interval arithmetic:

  * the reciprocal-table form the kernels run (interval(), csrc/qs_devfn.h; tables of csrc/qs_tables.cpp), written in
    numpy, is first pinned to the oracle port's qso_interval on a spread of (c, quantiser);
  * for every c in [-0x2400, 0x2400] (what a wave without a staged coefficient outside [-0x2000, 0x2000) can hold: 0x2000
    plus less than a quantiser < 0x800, with room), every quantiser 1..0x7ff and mul in {8192, 8193, a spread, 0x7fff,
    2^31 - 1}: c and orig never differ in sign, c lies in its own interval, the helper's arithmetic (rounding constant
    and shift as scalars, +-d0 as (d0 + t) ^ t, the median of {v, b, c}) equals the two-sided clamp -- the inward bound
    never changes the result;
  * the product is the reference's wrapping 32-bit one: up to QS_REB_MUL_MAX = 0x7fff nothing wraps, so the statement
    holds for the arithmetic the kernel executes; at 2^31 - 1 it holds for the exact product only -- wrapped, the result
    can land on the inward side -- which is why the kernel checks mul against QS_REB_MUL_MAX (wave-uniformly) and sends
    anything larger down the two-sided loop instead of assuming the bound mul <= 16384 that its sums imply."""
import numpy as np
import pytest

from oracle import oracle as om

C_MAX = 0x2400
QS_REB_MUL_MAX = 0x7fff
MULS = (8192, 8193, 9000, 12000, 16384, QS_REB_MUL_MAX, 2**31 - 1)


def _tables(q):
    """x1 (as int16) and the shift 15 - floor(log2 q) of quantisers q (csrc/qs_tables.cpp, reference :2514-2539)"""
    q = np.asarray(q, np.int64)
    n = np.floor(np.log2(q)).astype(np.int64)
    assert ((1 << n) <= q).all() and (q < (2 << n)).all()
    x1 = ((0x10000 << n) + q - 1) // q
    x1 = np.where(n > 0, x1 | (x1 >> 16), x1)
    return ((x1 & 0xffff) ^ 0x8000) - 0x8000, 15 - n


def _interval(c, q, x1, sh):
    """interval() of csrc/qs_devfn.h -> orig, lo, hi"""
    a = ((x1 * c) >> 16) + c
    a = ((a << sh) + 0x4000) >> 15
    a = a * q
    d0, d1 = (q - 1) >> 1, q >> 1
    return a, a - np.where(a > 0, d1, d0), a + np.where(a < 0, d1, d0)


def _outward_bound(c, q, x1, sh):
    """qs_rebalance_outward's b, with its own arithmetic"""
    rnd, shr = 0x4000 >> sh, 15 - sh
    a = (((x1 * c) >> 16) + c + rnd) >> shr
    d0, t = (q - 1) >> 1, c >> 63
    return a * q + ((d0 + t) ^ t)


def _wrap32(x):
    return ((x + 2**31) & (2**32 - 1)) - 2**31


def test_numpy_interval_is_the_oracle_ports():
    o = om.Oracle()
    rng = np.random.default_rng(5)
    qs = np.concatenate([np.arange(1, 40), [63, 64, 65, 127, 128, 255, 256, 1023, 1024, 2046, 2047], rng.integers(1, 0x800, 40)])
    cs = np.concatenate([np.arange(-70, 71), [-C_MAX, C_MAX, 0x1fff, -0x2000, 0x2000], rng.integers(-C_MAX, C_MAX + 1, 100)])
    x1, sh = _tables(qs)
    orig, lo, hi = _interval(cs[None, :], qs[:, None], x1[:, None], sh[:, None])
    for i, q in enumerate(qs):
        for j, c in enumerate(cs):
            assert o.interval(int(c), int(q)) == (orig[i, j], lo[i, j], hi[i, j]), (c, q)


@pytest.mark.parametrize("q0", range(1, 0x800, 256))   # (256 quantisers a case: memory)
def test_only_the_outward_bound_can_bind(q0):
    c = np.arange(-C_MAX, C_MAX + 1, dtype=np.int64)[None, :, None]
    qs = np.arange(q0, min(q0 + 256, 0x800), dtype=np.int64)
    x1, sh = _tables(qs)
    q, x1, sh = qs[:, None, None], x1[:, None, None], sh[:, None, None]
    mul = np.array(MULS, np.int64)[None, None, :]
    orig, lo, hi = _interval(c, q, x1, sh)
    assert (orig * c >= 0).all(), "c and orig differ in sign"
    assert ((lo <= c) & (c <= hi)).all(), "c outside its own interval"
    b = _outward_bound(c, q, x1, sh)
    assert (b == np.where(c < 0, lo, hi))[np.broadcast_to(c != 0, b.shape)].all(), "b is not the bound on the far side of zero"
    exact = c * mul + 0x1000
    v = exact >> 13
    want = np.minimum(np.maximum(v, lo), hi)                # the reference's two-sided clamp
    assert (np.where(c > 0, v >= lo, v <= hi) | (c == 0)).all(), "the inward bound binds"
    got = v + b + c - np.maximum(np.maximum(v, b), c) - np.minimum(np.minimum(v, b), c)   # v_med3_i32: the median
    assert np.array_equal(got, want)
    # what the kernel executes is the wrapping 32-bit product: identical as long as mul <= QS_REB_MUL_MAX
    small = np.broadcast_to(mul <= QS_REB_MUL_MAX, exact.shape)
    assert (np.abs(exact[small]) < 2**31).all() and np.array_equal(_wrap32(exact)[small], exact[small])


def test_wrapped_product_beyond_the_checked_mul_breaks_the_lemma():
    """c = 5, quantiser 4 (interval [2, 5] around 4), mul = 2^31 - 1: the 32-bit product wraps to 2^31 - 5 and the rounding
    constant carries it below zero -- the two-sided clamp answers lo = 2, the median of {v, hi, c} would answer 5.  The
    kernel's check of mul keeps such a wave on the two-sided loop."""
    c, q, mul = 5, 4, 2**31 - 1
    x1, sh = _tables([q])
    orig, lo, hi = (int(x[0]) for x in _interval(np.int64(c), np.int64(q), x1, sh))
    assert (orig, lo, hi) == (4, 2, 5)
    v = int(_wrap32(int(_wrap32(c * mul)) + 0x1000)) >> 13
    assert v < 0 and min(max(v, lo), hi) == 2 and sorted((v, hi, c))[1] == 5
    assert mul > QS_REB_MUL_MAX
