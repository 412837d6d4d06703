"""Coefficient arrays whose AC histogram is prescribed symbol by symbol, so that Huffman's procedure builds a tree of a
chosen depth on the scan's own statistics: what the whole-file coder needs to meet the cut-back of figure K.3 (code
sizes 17 .. 32) and libjpeg's refusal (above 32) from arrays rather than from synthetic histograms.  numpy only.

The counts of a chain of n symbols are 1, 2, 3, 5, 8, 13, ... (a_k = a_(k-1) + a_(k-2)).  With libjpeg's reserved symbol
(count 1) the running tree's sum is a_(k+2) - 1 after symbol k joined it: more than a_(k+1), less than a_(k+2), so every
merge takes the running tree and the next leaf and the largest code size is n.  The chain has no slack -- these are the
smallest counts that reach the depth -- so every count is hit exactly; the users assert that on the realised arrays
with the suite's own restatements (huff_oracle.code_sizes, encode_oracle.histogram), never on this file's word.

Symbols: the heavy counts go to the run-0 symbols (0, s), s = 1 .. 10, one rank near the eighth largest to EOB and the
light counts to (r, s) with r = 1 .. 5.  Block kinds: blocks that hold the light symbols, topped up to 63 positions
with run-0 symbols; "short" blocks of 62 run-0 symbols and EOB (where the parity of the three-component form asks for
it, one or two of 61); full blocks of 63 run-0 symbols; blocks of DC alone (one EOB).

The EOB count is the short blocks plus the blocks of DC alone (plus, in the three-component form, the blocks of Cr).
So the short blocks are chosen congruent to minus the remaining run-0 symbols mod 63, which leaves no partial block,
and then stepped by 63 until the block total is a whole number of rows of an odd width: no padding blocks."""
import functools

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])
_NBITS = np.zeros(32769, np.uint8)                                  # bit length of a magnitude
for _s in range(1, 17):
    _NBITS[1 << (_s - 1):min(1 << _s, 32769)] = _s


def chain_counts(n):
    """1, 2, 3, 5, 8, ...: n counts, rising"""
    a = [1, 2]
    while len(a) < n:
        a.append(a[-1] + a[-2])
    return a[:n]


def prescribed_histogram(depth, seed=0, eob_rank=7):
    """{symbol: count} of the table under test: ranks 0 .. 10 from the top without eob_rank to the ten run-0 symbols, rank
    eob_rank to EOB, the rest to seeded picks among (r, s), r = 1 .. 5, s = 1 .. 10"""
    assert 12 <= depth <= 61
    rng = np.random.default_rng(1000 * depth + seed)
    falling = chain_counts(depth)[::-1]
    heavy = [k for k in range(11) if k != eob_rank]
    run0 = rng.permutation(np.arange(1, 11))
    light = rng.permutation(np.array([(r << 4) | s for r in range(1, 6) for s in range(1, 11)]))[:depth - 11]
    h = {0: falling[eob_rank]}
    for k, s in zip(heavy, run0):
        h[int(s)] = falling[k]
    for k, sym in zip(range(11, depth), light):
        h[int(sym)] = falling[k]
    assert len(h) == depth and sum(h.values()) == sum(falling)
    return h


def _values(rng, sizes):
    """a random value of each size class, random sign"""
    sizes = np.asarray(sizes, np.int64)
    lo = np.int64(1) << (sizes - 1)
    v = lo + (rng.random(len(sizes)) * lo).astype(np.int64)         # [2^(s-1), 2^s - 1]
    return np.where(rng.random(len(sizes)) < 0.5, -v, v).astype(np.int16)


def _solve(light_positions, nlight, run0, eob, ycc, spread=(2, 16)):
    """-> (blocks with light symbols, blocks of 61 run-0 symbols and EOB, short, full, DC-alone, width in blocks); widths
    near the square root first, then (small arrays have few choices) any odd width of at least 7 that leaves two rows.
    With ycc twice the block total is the blocks without an EOB plus the EOB count, and stepping the short blocks by 63
    keeps that sum's parity: one block of 61 run-0 symbols instead of 62 shifts the congruence and with it the parity.

    Worked for the gray array of depth 17 (6642 run-0 symbols, 32 light symbols on 144 positions, 89 EOBs): ten light
    symbols to a block make nm = 4 blocks with 4 * 63 - 144 = 108 positions to top up, which leaves rest = 6534 run-0
    symbols for short and full blocks: 62 ns + 63 nf = 6534.  Mod 63 that reads -ns = 6534 = 45, so ns = 18, 81, ...
    ns = 18 gives nf = 86, nz = 89 - 18 = 71 blocks of DC alone and 179 blocks in all, a prime; ns = 81 gives nf = 24,
    nz = 8 and 4 + 81 + 24 + 8 = 117 = 13 rows of 9"""
    for far, n61, per in [(f, e, p) for f in spread for e in (0, 1, 2) for p in (10, 9, 8, 7, 6, 5)]:
        nm = -(-nlight // per)
        rest = run0 - (63 * nm - light_positions) - 61 * n61
        if rest < 0:
            continue
        ns = -rest % 63
        while 62 * ns <= rest:
            nf = (rest - 62 * ns) // 63
            if ycc:                                                 # Cr's blocks each bring an EOB of their own
                total, odd = divmod(nm + nf + eob, 2)
                nz = -1 if odd else eob - ns - n61 - total
            else:
                nz = eob - ns - n61
                total = nm + n61 + ns + nf + nz
            if nz >= 0:
                root = int(total ** 0.5)
                for wb in sorted(range(max(7, root // far) | 1, max(9, far * root), 2), key=lambda w: abs(w - root)):
                    if total % wb == 0 and total // wb >= 2:
                        return nm, n61, ns, nf, nz, wb
            ns += 63
    raise AssertionError("no block layout with these counts")


def crafted_blocks(hist, rng, ycc=False):
    """the prescribed {symbol: count} -> int16 (hb, wb, 64) in natural order, shuffled, DC random in [-1000, 1000]; with
    ycc as many EOBs are left out as the array has blocks (Cr brings them)"""
    light = np.repeat([s for s in hist if s >> 4], [hist[s] for s in hist if s >> 4]).astype(np.int64)
    run0 = np.repeat([s for s in hist if 0 < s < 16], [hist[s] for s in hist if 0 < s < 16]).astype(np.int64)
    rng.shuffle(light)
    rng.shuffle(run0)
    positions = int(((light >> 4) + 1).sum())
    nm, n61, ns, nf, nz, wb = _solve(positions, len(light), len(run0), hist[0], ycc)
    per = -(-len(light) // nm)
    total = nm + n61 + ns + nf + nz
    z = np.zeros((total, 64), np.int16)                             # zigzag order
    # the blocks with light symbols: `per` of them in front (r zeros, then the value), run-0 symbols up to position 63
    pad = nm * per - len(light)
    runs = np.concatenate([light >> 4, np.full(pad, -1)]).reshape(nm, per)        # (a missing one takes no position)
    vals = np.concatenate([_values(rng, light & 15), np.zeros(pad, np.int16)]).reshape(nm, per)
    at = np.cumsum(runs + 1, axis=1)
    rows = np.repeat(np.arange(nm), per).reshape(nm, per)
    z[rows[runs >= 0], at[runs >= 0]] = vals[runs >= 0]
    used = at[:, -1]
    fill = np.arange(64)[None, :] > used[:, None]
    ntop = int(fill.sum())
    assert ntop == 63 * nm - positions and ntop + 61 * n61 + 62 * ns + 63 * nf == len(run0)
    v0 = _values(rng, run0)
    z[:nm][fill] = v0[:ntop]
    cut = np.cumsum([ntop, 61 * n61, 62 * ns, 63 * nf])
    row = np.cumsum([nm, n61, ns, nf])
    z[row[0]:row[1], 1:62] = v0[cut[0]:cut[1]].reshape(n61, 61)
    z[row[1]:row[2], 1:63] = v0[cut[1]:cut[2]].reshape(ns, 62)
    z[row[2]:row[3], 1:64] = v0[cut[2]:cut[3]].reshape(nf, 63)
    z = z[rng.permutation(total)]
    z[:, 0] = rng.integers(-1000, 1001, total)
    nat = np.empty_like(z)
    nat[:, ZIGZAG] = z
    return nat.reshape(total // wb, wb, 64)


def deep_image(depth, seed=0, ycc=False):
    """the image dict (coefs, quants all ones, hsamp, vsamp, colorspace, image_size) whose AC table under test -- AC 0 of
    a gray image, or with ycc AC 1 of a 4:4:4 YCbCr image with the crafted blocks in Cb, ordinary Y and a Cr of DC alone --
    gets a Huffman tree of `depth` levels; the size is no multiple of 8"""
    rng = np.random.default_rng(7000 * depth + seed + (500 if ycc else 0))
    blocks = crafted_blocks(prescribed_histogram(depth, seed, eob_rank=6 if ycc else 7), rng, ycc)
    hb, wb = blocks.shape[:2]
    coefs = [blocks]
    if ycc:
        y = rng.integers(-40, 41, (hb, wb, 64))                     # encode_oracle.synth_scan_image's statistics
        y[rng.random((hb, wb, 64)) > 0.35] = 0
        y[rng.random((hb, wb)) < 0.1, 1:] = 0
        tail = rng.random((hb, wb)) < 0.3
        y[tail, 1:60] = 0
        y[tail, 63] = rng.integers(1, 1024, int(tail.sum()))
        y[..., 0] = rng.integers(-1000, 1001, (hb, wb))
        cr = np.zeros((hb, wb, 64), np.int16)
        cr[..., 0] = rng.integers(-1000, 1001, (hb, wb))
        coefs = [y.astype(np.int16), blocks, cr]
    n = len(coefs)
    return dict(coefs=coefs, quants=[np.ones(64, np.uint16) for _ in range(n)], hsamp=[1] * n, vsamp=[1] * n,
                colorspace=3 if ycc else 1, image_size=(8 * wb - 3, 8 * hb - 5))


@functools.lru_cache(maxsize=None)
def shared_deep_image(depth, ycc=False):
    """deep_image(depth, 0, ycc), built once per process: the large ones take seconds and tens of megabytes, and more
    than one module uses them.  Read only: whoever plants something copies the array first"""
    im = deep_image(depth, 0, ycc)
    for c in im["coefs"]:
        c.setflags(write=False)
    return im


def ac_histogram(im, comps=(0,), chunk=1 << 16):
    """the 256 AC symbol counts of the scan's blocks of the given components (a gray scan: component 0), vectorised;
    valid where the arrays hold exactly the scan's blocks (no dummy blocks: one component, or every factor 1)"""
    h = np.zeros(256, np.int64)
    k = np.arange(1, 64, dtype=np.int16)
    for ci in comps:
        blocks = im["coefs"][ci].reshape(-1, 64)
        for first in range(0, len(blocks), chunk):
            z = blocks[first:first + chunk][:, ZIGZAG[1:]]
            nz = z != 0
            pos = np.where(nz, k[None, :], np.int16(0))
            last = np.maximum.accumulate(pos, axis=1)               # position of the last value up to here
            before = np.concatenate([np.zeros((len(z), 1), np.int16), last[:, :-1]], axis=1)
            run = (k[None, :] - before - 1)[nz].astype(np.int64)
            size = _NBITS[np.abs(z[nz].astype(np.int32))].astype(np.int64)
            h += np.bincount(((run & 15) << 4) | size, minlength=256)[:256]
            h[0xF0] += int((run >> 4).sum())
            h[0] += int((last[:, -1] != 63).sum())
    return h


def dc_histogram(im, comps=(0,)):
    """the 16 counts of the DC-difference sizes of a scan without restarts, per component in raster order (the same
    validity as ac_histogram)"""
    h = np.zeros(16, np.int64)
    for ci in comps:
        dc = im["coefs"][ci].reshape(-1, 64)[:, 0].astype(np.int64)
        h += np.bincount(_NBITS[np.abs(np.diff(dc, prepend=0))], minlength=16)[:16]
    return h
