"""What the tests of the optimal-table procedure (csrc/qs_huff.h) share: a restatement of libjpeg's
jpeg_gen_optimal_table that walks the others[] chains as jchuff.c does, the histograms both the CPU and the GPU tests
run, and the host build of the header (tests/huff_host.cpp)."""
import struct

import numpy as np

from host_tools import Tool, build

MAX_CLEN = 32
_BIG = np.int64(1) << 62


def code_sizes(freq256):
    """Huffman's procedure as jchuff.c carries it out: freq[256] = 1, c1 = the least count (the larger index in a tie), c2
    the same without c1, the sums kept under c1, and the code size of every member of both trees raised by walking their
    others[] chains -> the 257 code sizes"""
    freq = np.zeros(257, np.int64)
    freq[:256] = np.asarray(freq256, np.int64)[:256]
    freq[256] = 1
    codesize, others = [0] * 257, [-1] * 257
    while True:
        fl = np.where(freq > 0, freq, _BIG)
        v = fl.min()
        if v == _BIG:
            break
        c1 = int(np.flatnonzero(fl == v)[-1])
        fl[c1] = _BIG
        v = fl.min()
        if v == _BIG:
            break
        c2 = int(np.flatnonzero(fl == v)[-1])
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    return codesize


def libjpeg_optimal(freq256):
    """-> (bits[17], huffval) as libjpeg 9d's jpeg_gen_optimal_table leaves them, or None where it stops with
    JERR_HUFF_CLEN_OVERFLOW (a code size above 32)"""
    sizes = code_sizes(freq256)
    if max(sizes) > MAX_CLEN:
        return None
    bits = [0] * (MAX_CLEN + 1)
    for s in sizes:
        if s:
            bits[s] += 1
    for i in range(MAX_CLEN, 16, -1):                                   # figure K.3
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while i > 0 and bits[i] == 0:                                       # (libjpeg never gets here with nothing counted)
        i -= 1
    if i > 0:
        bits[i] -= 1
    f = [int(v) for v in list(freq256)[:256]]
    vals = sorted((s for s in range(256) if f[s]), key=lambda s: (-f[s], s))
    return bits[:17], vals


def spread(seed):
    """floor(exp(20 u)) on about half the symbols"""
    rng = np.random.default_rng(seed)
    h = np.floor(np.exp(20 * rng.random(256))).astype(np.int64)
    h[rng.random(256) < 0.5] = 0
    return h


def find_spread(want, start=0, tries=4000):
    """the first seeded spread whose largest code size satisfies `want`"""
    for seed in range(start, start + tries):
        h = spread(seed)
        if want(max(code_sizes(h))):
            return h
    raise AssertionError("no such histogram among the seeded spreads")


def edge_histograms():
    """[(name, counts[256])]"""
    one, two = np.zeros(256, np.int64), np.zeros(256, np.int64)
    one[37] = 5
    two[3], two[200] = 9, 9
    return [("all zero", np.zeros(256, np.int64)), ("one symbol", one), ("two symbols", two),
            ("256 equal", np.full(256, 7, np.int64)), ("all ones", np.ones(256, np.int64)),
            ("all 2^32 - 1", np.full(256, 2 ** 32 - 1, np.int64)),
            ("cut back", find_spread(lambda m: 17 <= m <= 32)), ("above 32", find_spread(lambda m: m > 32))]


def seeded_histograms(n, seed):
    """n histograms of the kinds that stress the procedure: small ties, sparse, exponential spreads, Fibonacci-like"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        kind = k % 5
        h = np.zeros(256, np.int64)
        if kind == 0:                                                   # small counts: ties everywhere
            h = rng.integers(0, 4, 256)
        elif kind == 1:                                                 # sparse
            idx = rng.choice(256, int(rng.integers(1, 12)), replace=False)
            h[idx] = rng.integers(1, 1000, len(idx))
        elif kind == 2:                                                 # exponential spread
            h = np.floor(np.exp(20 * rng.random(256))).astype(np.int64)
            h[rng.random(256) < 0.5] = 0
        elif kind == 3:                                                 # Fibonacci-like: the deepest trees
            m = int(rng.integers(5, 47))
            fib = [1, int(rng.integers(1, 3))]
            while len(fib) < m:
                fib.append(fib[-1] + fib[-2])
            idx = rng.choice(256, m, replace=False)
            h[idx] = np.minimum(np.array(fib, np.int64) + (rng.integers(0, 2, m) if k % 2 else 0), 2 ** 32 - 1)
        else:                                                           # what a scan gives: a few heavy symbols, a long tail
            h = (rng.pareto(0.7, 256) * rng.integers(1, 50)).astype(np.int64)
            h = np.minimum(h, 2 ** 32 - 1)
        out.append(np.asarray(h, np.int64))
    return out


class HuffHost(Tool):
    """tests/huff_host.cpp: the table procedure of csrc/qs_huff.h in its host form, as a process"""
    SILENT = True

    def __init__(self, workdir, sanitize=False):
        super().__init__(build("huff_host.cpp", sanitize=sanitize), workdir)

    def run(self, hists):
        """[counts[256]] -> [(status, bits[17], huffval: the first sum(bits) symbols, rest: the bytes behind them)];
        fails on a non-zero exit or anything on stderr (a sanitizer report)"""
        src, dst = self.tmp(".bin"), self.tmp(".out")
        src.write_bytes(struct.pack("<i", len(hists)) + b"".join(np.asarray(h, np.uint32)[:256].tobytes() for h in hists))
        self._run("run", src, dst)
        b = dst.read_bytes()
        src.unlink()
        dst.unlink()
        assert len(b) == len(hists) * (4 + 17 + 256)
        out = []
        for k in range(len(hists)):
            off = k * 277
            bits = list(b[off + 4:off + 21])
            vals = list(b[off + 21:off + 277])
            out.append((struct.unpack_from("<i", b, off)[0], bits, vals[:sum(bits)], vals[sum(bits):]))
        return out
