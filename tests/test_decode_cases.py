"""The decode edge cases (tests/decode_cases.py) without a device: that the cases have the properties the GPU tests rely
on, and the product's own decode arithmetic (csrc/qs_decode.h through tests/decode_host.cpp, compiled for the host)
byte for byte against libjpeg 9 on them -- the 32-bit and the 64-bit pass 1 on both sides of QS_DEC_FAST_BOUND, and
the colour conversion over every (Cb, Cr) pair."""
import numpy as np
import pytest

import decode_cases as dc
from decode_oracle import LibJpeg9, blocks_needed

KINDS = ("islow", "16x16", "16x8", "8x16")


@pytest.fixture(scope="module")
def lj9(tmp_path_factory):
    return LibJpeg9(tmp_path_factory.mktemp("lj9"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return dc.DecodeHost(tmp_path_factory.mktemp("dechost"))


@pytest.fixture(scope="module")
def grid(lj9):
    """libjpeg 9's pixels of the 4:4:4 colour grid, one image per luma value"""
    out = {}
    for y in dc.GRID_Y:
        im = dc.colour_grid(y)
        out[y] = lj9.decode(im["coefs"], im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"])
    return out


def test_the_bound_is_the_one_the_cases_straddle(host):
    info = host.info()
    assert info["fast_bound"] == dc.BOUND == dc.header_constant("QS_DEC_FAST_BOUND")
    assert (info["tile_w"], info["tile_h"]) == (dc.TILE_W, dc.TILE_H)


def test_pass1_l1_norms_and_the_limits_they_imply(host):
    """the largest row L1 norm of each pass-1 matrix (unit vectors through qd_idct8/16<int64_t>), the largest |dq| at
    which every final sum + 2^10 still fits int32, and that QS_DEC_FAST_BOUND lies below both"""
    info = host.info()
    assert (info["l1_8"], info["l1_16"]) == (61214, 81678)
    limit = {n: (2 ** 31 - 1 - 2 ** 10) // info[f"l1_{n}"] for n in (8, 16)}
    assert limit == {8: 35081, 16: 26292}
    assert info["fast_bound"] <= min(limit.values())


@pytest.mark.parametrize("kind", KINDS)
def test_bound_blocks_sit_on_both_sides_of_the_bound(kind):
    groups = dc.bound_blocks(kind)
    mx = np.concatenate([g["mx"] for g in groups])
    for g in groups:
        assert np.array_equal(g["mx"], np.abs(g["coefs"].astype(np.int64) * g["table"].astype(np.int64)).max(axis=1))
        assert len(g["labels"]) == len(g["coefs"])
    assert (mx == dc.BOUND).sum() >= 16 and (mx == dc.BOUND + 1).sum() >= 16
    for a in (8192, 16383, 20000, 26292, 26293, 32767, 35081, 35082, 65535):
        assert (mx == a).sum() >= 2 * dc.PASS1_POINTS[kind], a
    # the aligned blocks carry the signs of the DCT basis: column c of the block of row i is +-A * sign(cos(...))
    points = dc.PASS1_POINTS[kind]
    g = groups[0]
    for i in range(points):
        blk = g["coefs"][2 * i].reshape(8, 8)              # amplitude 8192, all columns, sign +
        want = np.sign(np.cos((2 * i + 1) * np.arange(8) * np.pi / (2 * points)))
        assert (blk == 8192 * want[:, None]).all()


@pytest.mark.parametrize("hs,vs", list(dc.KIND_OF))
def test_every_tile_of_a_bound_image_holds_fast_and_slow_blocks(hs, vs):
    for im in dc.bound_images(hs, vs):
        w, h = im["image_size"]
        assert w % dc.TILE_W == 0 and h % dc.TILE_H == 0
        for ci, (g, idx) in enumerate(zip(im["groups"], im["index"])):
            assert idx.shape == blocks_needed(im["image_size"], im["hsamp"], im["vsamp"], ci)
            assert set(idx.reshape(-1).tolist()) == set(range(len(g["coefs"]))), "a block of the group is missing"
            assert np.array_equal(im["coefs"][ci], g["coefs"][idx])
            ph, pw = (8 * vs, 8 * hs) if ci else (8, 8)
            th, tw = dc.TILE_H // ph, dc.TILE_W // pw      # blocks of this component per tile
            fast = (g["mx"][idx] <= dc.BOUND).reshape(idx.shape[0] // th, th, idx.shape[1] // tw, tw)
            per_tile = fast.transpose(0, 2, 1, 3).reshape(-1, th * tw)
            assert (per_tile.any(axis=1) & ~per_tile.all(axis=1)).all(), f"component {ci}: a tile lies on one side"


@pytest.mark.parametrize("kind", KINDS + ("32x8",))
def test_host_idct_equals_libjpeg_on_the_bound_blocks(lj9, host, kind):
    """qd_idct_block<W16, H16, XREP>, fast path and slow path, against jpeg_idct_<kind> of libjpeg 9"""
    ref_kind = "16x8" if kind == "32x8" else kind
    groups = dc.bound_blocks(ref_kind)
    everything = []
    for g in groups:
        tables = np.broadcast_to(g["table"], g["coefs"].shape)
        want = lj9.blocks(ref_kind, g["coefs"], tables)
        if kind == "32x8":
            want = np.repeat(want, 2, axis=2)
        got = host.blocks(kind, g["coefs"], tables)
        bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
        assert not len(bad), f"{len(bad)} blocks differ, first: {g['labels'][bad[0]]}, max|dq| {int(g['mx'][bad[0]])}"
        everything.append(want.reshape(-1))
    # libjpeg's own output over these cases is not degenerate
    px = np.concatenate(everything)
    assert (px == 0).any() and (px == 255).any()
    assert len(np.unique(px[(px > 0) & (px < 255)])) > 50


def test_chunk_batch_crosses_two_chunk_borders():
    chunk = dc.header_constant("QS_DEC_CHUNK")
    ims = dc.chunk_batch(91)
    assert [len(ims[j:j + chunk]) for j in range(0, len(ims), chunk)] == [chunk, chunk, 3]
    lay = dc.layouts()
    assert len(lay) == 10
    sizes = [im["image_size"] for im in ims]
    for k, im in enumerate(ims):
        assert (im["hsamp"], im["vsamp"], im["colorspace"]) == (list(lay[k % 10][0]), list(lay[k % 10][1]), lay[k % 10][2])
        assert 1 <= sizes[k][0] <= 40 and 1 <= sizes[k][1] <= 40
    assert (1, 1) in sizes and (40, 40) in sizes
    tiles = [dc.tile_count(s) for s in sizes]
    assert all(a != b for a, b in zip(tiles, tiles[1:]))
    assert len({(tuple(im["hsamp"]), im["colorspace"], im["image_size"]) for im in ims}) > 80      # differing sizes


def test_padded_arrays_cut_back_equal_the_original():
    rng = np.random.default_rng(5)
    for hs, vs, cs in dc.layouts():
        im = dc.synth_image(rng, (67, 131), hs, vs, cs)
        extras = [tuple(zip(*dc.mcu_extra(im))), (3, 2)]
        assert any(any(e) for e in extras[0]) or len(hs) == 1 or (hs[0], vs[0]) == (1, 1)
        for ew, eh in extras:
            p = dc.padded(im, ew, eh)
            for ci, (a, b) in enumerate(zip(p["coefs"], im["coefs"])):
                hb, wb = blocks_needed(im["image_size"], hs, vs, ci)
                assert b.shape[:2] == (hb, wb) and a.dtype == np.int16
                assert np.array_equal(a[:hb, :wb], b)
                rest = np.ones(a.shape[:2], bool)
                rest[:hb, :wb] = False
                assert (np.abs(a[rest].astype(np.int32)) == 32767).all()
        p = dc.padded(im, 3, 2)
        assert all(a.shape[:2] == (b.shape[0] + 2, b.shape[1] + 3) for a, b in zip(p["coefs"], im["coefs"]))


def test_edge_sizes_meet_every_width_and_height_in_every_layout():
    ims = dc.edge_sizes()
    lay = dc.layouts()
    assert len(ims) == 8 * len(lay)
    for li, (hs, vs, cs) in enumerate(lay):
        mine = ims[8 * li:8 * li + 8]
        assert all((im["hsamp"], im["vsamp"], im["colorspace"]) == (list(hs), list(vs), cs) for im in mine)
        assert {im["image_size"][0] for im in mine} == set(dc.EDGE_WIDTHS)
        assert {im["image_size"][1] for im in mine} == set(dc.EDGE_HEIGHTS)
        assert mine[0]["image_size"] == (1, 1)


def test_colour_grid_enumerates_every_chroma_pair_and_is_flat(grid):
    for y in dc.GRID_Y:
        im = dc.colour_grid(y)
        pairs = (im["coefs"][1][:, :, 0].astype(np.int64) + 128) * 256 + im["coefs"][2][:, :, 0] + 128
        assert len(np.unique(pairs)) == 65536
        assert all((c[:, :, 1:] == 0).all() for c in im["coefs"]) and all(q[0] == 8 for q in im["quants"])
        px = grid[y]
        assert px.shape == (2048, 2048, 3)
        assert np.array_equal(px, np.repeat(np.repeat(px[::8, ::8], 8, axis=0), 8, axis=1)), "a DC-only block is not flat"
    allpx = np.stack([grid[y][::8, ::8] for y in dc.GRID_Y])
    for ch in range(3):
        assert (allpx[..., ch] == 0).any() and (allpx[..., ch] == 255).any(), f"channel {ch} never clamps"
    im = dc.colour_grid_420()
    pairs = (im["coefs"][1][:, :, 0].astype(np.int64) + 128) * 256 + im["coefs"][2][:, :, 0] + 128
    assert len(np.unique(pairs)) == 65536
    assert set(np.unique(im["coefs"][0][:, :, 0] + 128).tolist()) == set(dc.GRID_Y)


def test_host_colour_conversion_equals_libjpeg_on_every_chroma_pair(host, grid):
    """qd_ycc_rgb over the whole grid: the flat sample 128 + c of each DC-only block is its (Y, Cb, Cr)"""
    cb, cr = np.meshgrid(np.arange(256), np.arange(256))   # Cb = block column, Cr = block row
    for y in dc.GRID_Y:
        ycc = np.stack([np.full(65536, y), cb.reshape(-1), cr.reshape(-1)], axis=1).astype(np.uint8)
        got = host.ycc_rgb(ycc).reshape(256, 256, 3)
        want = grid[y][::8, ::8]
        bad = np.argwhere((got != want).any(axis=2))
        assert not len(bad), (f"Y {y}: {len(bad)} pairs differ, first (Cb, Cr) = ({bad[0][1]}, {bad[0][0]}): "
                              f"{got[tuple(bad[0])]} != libjpeg {want[tuple(bad[0])]}")
