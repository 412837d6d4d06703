"""Progressive files with refinement scans (Ah > 0) before any GPU is involved: libjpeg 9 itself writes the files
(tests/libjpeg9_encode.c); the plain Python restatement of tests/encode_refine_oracle.py and the host build of
csrc/qs_encode_prog.h (tests/encode_refine_host.cpp, plain and under ASan + UBSan as a program of its own) are pinned to
them, whole file; crafted images put every rule of the AC refinement's EOB runs to work; libjpeg and Pillow read the files
back; jpeg_file.simple_progression is libjpeg's jpeg_simple_progression.  DESIGN.md section 17.1."""
import io

import numpy as np
import pytest

import jpegqs_pkg
from decode_oracle import LibJpeg9
from encode_oracle import LAYOUTS, LibjpegError
from encode_prog_oracle import BAD_SCRIPTS, PROG_SIZES, RESTARTS, LibJpeg9EncProg, complete, grid_images, scan_summary
from encode_refine_oracle import (GRAY_REFINE, RefineHost, big_crafted_images, crafted_images, encode_refine,
                                  libjpeg_simple_progression, refine_scripts, run_pieces)
from encode_rst_oracle import RST_LAYOUTS

pkg = jpegqs_pkg.load()
jpeg_file = pkg.jpeg_file

SCRIPT_NAMES = ("simple", "dc twice", "ac two steps", "dc per component")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return LibJpeg9EncProg(tmp_path_factory.mktemp("lj9prog"))


@pytest.fixture(scope="module")
def lj9(tmp_path_factory):
    return LibJpeg9(tmp_path_factory.mktemp("lj9"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return RefineHost(tmp_path_factory.mktemp("refhost"))


@pytest.fixture(scope="module")
def host_san(tmp_path_factory):
    return RefineHost(tmp_path_factory.mktemp("refhost_san"), sanitize=True)


@pytest.fixture(scope="module")
def images():
    return grid_images()


def _head(im):
    return jpeg_file.compose_parts(im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"], progressive=True)[0]


def _scripts(im):
    return refine_scripts(len(im["coefs"]), im["colorspace"], jpeg_file.simple_progression)


@pytest.fixture(scope="module")
def written(prog, images):
    """{(layout, size, script name, restart): libjpeg's file}: the whole grid, written once"""
    out = {}
    for (li, size), im in images.items():
        for name, script in _scripts(im).items():
            for rst in RESTARTS:
                out[(li, size, name, rst)] = prog.write(im, script, *rst)
    assert len(out) == len(RST_LAYOUTS) * len(PROG_SIZES) * len(SCRIPT_NAMES) * len(RESTARTS)
    return out


def test_simple_progression_is_libjpegs(tmp_path):
    """jpeg_file.simple_progression against cinfo.scan_info after jpeg_simple_progression: 1, 3 (YCbCr and RGB) and 4
    components (CMYK and YCCK)"""
    for ncomp, cs in ((1, 1), (3, 3), (3, 2), (4, 4), (4, 5)):
        want = libjpeg_simple_progression(tmp_path, ncomp, cs)
        assert jpeg_file.simple_progression(ncomp, cs) == want, (ncomp, cs)
        assert len(want) == (10 if (ncomp, cs) == (3, 3) else 2 + 4 * ncomp)
        assert jpeg_file.validate_script(want, ncomp) is False         # valid, with refinement scans
    ten = jpeg_file.simple_progression(3, 3)
    assert [s for s in ten if s[3] > 0] == [((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0),
                                            ((0,), 1, 63, 1, 0)]
    assert ten[0] == ((0, 1, 2), 0, 0, 0, 1)


def test_the_python_restatement_equals_libjpeg(written, images):
    for key, want in written.items():
        im = images[key[:2]]
        assert encode_refine(im, _scripts(im)[key[2]], _head(im), *key[3]) == want, key


def test_the_host_build_equals_libjpeg(written, images, host):
    for key, want in written.items():
        im = images[key[:2]]
        assert host.write(im, _scripts(im)[key[2]], _head(im), *key[3]) == want, key


def test_the_host_build_under_sanitizers(written, images, host_san):
    """the same program with -fsanitize=address,undefined, every array in an allocation of its own: the whole grid"""
    n = 0
    for key, want in written.items():
        im = images[key[:2]]
        assert host_san.write(im, _scripts(im)[key[2]], _head(im), *key[3]) == want, key
        n += 1
    assert n == len(RST_LAYOUTS) * len(PROG_SIZES) * 4 * len(RESTARTS) == 784
    assert host_san.bounds().startswith("bounds ok")


def test_the_bounds_of_the_refinement_coders(host, hip):
    """the per-block worst cases the header states are reached by construction, and they size the workspace and
    max_body_bytes: an AC refinement scan of 256 blocks takes 256 * (63 * 17 + 14) bits of stream where the first scan of
    the band takes 256 * (63 * 26 + 30)"""
    assert host.bounds().startswith("bounds ok: AC refinement 1..63 1085 bits, DC refinement 1 bit, a piece has at least 15 blocks")
    im = crafted_images()["be cut"]
    im = dict(im, coefs=[np.zeros((1, 256, 64), np.int16)], image_size=(2048, 8))
    job, _keep = hip._make_job(im["coefs"], im["quants"], hsamp=[1], vsamp=[1], colorspace=1, image_size=(2048, 8))
    first = [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1)]
    (i1,), ws1, _sc = hip.encode_progressive_info([job], [hip.prog_opts(first, refinement=True)])
    (i2,), ws2, _sc = hip.encode_progressive_info([job], [hip.prog_opts(GRAY_REFINE, refinement=True)])

    def stream(bits):
        return -(-(256 * bits // 8 + 16) // 256) * 256
    # refining the bands 1-63 and 1-5: every other array of the two workspaces has the same size (256 blocks, at most 32
    # stuffing units), so they differ by exactly the bound's difference
    narrow = GRAY_REFINE[:2] + [((0,), 1, 5, 1, 0)]
    (_i,), ws_narrow, _sc = hip.encode_progressive_info([job], [hip.prog_opts(narrow, refinement=True)])
    assert stream(63 * 17 + 14) == 34816 and ws2 - ws_narrow == stream(63 * 17 + 14) - stream(5 * 17 + 14) == 31488
    assert ws2 > ws1
    # per scan: every byte of the worst stream stuffed, the two largest DHT markers, DRI and the longest SOS (24 bytes)
    assert i2["max_body_bytes"] - i1["max_body_bytes"] == 2 * ((256 * 1085 + 7) // 8 + 1) + 2 * (21 + 256) + 24
    dc = [((0,), 0, 0, 0, 1), ((0,), 0, 0, 1, 0)]
    (i3,), _ws, _sc = hip.encode_progressive_info([job], [hip.prog_opts(dc, refinement=True)])
    (i4,), _ws, _sc = hip.encode_progressive_info([job], [hip.prog_opts(dc[:1])])
    assert i3["max_body_bytes"] - i4["max_body_bytes"] == 2 * ((256 * 1 + 7) // 8 + 1) + 2 * (21 + 256) + 24


def _check_crafted(prog, host, im, script, rst=(0, 0)):
    want = prog.write(im, script, *rst)
    assert encode_refine(im, script, _head(im), *rst) == want
    assert host.write(im, script, _head(im), *rst) == want
    return want


def test_the_cut_at_937_buffered_bits(prog, host):
    """16 blocks that each leave 63 correction bits: the run is cut behind block 15 (945 > 937); 937 bits exactly are not
    cut, 938 are; a restart boundary inside the run ends the piece first"""
    ims = crafted_images()
    scan = GRAY_REFINE[2]
    assert run_pieces(ims["be cut"], scan) == [(15, 945), (1, 63)]
    assert run_pieces(ims["be 937"], scan) == [(16, 937 + 63)]
    assert run_pieces(ims["be 938"], scan) == [(15, 938), (1, 63)]
    assert run_pieces(ims["be cut"], scan, 10) == [(10, 630), (6, 378)]
    assert run_pieces(ims["be 938"], scan, 15) == [(15, 938), (1, 63)]
    for name in ("be cut", "be 937", "be 938"):
        for rst in ((0, 0), (10, 0), (15, 0), (1, 0)):
            _check_crafted(prog, host, ims[name], GRAY_REFINE, rst)


def test_zero_runs_tails_and_heads(prog, host, host_san):
    """0xF0 followed by correction bits; zeros behind the last new coefficient folded into the run; a writing block
    whose last band coefficient is new, so that the next run starts behind it; pieces across workgroup borders"""
    ims = crafted_images()
    scan = GRAY_REFINE[2]
    im = ims["mixed"]
    from encode_refine_oracle import scan_symbols_refine
    syms = scan_symbols_refine(im, scan, 0)[0]
    zrl = [i for i, s in enumerate(syms) if s[1] == 0xF0]
    assert zrl and all(syms[i + 1][1] is None for i in zrl[:1])         # bits directly behind the first 0xF0
    pieces = run_pieces(im, scan)
    assert (15, 945) in pieces and any(n > 1 and bits < 938 for n, bits in pieces)
    for name in ("mixed", "border 264", "border 520"):
        for rst in ((0, 0), (7, 0), (256, 0), (0, 1)):
            want = _check_crafted(prog, host, ims[name], GRAY_REFINE, rst)
            assert host_san.write(ims[name], GRAY_REFINE, _head(ims[name]), *rst) == want
    for n in (264, 520):
        cuts, at = [], 0
        for length, _bits in run_pieces(ims[f"border {n}"], scan):
            at += length
            cuts.append(at)
        assert cuts                                                     # (positions inside the runs only: a sanity look)


def test_both_cuts_in_one_run(prog, host):
    """2048 x 1024, 32 768 blocks: the band all zero is one run cut at 0x7FFF; 2056 x 1024 with sparse tails: the count
    cuts the run's first piece, which carries 882 buffered bits, and the 937-bit rule cuts the rest every 15 blocks"""
    ims = big_crafted_images()
    scan = GRAY_REFINE[2]
    assert run_pieces(ims["all zero"], scan) == [(0x7FFF, 0), (1, 0)]
    pieces = run_pieces(ims["sparse tails"], scan)
    assert pieces == [(0x7FFF, 882)] + [(15, 945)] * 8 + [(9, 567)]
    for im in ims.values():
        _check_crafted(prog, host, im, GRAY_REFINE)
    _check_crafted(prog, host, ims["sparse tails"], GRAY_REFINE, (0, 40))


def test_complete_scripts_read_back(written, images, lj9, tmp_path):
    """every file of the grid (all four scripts end with every coefficient at Al = 0) is read back by libjpeg to the arrays
    that went in, and Pillow opens and decodes it and reports it as progressive"""
    from PIL import Image
    n = 0
    for key, data in written.items():
        li, size, name, rst = key
        im = images[(li, size)]
        assert complete(_scripts(im)[name], len(im["coefs"]))
        p = tmp_path / "f.jpg"
        p.write_bytes(data)
        back = lj9.read(p)
        for a, b in zip(back["coefs"], im["coefs"]):
            assert np.array_equal(a[:b.shape[0], :b.shape[1]], b), key
        with Image.open(io.BytesIO(data)) as pil:
            assert pil.info.get("progressive") and pil.info.get("progression"), key
            assert pil.size == tuple(size)
            pil.load()
        n += 1
    assert n == 784


def test_marker_layout_of_the_ten_scan_file(prog, images):
    """no DHT in front of the DC refinement, one AC DHT in front of each AC refinement, DRI as the existing rule gives it
    (when the scan's interval differs from the last one written)"""
    im = images[(4, (141, 93))]
    assert LAYOUTS[4][2] == 3 and len(im["coefs"]) == 3
    script = jpeg_file.simple_progression(3, 3)

    def layout(data):
        out = []
        for code, p in scan_summary(data):
            if code == 0xC4:
                out.append("DHT(%02x)" % p[0])
            elif code == 0xDD:
                out.append("DRI %d" % int.from_bytes(p, "big"))
            elif code == 0xDA:
                out.append("SOS(%d-%d %x)" % (p[-3], p[-2], p[-1]))
        return " ".join(out)
    plain = ("DHT(00) DHT(01) SOS(0-0 1) DHT(10) SOS(1-5 2) DHT(11) SOS(1-63 1) DHT(11) SOS(1-63 1) DHT(10) SOS(6-63 2) "
             "DHT(10) SOS(1-63 21) SOS(0-0 10) DHT(11) SOS(1-63 10) DHT(11) SOS(1-63 10) DHT(10) SOS(1-63 10)")
    assert layout(prog.write(im, script)) == plain
    hs, vs = im["hsamp"], im["vsamp"]
    rows = layout(prog.write(im, script, 0, 1))
    assert rows.count("DHT") == 10 and "SOS(1-63 21) DRI" in rows and rows.count("DRI") >= 4, (hs, vs, rows)
    assert encode_refine(im, script, _head(im), 0, 1) == prog.write(im, script, 0, 1)


def _verdict(hip, job, script, **kw):
    try:
        hip.encode_progressive_info([job], [hip.prog_opts(script, **kw)])
        return "ok", ""
    except pkg.QsHipError as e:
        return {-2: "EINVAL", -4: "ENOTSUP"}[e.code], str(e)


def test_the_flag_decides(hip, images, prog):
    """without QS_HIP_PROG_REFINE the refusal is today's message; with it the script is planned; a valid script of 380
    scans and a sequential script are QS_HIP_ENOTSUP with it too, what libjpeg refuses stays QS_HIP_EINVAL"""
    im = images[(4, (33, 18))]
    job, _keep = hip._make_job(im["coefs"], im["quants"], hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=3,
                               image_size=im["image_size"])
    script = jpeg_file.simple_progression(3, 3)
    assert hip.prog_opts(script).flags == 0 and hip.prog_opts(script, refinement=True).flags == 1
    v = _verdict(hip, job, script)
    assert v[0] == "ENOTSUP"
    assert v[1].endswith("qs_hip_encode_progressive_device_batch_info: job 0, scan 5: a refinement scan (Ah > 0): refinement scans "
                         "are not implemented")
    assert _verdict(hip, job, script, refinement=True)[0] == "ok"
    info, ws, sc = hip.encode_progressive_info([job], [hip.prog_opts(script, refinement=True)])
    assert info[0]["nscans"] == 10 and ws % 256 == 0 and sc % 256 == 0
    assert len(prog.write(im, script)) <= len(_head(im)) + info[0]["max_body_bytes"]
    long_script = [((0, 1, 2), 0, 0, 0, 1)] + [((c,), k, k, 0, 1) for c in range(3) for k in range(1, 64)] \
        + [((0, 1, 2), 0, 0, 1, 0)] + [((c,), k, k, 1, 0) for c in range(3) for k in range(1, 64)]
    assert len(long_script) == 380
    v = _verdict(hip, job, long_script, refinement=True)
    assert v[0] == "ENOTSUP" and "380 scans" in v[1] and "at most 256" in v[1]
    assert _verdict(hip, job, long_script[:256], refinement=True)[0] == "ok"
    sequential = [((0,), 0, 63, 0, 0), ((1,), 0, 63, 0, 0), ((2,), 0, 63, 0, 0)]
    assert _verdict(hip, job, sequential, refinement=True)[0] == "ENOTSUP"
    for name, make in BAD_SCRIPTS.items():
        assert _verdict(hip, job, make(3), refinement=True)[0] == "EINVAL", name
        with pytest.raises(LibjpegError):
            prog.write(im, make(3))
    # a refinement that skips a bit, and one of a coefficient never sent: libjpeg refuses them, flag or not
    for bad in ([((0, 1, 2), 0, 0, 0, 2), ((0, 1, 2), 0, 0, 2, 0)], [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 5, 1, 0)]):
        with pytest.raises(LibjpegError):
            prog.write(im, bad)
        assert _verdict(hip, job, bad, refinement=True)[0] == "EINVAL"
    o = hip.prog_opts(script)
    o.flags = 2
    with pytest.raises(pkg.QsHipError, match="flags"):
        hip.encode_progressive_info([job], [o])
