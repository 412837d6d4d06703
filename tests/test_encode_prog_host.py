"""Progressive files (spectral selection) before any GPU is involved: libjpeg 9 itself writes the files
(tests/libjpeg9_encode.c); the plain Python restatement of tests/encode_prog_oracle.py and the host build of
csrc/qs_encode_prog.h (tests/encode_prog_host.cpp, plain and under ASan + UBSan as a program of its own) are pinned to
them, whole file; the script validation of the library, of jpeg_file and of libjpeg agree; libjpeg and Pillow read the
files back.  DESIGN.md section 17."""
import io

import numpy as np
import pytest

import jpegqs_pkg
from decode_oracle import GOLD, LibJpeg9
from encode_oracle import LibjpegError, synth_scan_image
from encode_prog_oracle import (BAD_SCRIPTS, PROG_SIZES, RESTARTS, LibJpeg9EncProg, ProgHost, big_mcu_cases, complete,
                                encode_progressive, grid_images, scan_summary, scripts_for)
from encode_rst_oracle import RST_LAYOUTS

pkg = jpegqs_pkg.load()
jpeg_file = pkg.jpeg_file

FIVE_SCANS = [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 5, 0, 0), ((2,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0), ((0,), 6, 63, 0, 0)]


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return LibJpeg9EncProg(tmp_path_factory.mktemp("lj9prog"))


@pytest.fixture(scope="module")
def lj9(tmp_path_factory):
    return LibJpeg9(tmp_path_factory.mktemp("lj9"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ProgHost(tmp_path_factory.mktemp("proghost"))


@pytest.fixture(scope="module")
def host_san(tmp_path_factory):
    return ProgHost(tmp_path_factory.mktemp("proghost_san"), sanitize=True)


@pytest.fixture(scope="module")
def images():
    return grid_images()


def _head(im):
    return jpeg_file.compose_parts(im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"], progressive=True)[0]


@pytest.fixture(scope="module")
def written(prog, images):
    """{(layout, size, script name, restart): libjpeg's file}: the whole grid, written once"""
    out = {}
    for (li, size), im in images.items():
        for name, script in scripts_for(len(im["coefs"]), jpeg_file.spectral_script).items():
            for rst in RESTARTS:
                out[(li, size, name, rst)] = prog.write(im, script, *rst)
    assert len(out) == len(RST_LAYOUTS) * len(PROG_SIZES) * 9 * len(RESTARTS)
    return out


def _script(key, images):
    li, size, name, _rst = key
    return scripts_for(len(images[(li, size)]["coefs"]), jpeg_file.spectral_script)[name]


def test_the_python_restatement_equals_libjpeg(written, images):
    for key, want in written.items():
        im = images[key[:2]]
        assert encode_progressive(im, _script(key, images), _head(im), *key[3]) == want, key


def test_the_host_build_equals_libjpeg(written, images, host):
    for key, want in written.items():
        im = images[key[:2]]
        assert host.write(im, _script(key, images), _head(im), *key[3]) == want, key


def test_the_host_build_under_sanitizers(written, images, host_san):
    """the same program with -fsanitize=address,undefined, every array in an allocation of its own: the whole grid"""
    n = 0
    for key, want in written.items():
        im = images[key[:2]]
        assert host_san.write(im, _script(key, images), _head(im), *key[3]) == want, key
        n += 1
    assert n == len(RST_LAYOUTS) * len(PROG_SIZES) * 9 * len(RESTARTS) == 1764
    assert host_san.bounds().startswith("bounds ok")


def test_the_bounds_of_the_header(host, hip):
    """the per-block worst case the header states is reached by construction and sizes the workspace: an AC scan over
    1-63 needs more than the baseline coder's 208 bytes per block"""
    assert host.bounds().startswith("bounds ok: AC 1..63 1668 bits, DC 27 bits")
    im = synth_scan_image(np.random.default_rng(1), (2048, 8), [1], [1], 1)
    job, _keep = hip._make_job(im["coefs"], im["quants"], hsamp=[1], vsamp=[1], colorspace=1, image_size=(2048, 8))
    sizes = {}
    for band in ((1, 63), (1, 5), (6, 63)):
        opts = [hip.prog_opts([((0,), 0, 0, 0, 0), ((0,), band[0], band[1], 0, 0)])]
        _info, ws, _sc = hip.encode_progressive_info([job], opts)
        sizes[band] = ws

    def stream(ss, se):
        """what the workspace holds for the unstuffed stream of an AC scan of 256 blocks (one workgroup, one interval):
        256 * ((Se - Ss + 1) * 26 + 30) bits, 16 bytes for the last lane's read, in the layout's steps of 256"""
        return -(-(256 * ((se - ss + 1) * 26 + 30) // 8 + 16) // 256) * 256
    # every other array of the three workspaces has the same size (256 blocks, at most 32 stuffing units): the
    # workspaces differ by exactly the bound's difference
    assert stream(1, 63) == 53504 > 256 * 208
    assert sizes[(1, 63)] - sizes[(1, 5)] == stream(1, 63) - stream(1, 5) == 48128
    assert sizes[(1, 63)] - sizes[(6, 63)] == stream(1, 63) - stream(6, 63) == 4096


def test_marker_layout_rules(prog, lj9):
    """the rules the issue lists, on libjpeg's own files of tests/golden/cli/rgb141x93_420.jpg with the script "DC all; Y
    1-5; Cr 1-63; Cb 1-63; Y 6-63": the DHT markers of each scan in front of its SOS, DRI when the interval changes"""
    im = lj9.read(GOLD / "rgb141x93_420.jpg")

    def layout(data):
        out = []
        for code, p in scan_summary(data):
            if code == 0xC4:
                out.append("DHT(%02x)" % p[0])
            elif code == 0xDD:
                out.append("DRI %d" % int.from_bytes(p, "big"))
            elif code in (0xC2, 0xDA, 0xD9):
                out.append({0xC2: "SOF2", 0xDA: "SOS", 0xD9: "EOI"}[code])
        return " ".join(out[out.index("SOF2"):])
    assert layout(prog.write(im, FIVE_SCANS)) == "SOF2 DHT(00) DHT(01) SOS DHT(10) SOS DHT(11) SOS DHT(11) SOS DHT(10) SOS EOI"
    assert layout(prog.write(im, FIVE_SCANS, 0, 1)) == ("SOF2 DHT(00) DHT(01) DRI 9 SOS DHT(10) DRI 18 SOS DHT(11) DRI 9 SOS "
                                                        "DHT(11) SOS DHT(10) DRI 18 SOS EOI")
    assert layout(prog.write(im, FIVE_SCANS, 5, 0)) == ("SOF2 DHT(00) DHT(01) DRI 5 SOS DHT(10) SOS DHT(11) SOS DHT(11) SOS "
                                                        "DHT(10) SOS EOI")
    for rst in ((0, 0), (0, 1), (5, 0)):
        assert encode_progressive(im, FIVE_SCANS, _head(im), *rst) == prog.write(im, FIVE_SCANS, *rst)


def _lib_verdict(hip, job, script):
    try:
        hip.encode_progressive_info([job], [hip.prog_opts(script)])
        return "ok"
    except pkg.QsHipError as e:
        return {-2: "EINVAL", -4: "ENOTSUP"}[e.code], str(e)


def test_script_validation_agrees_with_libjpeg(prog, host, hip, images):
    """the library, the host build of the header, jpeg_file.validate_script and libjpeg on bad scripts (three
    components); Al up to 10 is accepted; Ah > 0 is QS_HIP_ENOTSUP, a sequential multi-scan script as well"""
    im = images[(4, (33, 18))]
    job, _keep = hip._make_job(im["coefs"], im["quants"], hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=3,
                               image_size=im["image_size"])
    for name, make in BAD_SCRIPTS.items():
        script = make(3)
        with pytest.raises(LibjpegError):
            prog.write(im, script)
        with pytest.raises(jpeg_file.ScriptError):
            jpeg_file.validate_script(script, 3)
        assert host.validate(script, 3)[0] == 1, name
        verdict = _lib_verdict(hip, job, script)
        assert verdict[0] == "EINVAL", (name, verdict)
        if name != "no DC for a component":
            assert "scan" in verdict[1], (name, verdict)
    good = [((0, 1, 2), 0, 0, 0, 10), ((1,), 1, 63, 0, 10)]
    assert prog.write(im, good) == encode_progressive(im, good, _head(im))
    assert jpeg_file.validate_script(good, 3) is True and host.validate(good, 3) == (0, -1)
    assert _lib_verdict(hip, job, good) == "ok"
    refine = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 63, 0, 0), ((0, 1, 2), 0, 0, 1, 0)]
    prog.write(im, refine)                                              # libjpeg writes it
    assert jpeg_file.validate_script(refine, 3) is False and host.validate(refine, 3) == (2, 2)
    verdict = _lib_verdict(hip, job, refine)
    assert verdict[0] == "ENOTSUP" and "scan 2" in verdict[1] and "refinement scans are not implemented" in verdict[1]
    sequential = [((0,), 0, 63, 0, 0), ((1,), 0, 63, 0, 0), ((2,), 0, 63, 0, 0)]
    prog.write(im, sequential)
    assert host.validate(sequential, 3)[0] == 3 and _lib_verdict(hip, job, sequential)[0] == "ENOTSUP"
    with pytest.raises(jpeg_file.ScriptError, match="sequential"):
        jpeg_file.validate_script(sequential, 3)
    # ENOTSUP is for scripts libjpeg accepts: a malformed script whose first scan is 0 .. 63 is refused like any other
    for bad in ([((0,), 0, 63, 0, 0), ((1,), 0, 63, 0, 0)], [((0,), 0, 63, 0, 0), ((1,), 0, 63, 0, 0), ((3,), 0, 63, 0, 0)],
                [((0, 1, 2), 0, 63, 0, 0), ((1,), 1, 63, 0, 0)], [((0, 1, 2), 0, 63, 0, 0), ((0,), 0, 63, 0, 0)]):
        with pytest.raises(LibjpegError):
            prog.write(im, bad)
        assert host.validate(bad, 3)[0] == 1 and _lib_verdict(hip, job, bad)[0] == "EINVAL", bad
        with pytest.raises(jpeg_file.ScriptError):
            jpeg_file.validate_script(bad, 3)
    # ... and a valid script of more than 256 scans (refinement passes one coefficient at a time) is ENOTSUP, not "too long"
    long_script = [((0, 1, 2), 0, 0, 0, 1)] + [((c,), k, k, 0, 1) for c in range(3) for k in range(1, 64)] \
        + [((0, 1, 2), 0, 0, 1, 0)] + [((c,), k, k, 1, 0) for c in range(3) for k in range(1, 64)]
    assert len(long_script) == 380
    prog.write(im, long_script)
    assert host.validate(long_script, 3) == (2, 190) and jpeg_file.validate_script(long_script, 3) is False
    verdict = _lib_verdict(hip, job, long_script)
    assert verdict[0] == "ENOTSUP" and "scan 190" in verdict[1]


def test_more_than_ten_blocks_per_mcu_is_judged_scan_by_scan(prog, host, host_san, hip):
    """a 4x4, 1x1, 1x1 frame has 18 blocks per MCU: libjpeg writes it as long as no scan interleaves more than 10, and
    refuses the script whose DC scan carries all three components -- so do the restatements and the library
    (QS_HIP_EINVAL, naming the scan)"""
    ims, good, refused = big_mcu_cases()
    for size, im in ims.items():
        for name, script in good.items():
            for rst in RESTARTS:
                want = prog.write(im, script, *rst)
                assert encode_progressive(im, script, _head(im), *rst) == want, (size, name, rst)
                assert host.write(im, script, _head(im), *rst) == want, (size, name, rst)
                assert host_san.write(im, script, _head(im), *rst) == want, (size, name, rst)
        with pytest.raises(LibjpegError):
            prog.write(im, refused)
        assert host.write(im, refused, _head(im)) == "mcu"
        job, _keep = hip._make_job(im["coefs"], im["quants"], hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=3,
                                   image_size=im["image_size"])
        verdict = _lib_verdict(hip, job, refused)
        assert verdict[0] == "EINVAL" and "scan 0" in verdict[1] and "18 blocks" in verdict[1]
        assert all(_lib_verdict(hip, job, s) == "ok" for s in good.values())
        # the baseline coder, whose one scan carries all components, keeps refusing the frame
        with pytest.raises(pkg.QsHipError, match="18 blocks in an MCU"):
            hip.encode_batch_info([job])


def test_info_reports_scans_mcus_and_intervals(hip, lj9, prog):
    im = lj9.read(GOLD / "rgb141x93_420.jpg")
    job, _keep = hip._make_job(im["coefs"], im["quants"], hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=3,
                               image_size=im["image_size"])
    info, ws, sc = hip.encode_progressive_info([job, job], [hip.prog_opts(FIVE_SCANS, 0, 1), hip.prog_opts(FIVE_SCANS, 5, 0)])
    assert [i["nscans"] for i in info] == [5, 5] and ws % 256 == 0 and sc % 256 == 0 and ws > 0 and sc > 0
    assert info[0]["mcus"] == [54, 216, 54, 54, 216] and info[0]["interval"] == [9, 18, 9, 9, 18]
    assert info[1]["interval"] == [5] * 5
    for i, rst in zip(info, ((0, 1), (5, 0))):
        assert len(prog.write(im, FIVE_SCANS, *rst)) <= len(_head(im)) + i["max_body_bytes"]


def test_sof2_head_and_the_reader(prog, lj9, images):
    """compose_parts(progressive=True) changes the SOF marker's code and nothing else, existing calls keep their bytes,
    and parse keeps refusing SOF2"""
    for key in ((0, (8, 8)), (4, (141, 93)), (7, (33, 18))):
        im = images[key]
        args = (im["quants"], im["hsamp"], im["vsamp"], im["colorspace"], im["image_size"])
        base, prg = jpeg_file.compose_parts(*args), jpeg_file.compose_parts(*args, progressive=True)
        assert base[1] == prg[1] and len(base[0]) == len(prg[0])
        diff = [i for i in range(len(base[0])) if base[0][i] != prg[0][i]]
        assert len(diff) == 1 and base[0][diff[0]] in (0xC0, 0xC1) and prg[0][diff[0]] == 0xC2 and base[0][diff[0] - 1] == 0xFF
        assert jpeg_file.compose_parts(*args, None, None, 0) == base
        script = jpeg_file.spectral_script(len(im["coefs"]))
        f = prog.write(im, script)
        assert f.startswith(prg[0])
        with pytest.raises(ValueError, match="progressive"):
            jpeg_file.parse(f)
    assert jpeg_file.spectral_script(3) == [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 5, 0, 0), ((0,), 6, 63, 0, 0), ((1,), 1, 5, 0, 0),
                                            ((1,), 6, 63, 0, 0), ((2,), 1, 5, 0, 0), ((2,), 6, 63, 0, 0)]


def test_complete_scripts_read_back(written, images, lj9, tmp_path):
    """every complete script's file of the grid (spectral, band 1-63 and reversed: every coefficient with Al = 0) is read
    back by libjpeg to the arrays that went in, and Pillow opens and decodes it and reports it as progressive"""
    from PIL import Image
    n, names = 0, set()
    for key, data in written.items():
        li, size, name, rst = key
        im = images[(li, size)]
        if not complete(_script(key, images), len(im["coefs"])):
            continue
        names.add(name)
        p = tmp_path / "f.jpg"
        p.write_bytes(data)
        back = lj9.read(p)
        assert len(back["coefs"]) == len(im["coefs"])
        for a, b in zip(back["coefs"], im["coefs"]):
            assert np.array_equal(a[:b.shape[0], :b.shape[1]], b), key
        with Image.open(io.BytesIO(data)) as pil:
            assert pil.info.get("progressive") and pil.info.get("progression"), key
            assert pil.size == tuple(size)
            pil.load()
        n += 1
    assert names == {"spectral", "band 1-63", "reversed"}
    assert n == len(RST_LAYOUTS) * len(PROG_SIZES) * 3 * len(RESTARTS) == 588
