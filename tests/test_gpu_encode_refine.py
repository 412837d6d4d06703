"""Progressive files with refinement scans (Ah > 0) built on the device (torch_qs.encode_file_batch(scans=...,
refinement=True), qs_hip_encode_progressive_device_batch_files with QS_HIP_PROG_REFINE) against libjpeg 9 itself writing
the same arrays with the same scan script (tests/libjpeg9_encode.c): whole files, byte for byte.  DESIGN.md section
17.1."""
import warnings

import numpy as np
import pytest

import jpegqs_pkg
from decode_oracle import GOLD, LibJpeg9
from encode_oracle import LAYOUTS, synth_scan_image
from encode_prog_oracle import BAD_SCRIPTS, PROG_SIZES, RESTARTS, LibJpeg9EncProg, grid_images, scan_summary
from encode_refine_oracle import GRAY_REFINE, big_crafted_images, crafted_images, refine_scripts
from encode_rst_oracle import RST_LAYOUTS
from helpers import Guarded

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
jpeg_file = pkg.jpeg_file


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return LibJpeg9EncProg(tmp_path_factory.mktemp("lj9prog"))


@pytest.fixture(scope="module")
def lj9(tmp_path_factory):
    return LibJpeg9(tmp_path_factory.mktemp("lj9"))


@pytest.fixture(scope="module")
def tq():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible to torch")
    return pkg.torch_qs


@pytest.fixture(scope="module")
def images():
    return grid_images()


def _dev(im):
    """the arrays on the device, each between margins"""
    out = []
    for c in im["coefs"]:
        g = Guarded(c.size, torch.int16)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            g.view.copy_(torch.from_numpy(np.ascontiguousarray(c).reshape(-1)))
        out.append((g, g.view.view(c.shape)))
    return out


def _kw(im):
    return dict(hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"], image_size=im["image_size"])


def _batch(ims):
    devs = [_dev(im) for im in ims]
    return devs, [dict(coefs=[t for _g, t in d], quants=im["quants"], **_kw(im)) for d, im in zip(devs, ims)]


def _capacity(im, script):
    return 8192 + 600 * len(script) + 80 * sum(c.shape[0] * c.shape[1] for c in im["coefs"])


def _files(tq, ims, scripts, restarts=None, caps=None):
    """encode_file_batch(scans=..., refinement=True) with every output between margins and one byte off any alignment ->
    (files as bytes or None, len, status)"""
    devs, batch = _batch(ims)
    if caps is None:
        caps = [_capacity(im, s) for im, s in zip(ims, scripts)]
    outs = [Guarded(1 + c + 64) for c in caps]
    kw = {}
    if restarts is not None:
        kw = dict(restart_interval=[r[0] for r in restarts], restart_in_rows=[r[1] for r in restarts])
    r = tq.encode_file_batch(batch, outs=[o.view[1:1 + c] for o, c in zip(outs, caps)], scans=[list(s) for s in scripts],
                             refinement=True, **kw)
    torch.cuda.synchronize()
    lens, status = r["len"].cpu().tolist(), r["status"].cpu().tolist()
    for o, c in zip(outs, caps):
        o.check(untouched_from=1 + c)
        assert int(o.view[0]) == 0xA5, "the byte in front of the buffer changed"
    for d, im in zip(devs, ims):
        for (g, t), c in zip(d, im["coefs"]):
            g.check()
            assert np.array_equal(t.cpu().numpy(), c), "the encoder changed an input array"
    files = [o.view[1:1 + min(l, c)].cpu().numpy().tobytes() if s in (0, 2) else None for o, l, s, c in zip(outs, lens, status, caps)]
    return files, lens, status


def _scripts(im):
    """the refinement scripts of the issue, and the Ah = 0 script next to them: other scan counts, other kernels"""
    ncomp = len(im["coefs"])
    out = refine_scripts(ncomp, im["colorspace"], jpeg_file.simple_progression)
    out["spectral"] = jpeg_file.spectral_script(ncomp)
    return out


@pytest.mark.parametrize("li", RST_LAYOUTS)
def test_the_grid_equals_libjpeg(tq, prog, images, li):
    """one layout: every size x every script x every restart setting in ONE batch -- refinement and Ah = 0 scripts with
    5 to 18 scans side by side, many launch chunks of scan jobs"""
    cases = [(size, name, script, rst) for size in PROG_SIZES for name, script in _scripts(images[(li, size)]).items()
             for rst in RESTARTS]
    assert {"simple", "ac two steps", "spectral"} <= {c[1] for c in cases} and len({len(c[2]) for c in cases}) > 1
    ims = [images[(li, size)] for size, _n, _s, _r in cases]
    files, lens, status = _files(tq, ims, [c[2] for c in cases], [c[3] for c in cases])
    assert status == [0] * len(cases)
    for (size, name, script, rst), im, f, l in zip(cases, ims, files, lens):
        want = prog.write(im, script, *rst)
        assert l == len(want) and f == want, f"layout {li} at {size}, script {name}, restart {rst}"


def test_crafted_runs(tq, prog):
    """the crafted gray images of tests/encode_refine_oracle.py (test_encode_refine_host.py says what each is for): the cut
    at 937 buffered bits at its edge, with a restart boundary inside the run, 0xF0 followed by bits, folded zeros, heads
    without tails, pieces and runs across workgroup borders"""
    ims = crafted_images()
    cases = [(name, rst) for name in ims for rst in ((0, 0), (10, 0), (15, 0), (1, 0), (256, 0), (0, 1))]
    files, _lens, status = _files(tq, [ims[n] for n, _r in cases], [GRAY_REFINE] * len(cases), [r for _n, r in cases])
    assert status == [0] * len(cases)
    for (name, rst), f in zip(cases, files):
        assert f == prog.write(ims[name], GRAY_REFINE, *rst), (name, rst)


def test_both_cuts_in_one_run(tq, prog):
    """32 768 blocks with the band all zero (the 0x7FFF cut) and 32 896 blocks where the count cuts a piece that carries
    buffered bits and the 937-bit rule cuts the rest: twelve rounds of pointer doubling"""
    ims = list(big_crafted_images().values())
    files, _lens, status = _files(tq, ims + [ims[1]], [GRAY_REFINE] * 3, [(0, 0), (0, 0), (0, 40)])
    assert status == [0] * 3
    for im, rst, f in zip(ims + [ims[1]], [(0, 0), (0, 0), (0, 40)], files):
        assert f == prog.write(im, GRAY_REFINE, *rst), rst


def test_capacities_and_no_prepare(tq, prog):
    """the C ABI directly with QS_HIP_PROG_REFINE, sentinel margins around outputs, scratch and workspace: capacity L, one
    byte short, inside the DC refinement's SOS and inside an AC refinement's segment -- status 2, the exact length, the
    file's first bytes, nothing at or beyond the capacity; a workspace without a prepare: status 4"""
    hip = tq._hip()
    im = synth_scan_image(np.random.default_rng(1), (141, 93), [2, 1, 1], [2, 1, 1], 3)
    script = jpeg_file.simple_progression(3, 3)
    want = prog.write(im, script, 0, 1)
    sos = [i for i in range(len(want) - 1) if want[i] == 0xFF and want[i + 1] == 0xDA]
    caps = [len(want), len(want) - 1, sos[6] + 5, sos[9] + 40, 1]
    n = len(caps)
    devs, batch = _batch([im] * n)
    jobs = [hip.device_job([t.data_ptr() for t in b["coefs"]], [tuple(t.shape[:2]) for t in b["coefs"]], im["quants"], **_kw(im))
            for b in batch]
    opts = [hip.prog_opts(script, 0, 1, refinement=True) for _ in range(n)]
    info, ws_bytes, sc_bytes = hip.encode_progressive_info(jobs, opts)
    head = jpeg_file.compose_parts(im["quants"], im["hsamp"], im["vsamp"], 3, im["image_size"], progressive=True)[0]
    assert info[0]["nscans"] == 10 and len(want) <= len(head) + info[0]["max_body_bytes"]
    ws, sc = Guarded(ws_bytes), Guarded(sc_bytes)
    hd = torch.frombuffer(bytearray(head), dtype=torch.uint8).cuda()
    outs = [Guarded(1 + len(want) + 64) for _ in caps]
    length, status = Guarded(n, torch.int64), Guarded(n, torch.int32)
    stream = torch.cuda.current_stream().cuda_stream
    hip.encode_progressive_prepare(jobs, opts, ws.view.data_ptr(), ws_bytes, stream)
    frames = [hip.encode_frame(head=[(hd.data_ptr(), len(head)), None]) for _ in caps]
    hip.encode_progressive_files(jobs, frames, None, [o.view[1:].data_ptr() for o in outs], caps, length.view.data_ptr(),
                                 status.view.data_ptr(), sc.view.data_ptr(), sc_bytes, ws.view.data_ptr(), ws_bytes, stream)
    torch.cuda.synchronize()
    assert length.view.cpu().tolist() == [len(want)] * n
    assert status.view.cpu().tolist() == [0] + [2] * (n - 1)
    for g in [ws, sc, length, status]:
        g.check()
    for o, c in zip(outs, caps):
        o.check(untouched_from=1 + c)
        assert int(o.view[0]) == 0xA5
        assert o.view[1:1 + c].cpu().numpy().tobytes() == want[:c]
    other = Guarded(ws_bytes)
    other.view.copy_(ws.view)
    hip.encode_progressive_files(jobs, frames, None, [o.view[1:].data_ptr() for o in outs], caps, length.view.data_ptr(),
                                 status.view.data_ptr(), sc.view.data_ptr(), sc_bytes, other.view.data_ptr(), ws_bytes, stream)
    torch.cuda.synchronize()
    assert status.view.cpu().tolist() == [4] * n and length.view.cpu().tolist() == [0] * n


def test_after_smoothing_both_stop_outcomes(tq, prog, lj9):
    """jobs with replacement chroma under stop 0 and stop 1 in one batch, written with jpeg_simple_progression: the device
    picks the geometry, the head and the DRI values of the variant, in the refinement scans as in the others"""
    ims = [lj9.read(GOLD / f"{s}.jpg") for s in ("rgb141x93_420", "rgb128x96_420", "gray64")]
    im = ims[1]
    im["quants"][2] = im["quants"][2].copy()
    im["quants"][2][0] = max(int(im["quants"][2][0]), 3)
    im["coefs"][2] = im["coefs"][2].copy()
    im["coefs"][2][0, 0, 0] = 1000
    _devs, batch = _batch(ims)
    res = tq.quantsmooth_batch_(batch, pkg.flags_for_quality(6), 2)
    scripts = [jpeg_file.simple_progression(len(im["coefs"]), im["colorspace"]) for im in ims]
    r = tq.encode_file_batch(batch, result=res, scans=scripts, restart_in_rows=1, refinement=True)
    torch.cuda.synchronize()
    stops = res["stop"].cpu().tolist()
    assert stops == [0, 1, 0] and res["images"][0]["coef_up"] is not None and res["images"][1]["coef_up"] is not None
    assert r["status"].cpu().tolist() == [0] * 3
    for k, (im, b, ri) in enumerate(zip(ims, batch, res["images"])):
        host = [c.cpu().numpy() for c in b["coefs"]]
        if ri["coef_up"] is not None and stops[k] == 0:
            n = len(host)
            left = dict(coefs=[host[0]] + [u.cpu().numpy() for u in ri["coef_up"]], quants=ri["quants"], hsamp=[1] * n,
                        vsamp=[1] * n, colorspace=im["colorspace"], image_size=im["image_size"])
        else:
            left = dict(coefs=host, quants=ri["quants"], hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"],
                        image_size=im["image_size"])
        got = r["files"][k][:int(r["len"][k])].cpu().numpy().tobytes()
        assert got == prog.write(left, scripts[k], 0, 1), f"job {k} (stop {stops[k]})"


def test_a_captured_graph_follows_the_data(tq, prog, images):
    """encode_file_batch(scans=simple_progression, refinement=True) captured in a graph and replayed after the coefficient
    tensors changed: the runs, their cuts and the tables follow the data"""
    base = [images[(4, (141, 93))], images[(4, (65, 66))], images[(0, (141, 93))]]
    scripts = [jpeg_file.simple_progression(len(im["coefs"]), im["colorspace"]) for im in base]
    work = [[torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in im["coefs"]] for im in base]
    batch = [dict(coefs=w, quants=im["quants"], **_kw(im)) for w, im in zip(work, base)]
    outs = [Guarded(_capacity(im, s)) for im, s in zip(base, scripts)]

    def step(ws):
        return tq.encode_file_batch(batch, outs=[o.view for o in outs], workspace=ws, scans=scripts, restart_interval=7,
                                    refinement=True)

    def check(what, o):
        assert o["status"].cpu().tolist() == [0] * len(base), what
        seen = []
        for k, (im, g, l) in enumerate(zip(base, outs, o["len"].cpu().tolist())):
            got = g.view[:l].cpu().numpy().tobytes()
            now = dict(im, coefs=[w.cpu().numpy() for w in work[k]])
            assert got == prog.write(now, scripts[k], 7, 0), f"{what}, image {k}"
            g.check()
            seen.append(l)
        return tuple(seen)

    out = step(None)
    torch.cuda.synchronize()
    sizes = {check("eager", out)}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = step(out["workspace"])
    rng = np.random.default_rng(5)
    for rep in range(2):
        for w, im in zip(work, base):
            for t, c in zip(w, im["coefs"]):
                c = c.copy()
                c[..., (9 if rep else 40):] //= 2                          # other magnitudes: other tails, other runs
                c += rng.integers(-1, 2, c.shape).astype(np.int16) * (c != 0)
                t.copy_(torch.from_numpy(c))
        g.replay()
        torch.cuda.synchronize()
        sizes.add(check(f"replay {rep}", gout))
    assert len(sizes) == 3


def test_the_flag_decides(tq, prog, images):
    """without refinement=True / QS_HIP_PROG_REFINE the refusals are today's, byte for byte; with it the same script
    writes; a valid script of 380 scans and a sequential script are QS_HIP_ENOTSUP, what libjpeg refuses QS_HIP_EINVAL"""
    hip = tq._hip()
    im = images[(4, (33, 18))]
    _devs, batch = _batch([im])
    script = jpeg_file.simple_progression(3, 3)
    with pytest.raises(ValueError, match=r"encode_file_batch: image 0: the script holds refinement scans \(Ah > 0\), which are "
                                         r"not implemented$"):
        tq.encode_file_batch(batch, scans=script)
    job = hip.device_job([t.data_ptr() for t in batch[0]["coefs"]], [tuple(t.shape[:2]) for t in batch[0]["coefs"]], im["quants"],
                         **_kw(im))

    def verdict(s, **kw):
        try:
            hip.encode_progressive_info([job], [hip.prog_opts(s, **kw)])
            return "ok", ""
        except pkg.QsHipError as e:
            return {-2: "EINVAL", -4: "ENOTSUP"}[e.code], str(e)
    v = verdict(script)
    assert v[0] == "ENOTSUP" and v[1].endswith("qs_hip_encode_progressive_device_batch_info: job 0, scan 5: a refinement scan "
                                               "(Ah > 0): refinement scans are not implemented")
    r = tq.encode_file(batch[0]["coefs"], im["quants"], **_kw(im), scans=script, refinement=True)
    torch.cuda.synchronize()
    assert int(r["status"][0]) == 0 and r["file"][:int(r["len"][0])].cpu().numpy().tobytes() == prog.write(im, script)
    long_script = [((0, 1, 2), 0, 0, 0, 1)] + [((c,), k, k, 0, 1) for c in range(3) for k in range(1, 64)] \
        + [((0, 1, 2), 0, 0, 1, 0)] + [((c,), k, k, 1, 0) for c in range(3) for k in range(1, 64)]
    v = verdict(long_script, refinement=True)
    assert len(long_script) == 380 and v[0] == "ENOTSUP" and "380 scans" in v[1]
    with pytest.raises(pkg.QsHipError, match="380 scans"):
        tq.encode_file_batch(batch, scans=long_script, refinement=True)
    assert verdict([((0,), 0, 63, 0, 0), ((1,), 0, 63, 0, 0), ((2,), 0, 63, 0, 0)], refinement=True)[0] == "ENOTSUP"
    for name, make in BAD_SCRIPTS.items():
        assert verdict(make(3), refinement=True)[0] == "EINVAL", name
        with pytest.raises(ValueError):
            tq.encode_file_batch(batch, scans=make(3), refinement=True)


def test_marker_layout_on_the_device(tq, images):
    """the ten-scan file: no DHT in front of the DC refinement, whose SOS names no table; one AC DHT in front of each AC
    refinement"""
    im = images[(4, (65, 66))]
    files, _lens, status = _files(tq, [im], [jpeg_file.simple_progression(3, 3)])
    assert status == [0]
    marks = [(code, p) for code, p in scan_summary(files[0]) if code in (0xC4, 0xDA)]
    names = ["DHT(%02x)" % p[0] if code == 0xC4 else "SOS(%d-%d %02x)" % (p[-3], p[-2], p[-1]) for code, p in marks]
    assert " ".join(names) == ("DHT(00) DHT(01) SOS(0-0 01) DHT(10) SOS(1-5 02) DHT(11) SOS(1-63 01) DHT(11) SOS(1-63 01) DHT(10) "
                               "SOS(6-63 02) DHT(10) SOS(1-63 21) SOS(0-0 10) DHT(11) SOS(1-63 10) DHT(11) SOS(1-63 10) DHT(10) "
                               "SOS(1-63 10)")
    dc_refine = [p for code, p in marks if code == 0xDA and p[-3] == 0 and p[-1] == 0x10][0]
    assert dc_refine[:7] == bytes([3, 1, 0, 2, 0, 3, 0])
