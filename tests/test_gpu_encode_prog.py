"""Progressive files (spectral selection) built on the device (torch_qs.encode_file_batch(scans=...),
qs_hip_encode_progressive_device_batch_files) against libjpeg 9 itself writing the same arrays with the same scan script
(tests/libjpeg9_encode.c): whole files, byte for byte.  DESIGN.md section 17."""
import hashlib
import warnings

import numpy as np
import pytest

import jpegqs_pkg
from crafted_scans import ac_histogram, shared_deep_image
from decode_oracle import GOLD, LibJpeg9
from encode_oracle import LAYOUTS, ZIGZAG, LibJpeg9Enc, LibjpegError, synth_scan_image
from encode_prog_oracle import (EOB_MAX, PROG_SIZES, RESTARTS, LibJpeg9EncProg, big_mcu_cases, grid_images, scan_summary,
                                scan_symbols_prog, scripts_for)
from encode_rst_oracle import RST_LAYOUTS, gray_image
from helpers import Guarded
from huff_oracle import code_sizes

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
jpeg_file = pkg.jpeg_file

AC_SCRIPT = [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0)]                 # gray: the DC scan, then one scan over the whole AC band
# the script the marker-layout rules were observed with: DC all; Y 1-5; Cr 1-63; Cb 1-63; Y 6-63
FIVE_SCANS = [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 5, 0, 0), ((2,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0), ((0,), 6, 63, 0, 0)]


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return LibJpeg9EncProg(tmp_path_factory.mktemp("lj9prog"))


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    return LibJpeg9Enc(tmp_path_factory.mktemp("lj9enc"))


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
    """the arrays on the device, each between margins (read-only host arrays included: they are only read here)"""
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
    """encode_file_batch(scans=...) with every output between margins and one byte off any alignment -> (files as bytes
    or None, len, status)"""
    devs, batch = _batch(ims)
    if caps is None:
        caps = [_capacity(im, s) for im, s in zip(ims, scripts)]
    outs = [Guarded(1 + c + 64) for c in caps]
    kw = {}
    if restarts is not None:
        kw = dict(restart_interval=[r[0] for r in restarts], restart_in_rows=[r[1] for r in restarts])
    r = tq.encode_file_batch(batch, outs=[o.view[1:1 + c] for o, c in zip(outs, caps)], scans=[list(s) for s in scripts], **kw)
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


@pytest.mark.parametrize("li", RST_LAYOUTS)
def test_the_grid_equals_libjpeg(tq, prog, images, li):
    """one layout: every size x every script x every restart setting in ONE batch -- jobs with different scripts and
    restart settings side by side, many launch chunks of scan jobs"""
    ncomp = len(LAYOUTS[li][0])
    cases = [(size, name, script, rst) for size in PROG_SIZES for name, script in scripts_for(ncomp, jpeg_file.spectral_script).items()
             for rst in RESTARTS]
    ims = [images[(li, size)] for size, _n, _s, _r in cases]
    files, lens, status = _files(tq, ims, [c[2] for c in cases], [c[3] for c in cases])
    assert status == [0] * len(cases)
    for (size, name, script, rst), im, f, l in zip(cases, ims, files, lens):
        want = prog.write(im, script, *rst)
        assert l == len(want) and f == want, f"layout {li} at {size}, script {name}, restart {rst}"


def test_more_than_ten_blocks_per_mcu_scan_by_scan(tq, prog):
    """a 4x4, 1x1, 1x1 frame (18 blocks per MCU, which no single scan can carry) written scan by scan, chroma
    interleaved in one of the scripts, with every restart setting"""
    ims, good, refused = big_mcu_cases()
    cases = [(im, script, rst) for im in ims.values() for script in good.values() for rst in RESTARTS]
    files, _lens, status = _files(tq, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    assert status == [0] * len(cases)
    for (im, script, rst), f in zip(cases, files):
        assert f == prog.write(im, script, *rst), (im["image_size"], script, rst)
    _devs, batch = _batch(list(ims.values())[:1])
    with pytest.raises(pkg.QsHipError, match="18 blocks in an MCU"):
        tq.encode_file_batch(batch, scans=refused)


def _zero_ac_image(wb, hb, seed=5):
    rng = np.random.default_rng(seed)
    blocks = np.zeros((hb * wb, 64), np.int16)
    blocks[:, 0] = rng.integers(-200, 201, hb * wb)
    return blocks


def test_eob_run_cut_at_0x7fff(tq, prog):
    """gray 2056 x 1024 (257 x 128 = 32 896 blocks), all AC zero, AC scan 1-63: one run cut at 0x7FFF; and with a single
    non-zero block at index 32 766, 32 767 and 32 768"""
    ims = []
    for at in (None, EOB_MAX - 1, EOB_MAX, EOB_MAX + 1):
        b = _zero_ac_image(257, 128)
        if at is not None:
            b[at, 5] = 3
        ims.append(gray_image(b, 257))
    files, lens, status = _files(tq, ims, [AC_SCRIPT] * 4)
    assert status == [0] * 4
    for k, (im, f) in enumerate(zip(ims, files)):
        assert f == prog.write(im, AC_SCRIPT), k
    # the first file's AC scan is the two run symbols and nothing else: 0x7FFF blocks, then the remaining 129
    syms = scan_symbols_prog(ims[0], AC_SCRIPT[1], 0)[0]
    assert [(s[1], s[2]) for s in syms] == [(14 << 4, EOB_MAX & 0x3FFF), (7 << 4, 129 & 0x7F)]


LAST = {63: 1}                                                         # a block whose only band coefficient is the band's last


def _blk(pairs):
    b = np.zeros(64, np.int16)
    b[0] = 7
    for k, v in pairs.items():
        b[ZIGZAG[k]] = v
    return b


def _run_image():
    """gray, one row: runs of 1, 2, 3, 4, 7, 8, 255, 256 and 257 all-zero blocks between blocks that do not end in zeros,
    then blocks with 15, 16, 17 and 32 zeros in front of a value, bands that end in 16 or more zeros behind a value, and a
    last run that the end of the scan ends"""
    blocks = [_blk(LAST)]
    for n in (1, 2, 3, 4, 7, 8, 255, 256, 257):
        blocks += [_blk({})] * n + [_blk(LAST)]
    for zeros in (15, 16, 17, 32):
        blocks.append(_blk({1 + zeros: -5, 63: 2}))
    for last_value in (1, 47, 40):                                      # 62, 16 and 23 zeros to the end of the band
        blocks.append(_blk({last_value: 9}))
    blocks += [_blk({})] * 5
    return gray_image(np.array(blocks), len(blocks))


def test_run_lengths_endings_and_zero_runs(tq, prog):
    """the run image without restarts (runs ended by a writing block and by the end of the scan), with restart intervals
    that end runs at a boundary (inside the long runs, and of one block each), and with bands that split the zero runs"""
    im = _run_image()
    scripts = [AC_SCRIPT, AC_SCRIPT, AC_SCRIPT, AC_SCRIPT,
               [((0,), 0, 0, 0, 0), ((0,), 1, 16, 0, 0), ((0,), 17, 63, 0, 0)],
               [((0,), 0, 0, 0, 0), ((0,), 63, 63, 0, 0), ((0,), 1, 62, 0, 0)]]
    restarts = [(0, 0), (100, 0), (1, 0), (256, 0), (7, 0), (0, 0)]
    files, _lens, status = _files(tq, [im] * len(scripts), scripts, restarts)
    assert status == [0] * len(scripts)
    for s, r, f in zip(scripts, restarts, files):
        assert f == prog.write(im, s, *r), (s, r)
    # what the image is for, on the restatement: the run symbols of the plain scan
    runs = [(s[1] >> 4, s[2]) for s in scan_symbols_prog(im, AC_SCRIPT[1], 0)[0] if s[0] == 1 and s[1] & 15 == 0 and s[1] != 0xF0]
    lengths = [(1 << n) + low for n, low in runs]
    assert lengths[:9] == [1, 2, 3, 4, 7, 8, 255, 256, 257] and lengths[-1] == 5 + 1
    zrl = [s for s in scan_symbols_prog(im, AC_SCRIPT[1], 0)[0] if s[1] == 0xF0]
    # 62 zeros in front of each of the ten LAST blocks' value (3 ZRL each); 15, 16, 17 and 32 zeros (0, 1, 1, 2) and then
    # 46, 45, 44 and 29 up to position 63 (2, 2, 2, 1); 46 and 39 zeros in front of positions 47 and 40 (2, 2); the bands
    # that end in 62, 16 and 23 zeros add none
    assert len(zrl) == 30 + (0 + 1 + 1 + 2) + (2 + 2 + 2 + 1) + (2 + 2)


def test_point_transform(tq, prog):
    """coefficients -3 .. 3 with Al 1 and 2: a DC of -1 stays -1, an AC of +-1 becomes a zero that extends the run"""
    vals = np.arange(-3, 4)
    blocks = np.zeros((49, 64), np.int16)
    for i, d in enumerate(vals):
        for j, a in enumerate(vals):
            blocks[7 * i + j, 0] = d
            blocks[7 * i + j, 1] = a
            blocks[7 * i + j, 63] = a if j % 2 else 0
    gray = gray_image(blocks, 7)
    ycc = synth_scan_image(np.random.default_rng(8), (33, 18), [2, 1, 1], [2, 1, 1], 3, amp=3, density=0.6)
    for c in ycc["coefs"]:
        c[..., 0] = np.random.default_rng(9).integers(-3, 4, c.shape[:2])
    cases = []
    for im in (gray, ycc):
        sc = scripts_for(len(im["coefs"]), jpeg_file.spectral_script)
        cases += [(im, sc["Al 1"], (0, 0)), (im, sc["Al 2"], (0, 0)), (im, sc["Al 1"], (3, 0))]
    files, _lens, status = _files(tq, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    assert status == [0] * len(cases)
    for (im, s, r), f in zip(cases, files):
        assert f == prog.write(im, s, *r)
    dc = [s[1:3] for s in scan_symbols_prog(gray, ((0,), 0, 0, 0, 1), 0)[0]]
    # the DC of row i is -3 + i: shifted arithmetically -2, -1, -1, 0, 0, 1, 1 (a division would give -1, -1, 0, 0, ...),
    # so the differences at the row starts are -2, 1, 0, 1, 0, 1, 0
    assert [dc[7 * i] for i in range(7)] == [(2, 1), (1, 1), (0, 0), (1, 1), (0, 0), (1, 1), (0, 0)]


def test_refused_coefficients(tq, prog):
    """AC 2047 with Al = 1 passes; AC 2048 with Al = 1, AC 1024 with Al = 0 and a DC difference of 12 bits are refused:
    status 1 and length 0 for that job, the other jobs of the batch untouched"""
    base = synth_scan_image(np.random.default_rng(3), (40, 24), [1], [1], 1)
    al1 = [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1)]

    def planted(k, v):
        im = dict(base, coefs=[base["coefs"][0].copy()])
        im["coefs"][0][1, 2, k] = v
        return im
    dc12 = dict(base, coefs=[base["coefs"][0].copy()])
    dc12["coefs"][0][0, :3, 0] = [100, -1100, 1100]
    cases = [(base, AC_SCRIPT, 0), (planted(9, 2047), al1, 0), (planted(9, 2048), al1, 1), (planted(9, -2048), al1, 1),
             (planted(9, 1024), AC_SCRIPT, 1), (dc12, AC_SCRIPT, 1), (planted(63, -1023), AC_SCRIPT, 0)]
    files, lens, status = _files(tq, [c[0] for c in cases], [c[1] for c in cases])
    assert status == [c[2] for c in cases]
    for (im, s, st), f, l in zip(cases, files, lens):
        if st:
            assert l == 0
            with pytest.raises(LibjpegError):
                prog.write(im, s)
        else:
            assert f == prog.write(im, s)


def test_capacities_and_margins(tq, prog):
    """the C ABI directly, with sentinel margins around the outputs, the scratch and the workspace: capacity L, one byte
    short, inside a DHT marker, inside an SOS header and inside a segment -- status 2, the exact length, the file's first
    bytes and nothing at or beyond the capacity"""
    hip = tq._hip()
    im = synth_scan_image(np.random.default_rng(1), (141, 93), [2, 1, 1], [2, 1, 1], 3)
    want = prog.write(im, FIVE_SCANS, 0, 1)
    marks, pos = [], 2
    for code, payload in scan_summary(want)[:-1]:
        at = want.index(bytes([0xFF, code]) + (len(payload) + 2).to_bytes(2, "big") + payload, pos)
        marks.append((code, at, len(payload) + 4))
        pos = at + len(payload) + 4
    dht = [m for m in marks if m[0] == 0xC4][2]
    sos = [m for m in marks if m[0] == 0xDA][1]
    caps = [len(want), len(want) - 1, dht[1] + 9, sos[1] + 5, sos[1] + sos[2] + 11, 1]
    n = len(caps)
    devs, batch = _batch([im] * n)
    jobs = [hip.device_job([t.data_ptr() for t in b["coefs"]], [tuple(t.shape[:2]) for t in b["coefs"]], im["quants"], **_kw(im))
            for b in batch]
    opts = [hip.prog_opts(FIVE_SCANS, 0, 1) for _ in range(n)]
    info, ws_bytes, sc_bytes = hip.encode_progressive_info(jobs, opts)
    assert info[0]["nscans"] == 5 and info[0]["interval"] == [9, 18, 9, 9, 18] and info[0]["mcus"] == [54, 216, 54, 54, 216]
    head = jpeg_file.compose_parts(im["quants"], im["hsamp"], im["vsamp"], 3, im["image_size"], progressive=True)[0]
    assert len(want) <= len(head) + info[0]["max_body_bytes"]
    ws, sc = Guarded(ws_bytes), Guarded(sc_bytes)
    hd = torch.frombuffer(bytearray(head), dtype=torch.uint8).cuda()
    outs = [Guarded(1 + len(want) + 64) for _ in caps]
    length = Guarded(n, torch.int64)
    status = Guarded(n, torch.int32)
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
    # a workspace the run finds no prepare for (a copy at another address): status 4 for every job, length 0
    other = Guarded(ws_bytes)
    other.view.copy_(ws.view)
    hip.encode_progressive_files(jobs, frames, None, [o.view[1:].data_ptr() for o in outs], caps, length.view.data_ptr(),
                                 status.view.data_ptr(), sc.view.data_ptr(), sc_bytes, other.view.data_ptr(), ws_bytes, stream)
    torch.cuda.synchronize()
    assert status.view.cpu().tolist() == [4] * n and length.view.cpu().tolist() == [0] * n


def test_a_table_whose_code_lengths_pass_32(tq, prog):
    """the deep-table arrays of tests/crafted_scans.py in a one-component 1-63 scan.  Their construction prescribes the
    baseline scan's AC histogram, EOB symbols included; an AC-first scan counts EOB runs instead, which flattens the tree
    (27 and 28 levels for the arrays of 32 and 33).  With restart_interval = 1 every block is an interval, every run has
    one block, and its symbol is 0x00 without bits -- the baseline's EOB: the histogram, and with it the depth, carries
    over.  32 levels are cut back and written, 33 end with status 5 where libjpeg stops"""
    ims = {d: shared_deep_image(d, False) for d in (32, 33)}
    for d, im in ims.items():
        assert max(code_sizes(ac_histogram(im, (0,)))) == d
    with pytest.raises(LibjpegError):
        prog.write(ims[33], AC_SCRIPT, 1, 0)
    tiny = synth_scan_image(np.random.default_rng(4), (16, 16), [1], [1], 1)
    files, lens, status = _files(tq, [tiny, ims[33], ims[32]], [AC_SCRIPT] * 3, [(1, 0)] * 3)
    assert status == [0, 5, 0] and lens[1] == 0
    assert files[0] == prog.write(tiny, AC_SCRIPT, 1, 0) and files[2] == prog.write(ims[32], AC_SCRIPT, 1, 0)


def _stop_images(lj9):
    """UPSAMPLE_UV inputs (as tests/test_gpu_encode_files.py): 4:2:0 goldens as they are (stop 0) and with a planted
    range-check trip in the last component (stop 1), a grayscale job between them"""
    ims = [lj9.read(GOLD / f"{s}.jpg") for s in ("rgb141x93_420", "rgb128x96_420", "gray64")]
    im = ims[1]
    im["quants"][2] = im["quants"][2].copy()
    im["quants"][2][0] = max(int(im["quants"][2][0]), 3)
    im["coefs"][2] = im["coefs"][2].copy()
    im["coefs"][2][0, 0, 0] = 1000
    return ims


def _left_by_the_smoothing(im, coefs, res, stop):
    host = [c.cpu().numpy() for c in coefs]
    if res["coef_up"] is not None and stop == 0:
        n = len(host)
        return dict(coefs=[host[0]] + [u.cpu().numpy() for u in res["coef_up"]], quants=res["quants"], hsamp=[1] * n,
                    vsamp=[1] * n, colorspace=im["colorspace"], image_size=im["image_size"])
    return dict(coefs=host, quants=res["quants"], hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"],
                image_size=im["image_size"])


def test_after_smoothing_both_stop_outcomes(tq, prog, lj9):
    """jobs with replacement chroma under stop 0 and stop 1 in one batch: the device picks the geometry, the head and the
    DRI values of the variant"""
    ims = _stop_images(lj9)
    _devs, batch = _batch(ims)
    res = tq.quantsmooth_batch_(batch, pkg.flags_for_quality(6), 2)
    scripts = [jpeg_file.spectral_script(len(im["coefs"])) for im in ims]
    r = tq.encode_file_batch(batch, result=res, scans=scripts, restart_in_rows=1)
    torch.cuda.synchronize()
    stops = res["stop"].cpu().tolist()
    assert stops == [0, 1, 0] and res["images"][0]["coef_up"] is not None and res["images"][1]["coef_up"] is not None
    assert r["status"].cpu().tolist() == [0] * 3
    for k, (im, b, ri) in enumerate(zip(ims, batch, res["images"])):
        left = _left_by_the_smoothing(im, b["coefs"], ri, stops[k])
        got = r["files"][k][:int(r["len"][k])].cpu().numpy().tobytes()
        assert got == prog.write(left, scripts[k], 0, 1), f"job {k} (stop {stops[k]})"


def test_seven_jobs_of_five_scans_and_a_captured_graph(tq, prog, lj9):
    """7 jobs x 5 scans = 35 scan jobs, more than one launch chunk; quantsmooth_batch_ then encode_file_batch(scans=...)
    captured in one graph and replayed on other data of the same geometry: the tables follow the data"""
    base = lj9.read(GOLD / "rgb141x93_444.jpg")
    rng = np.random.default_rng(12)
    ims = []
    for k in range(7):
        im = dict(base, coefs=[c.copy() for c in base["coefs"]])
        for c in im["coefs"]:
            c[..., 1 + 6 * k:] = 0
        ims.append(im)
    flags = pkg.flags_for_quality(3)
    src = [[torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in im["coefs"]] for im in ims]
    work = [[t.clone() for t in s] for s in src]
    batch = [dict(coefs=w, quants=im["quants"], **_kw(im)) for w, im in zip(work, ims)]
    outs = [Guarded(200000) for _ in ims]
    ws1, ws2 = None, tq.Workspace()

    def step():
        for w, s in zip(work, src):
            for a, b in zip(w, s):
                a.copy_(b)
        res = tq.quantsmooth_batch_(batch, flags, 1, workspace=ws1)
        return res, tq.encode_file_batch(batch, result=res, outs=[o.view for o in outs], workspace=ws2, scans=FIVE_SCANS,
                                         restart_interval=5)

    res, out = step()                                          # eager: prepares both workspaces, uploads the heads
    ws1 = res["workspace"]
    torch.cuda.synchronize()

    def check(what, r, o):
        assert o["status"].cpu().tolist() == [0] * 7, what
        sizes = []
        for k, (im, g, l) in enumerate(zip(ims, outs, o["len"].cpu().tolist())):
            got = g.view[:l].cpu().numpy().tobytes()
            left = dict(im, coefs=[w.cpu().numpy() for w in work[k]], quants=r["images"][k]["quants"])
            assert got == prog.write(left, FIVE_SCANS, 5, 0), f"{what}, image {k}"
            g.check()
            sizes.append(sum(len(p) for code, p in scan_summary(got) if code == 0xC4))
        return tuple(sizes)

    seen = {check("eager", res, out)}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gres, gout = step()
    for rep in range(2):
        for s, im in zip(src, ims):
            for t, c in zip(s, im["coefs"]):
                c = c.copy()
                c[..., (4 if rep else 30):] = 0
                c += rng.integers(-1, 2, c.shape).astype(np.int16) * (c != 0)
                t.copy_(torch.from_numpy(c))
        g.replay()
        torch.cuda.synchronize()
        seen.add(check(f"replay {rep}", gres, gout))
    assert len(seen) == 3                                      # the size of the tables changed with the data


def test_arguments(tq):
    im = synth_scan_image(np.random.default_rng(2), (16, 16), [1], [1], 1)
    _devs, batch = _batch([im])
    with pytest.raises(ValueError, match="optimize"):
        tq.encode_file_batch(batch, optimize=False, scans=AC_SCRIPT)
    with pytest.raises(ValueError, match="refinement"):
        tq.encode_file_batch(batch, scans=[((0,), 0, 0, 0, 1), ((0,), 0, 0, 1, 0)])
    with pytest.raises(ValueError):
        tq.encode_file_batch(batch, scans=[((0,), 1, 63, 0, 0)])


# SHA-256 of the baseline optimized files of three images.  The parent commit's encode_file gives exactly libjpeg's
# optimize_coding file for them (its own suite pins that: tests/test_gpu_encode_files.py), so these are the parent's
# bytes; they were taken from libjpeg 9d's file and do not involve this tree.
PARENT_FILES = {
    (0, (141, 93)): "d96e50e20166a78e382af952e89a1971400e8f99ed0c679ff2f953a84308c176",
    (4, (141, 93)): "82f0493af63602d871cdb3668dd6fcef4393deca8c2d812320c938cabf404cdb",
    (7, (33, 18)): "4b222cc939982ef1c0e6d91d894e3e3813c5e1db61feb1658ff4385e4cacb9d4",
}


def test_without_scans_the_bytes_are_the_parents(tq, enc, images):
    for key, digest in PARENT_FILES.items():
        im = images[key]
        _devs, batch = _batch([im])
        r = tq.encode_file(batch[0]["coefs"], im["quants"], **_kw(im))
        torch.cuda.synchronize()
        got = r["file"][:int(r["len"][0])].cpu().numpy().tobytes()
        assert int(r["status"][0]) == 0 and r["tables"] is not None
        assert hashlib.sha256(got).hexdigest() == digest, key
        assert got == enc.write(im, optimize=True)
