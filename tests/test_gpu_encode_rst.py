"""Restart intervals of the device entropy coder on the GPU (torch_qs.encode / encode_scan / encode_histogram_batch with
restart_interval / restart_in_rows, qs_hip_encode_device_batch_prepare_opts): against libjpeg 9 itself writing the same
arrays with cinfo.restart_interval / cinfo.restart_in_rows (tests/libjpeg9_encode.c) and against the plain Python
restatement of its rules (tests/encode_rst_oracle.py).  Every output and workspace lies between sentinel margins."""
import numpy as np
import pytest

import jpegqs_pkg
import encode_rst_oracle as R
from decode_oracle import GOLD, LibJpeg9
from encode_oracle import LibjpegError, histogram, synth_scan_image
from encode_rst_oracle import (LibJpeg9EncRst, dc_range_images, encode_scan_rst, histogram_rst, interval_of, layout_cases,
                               mcu_geometry, optimize_cases, parse_rst, scan_layout_rst)
from helpers import Guarded

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
jpeg_file = pkg.jpeg_file


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    return LibJpeg9EncRst(tmp_path_factory.mktemp("lj9rst"))


@pytest.fixture(scope="module")
def lj9(tmp_path_factory):
    return LibJpeg9(tmp_path_factory.mktemp("lj9"))


@pytest.fixture(scope="module")
def tq():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible to torch")
    return pkg.torch_qs


@pytest.fixture(scope="module")
def std():
    hip = pkg.HipQS()
    dc, ac = {t: tuple(hip.huff_standard(0, t)) for t in (0, 1)}, {t: tuple(hip.huff_standard(1, t)) for t in (0, 1)}
    R.set_standard_tables(dc, ac)
    return dc, ac


def _tbl(im):
    return jpeg_file.table_assignment(im["colorspace"], len(im["coefs"]))


def _kw(im):
    return dict(hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"], image_size=im["image_size"])


class Uploaded:
    """the arrays of distinct images on the device, each between margins; jobs on one image share them"""

    def __init__(self, ims):
        self.ims, self.dev = ims, {}
        for im in ims:
            if id(im) not in self.dev:
                d = []
                for c in im["coefs"]:
                    g = Guarded(c.size, torch.int16)
                    g.view.copy_(torch.from_numpy(np.ascontiguousarray(c).reshape(-1)))
                    d.append((g, g.view.view(c.shape)))
                self.dev[id(im)] = (im, d)
        self.batch = [dict(coefs=[t for _g, t in self.dev[id(im)][1]], quants=im["quants"], **_kw(im)) for im in ims]

    def check(self):
        for im, d in self.dev.values():
            for (g, t), c in zip(d, im["coefs"]):
                g.check()
                assert np.array_equal(t.cpu().numpy(), c), "the encoder changed an input array"


def _scan(tq, ims, ri, rows, caps=None, **kw):
    """encode_scan_batch with restart options and every buffer, the workspace included, between margins -> (segments
    as bytes or None, len, status, output guards)"""
    up = Uploaded(ims)
    hip = pkg.HipQS()
    jobs = [hip.device_job([0] * len(im["coefs"]), [c.shape[:2] for c in im["coefs"]], [None] * len(im["coefs"]), **_kw(im))
            for im in ims]
    opts = None if ri is None and rows is None else list(zip(ri or [0] * len(ims), rows or [0] * len(ims)))
    per, total = hip.encode_batch_info(jobs, opts)
    if caps is None:
        caps = [min(p["max_segment_bytes"], 4096 + 72 * sum(c.shape[0] * c.shape[1] for c in im["coefs"]))
                for p, im in zip(per, ims)]
    outs = [Guarded(c) for c in caps]
    wsg = Guarded(total)
    ws = tq.Workspace(buf=wsg.view)
    r = tq.encode_scan_batch(up.batch, outs=[o.view for o in outs], workspace=ws, restart_interval=ri, restart_in_rows=rows,
                             **kw)
    torch.cuda.synchronize()
    assert r["workspace"].buf.data_ptr() == wsg.view.data_ptr()       # the guarded one was large enough and was used
    wsg.check()
    lens, status = r["len"].cpu().tolist(), r["status"].cpu().tolist()
    for o in outs:
        o.check()
    up.check()
    segs = [o.view[:l].cpu().numpy().tobytes() if s == 0 else None for o, l, s in zip(outs, lens, status)]
    return segs, lens, status, outs


def test_every_layout_size_and_interval_in_one_batch(tq, enc, std):
    """layouts x sizes with edge MCUs x Ri in {1, 2, 7, MCUs per row, M - 1, M, M + 1, 65535} and restart_in_rows in
    {1, 2}: a batch of many launch chunks, against libjpeg and the restatement"""
    dc, ac = std
    cases = layout_cases()
    ims = [im for _n, im, _ri, _rows in cases]
    segs, lens, status, _ = _scan(tq, ims, [ri for _n, _im, ri, _r in cases], [rows for _n, _im, _ri, rows in cases])
    assert status == [0] * len(cases)
    for (name, im, ri, rows), s, l in zip(cases, segs, lens):
        want = parse_rst(enc.write(im, ri, rows))["segment"]
        assert s == want and l == len(want), name
        assert s == encode_scan_rst(im, _tbl(im), dc, ac, interval_of(im, ri, rows)), name


def test_whole_files_carry_dri(tq, enc):
    cases = layout_cases()[3::11]
    up = Uploaded([im for _n, im, _ri, _rows in cases])
    files = tq.encode_batch(up.batch, restart_interval=[c[2] for c in cases], restart_in_rows=[c[3] for c in cases])
    for (name, im, ri, rows), f in zip(cases, files):
        assert f == enc.write(im, ri, rows), name
    name, im, ri, rows = cases[0]
    one = tq.encode(up.batch[0]["coefs"], im["quants"], **_kw(im), restart_interval=ri, restart_in_rows=rows)
    assert one == files[0]


def test_interval_ends_inside_workgroups(tq, enc, std):
    """4:2:0 over four workgroups with Ri = 7 (42 blocks against 256 lanes, more than 8 intervals: RSTn wraps); 512 x 512
    gray with Ri = 1: 16 workgroups of 256 interval ends each, once with few bits and once with blocks near the longest
    code a block can have"""
    dc, ac = std
    rng = np.random.default_rng(420)
    a = synth_scan_image(rng, (200, 150), [2, 1, 1], [2, 1, 1], 3)
    assert mcu_geometry(a)[1] * 6 > 3 * 256
    b = synth_scan_image(rng, (512, 512), [1], [1], 1)
    c = synth_scan_image(rng, (512, 512), [1], [1], 1, amp=1023, density=1.0)
    v = c["coefs"][0][..., 1:].astype(np.int32)
    c["coefs"][0][..., 1:] = np.where(v < 0, -1, 1) * ((np.abs(v) & 511) | 512)          # every AC value of 10 bits
    ims, ri = [a, b, c], [7, 1, 1]
    caps = [40000, 64 * 64 * 80, 64 * 64 * 420]
    segs, lens, status, _ = _scan(tq, ims, ri, None, caps=caps)
    assert status == [0, 0, 0]
    for k, (im, r, s) in enumerate(zip(ims, ri, segs)):
        want = parse_rst(enc.write(im, r, 0))["segment"]
        assert s == want, f"image {k}"
    lay = scan_layout_rst(c, (0,), dc, ac, 1)
    assert min(lay["bits"]) > 0.9 * (27 + 63 * 26) and segs[2] == R.compose_segment(lay["raw"])
    assert segs[0] == encode_scan_rst(a, _tbl(a), dc, ac, 7)
    assert segs[0].count(b"\xff\xd0") >= 2 and segs[0].count(b"\xff\xd7") >= 2          # more than 8 intervals


def test_padding_extremes_and_markers_at_the_stuffing_unit(tq, enc, std):
    """pad 0, a padded 0xFF and a data 0xFF in front of a marker; markers between two 4 KiB units of the unstuffed stream,
    behind a plain byte, a padded 0xFF and a data 0xFF (tests/test_encode_rst_host.py asserts the cases are that)"""
    dc, ac = std
    (p, pr), (u, ur) = R.padding_case(), R.unit_case()
    segs, lens, status, _ = _scan(tq, [p, u], [pr, ur], None)
    assert status == [0, 0]
    for k, (im, r, s) in enumerate(((p, pr, segs[0]), (u, ur, segs[1]))):
        assert s == parse_rst(enc.write(im, r, 0))["segment"], f"image {k}"
        assert s == encode_scan_rst(im, (0,), dc, ac, r), f"image {k}"


def test_mixed_batch_of_more_than_one_chunk(tq, enc, std):
    """45 jobs: the first launch chunk (32 jobs) has no restart job, the second mixes intervals with 0 and with
    intervals that cover the scan; jobs without a marker give the bytes of the call without the keyword"""
    dc, ac = std
    rng = np.random.default_rng(45)
    ims, ri, rows = [], [], []
    for k in range(45):
        hs, vs, cs = R.LAYOUTS[R.RST_LAYOUTS[k % 7]]
        im = synth_scan_image(rng, [(40, 24), (67, 35), (16, 50)][k % 3], hs, vs, cs)
        m = mcu_geometry(im)[1]
        ims.append(im)
        if k < 32:
            ri.append([0, m, 65535][k % 3]), rows.append(0)
        else:
            ri.append([0, 1, 3, m, m - 1][k % 5]), rows.append(1 if k % 6 == 0 else 0)
    segs, lens, status, _ = _scan(tq, ims, ri, rows)
    plain, plens, pstatus, _ = _scan(tq, ims, None, None)
    assert status == [0] * 45 == pstatus
    marked = 0
    for k, (im, s) in enumerate(zip(ims, segs)):
        Ri = interval_of(im, ri[k], rows[k])
        assert s == parse_rst(enc.write(im, ri[k], rows[k]))["segment"], f"job {k}"
        assert s == encode_scan_rst(im, _tbl(im), dc, ac, Ri), f"job {k}"
        if Ri == 0 or Ri >= mcu_geometry(im)[1]:
            assert s == plain[k], f"job {k}"
        else:
            marked += 1
    assert 5 < marked < 13
    first = _scan(tq, ims[:32], ri[:32], rows[:32])[0]                # a batch of one chunk without a restart job
    assert first == plain[:32]


def _stop_images(lj9):
    """UPSAMPLE_UV inputs (tests/test_gpu_encode.py): 4:2:0 and 4:2:2 goldens as they are (stop 0) and with a planted
    range-check trip in the last component (stop 1)"""
    ims = [lj9.read(GOLD / f"{s}.jpg") for s in ("rgb141x93_420", "rgb128x96_420", "rgb120x88_422_rst")]
    for k in (1, 2):
        im = ims[k]
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


def test_after_smoothing_each_geometry_gets_its_interval(tq, enc, lj9):
    """UPSAMPLE_UV jobs under both stop values: restart_in_rows = 1 is one MCU row of the geometry the device chose
    (1x1 chroma when the replacement stands, the sampled layout when it does not), and the file's DRI says so; a plain
    restart_interval applies to whichever geometry is chosen; optimize counts the restart scan's symbols"""
    ims = _stop_images(lj9)
    up = Uploaded(ims)
    res = tq.quantsmooth_batch_(up.batch, pkg.flags_for_quality(6), 2)
    stops = res["stop"].cpu().tolist()
    assert stops == [0, 1, 1] and all(r["coef_up"] is not None for r in res["images"])
    left = [_left_by_the_smoothing(im, b["coefs"], r, s) for im, b, r, s in zip(ims, up.batch, res["images"], stops)]
    files = tq.encode_batch(up.batch, result=res, restart_in_rows=1)
    dris = []
    for k, (l, f) in enumerate(zip(left, files)):
        assert f == enc.write(l, 0, 1), f"job {k} (stop {stops[k]})"
        dris.append(parse_rst(f)["dri"])
    assert dris == [-(-141 // 8), -(-128 // 16), -(-120 // 16)]     # 1x1 MCUs of 8 pixels; 4:2:0 and 4:2:2 of 16
    for opt in (False, True):
        files = tq.encode_batch(up.batch, result=res, restart_interval=5, optimize=opt)
        for k, (l, f) in enumerate(zip(left, files)):
            assert f == enc.write(l, 5, 0, optimize=opt), f"job {k} (stop {stops[k]}, optimize {opt})"


def test_smooth_and_encode_with_restarts_in_one_captured_graph(tq, enc, lj9):
    ims = _stop_images(lj9)[:2]
    ims[1]["coefs"][2][0, 0, 0] = int(lj9.read(GOLD / "rgb128x96_420.jpg")["coefs"][2][0, 0, 0])      # no trip to begin with
    flags = pkg.flags_for_quality(6)
    src = [[torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in im["coefs"]] for im in ims]
    work = [[t.clone() for t in s] for s in src]
    batch = [dict(coefs=w, quants=im["quants"], **_kw(im)) for w, im in zip(work, ims)]
    outs = [Guarded(200000) for _ in ims]
    ws1, ws2 = None, tq.Workspace()

    def step():
        for w, s in zip(work, src):
            for a, b in zip(w, s):
                a.copy_(b)
        res = tq.quantsmooth_batch_(batch, flags, 2, workspace=ws1)
        return res, tq.encode_scan_batch(batch, result=res, outs=[o.view for o in outs], workspace=ws2, restart_in_rows=1)

    res, out = step()                                          # eager: prepares both workspaces
    ws1 = res["workspace"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gres, gout = step()
    seen = set()
    for rep in range(2):
        src[1][2].view(-1)[0] = 1000 if rep == 1 else int(ims[1]["coefs"][2].reshape(-1)[0])
        g.replay()
        torch.cuda.synchronize()
        glen, gstatus, gstop = gout["len"].cpu().tolist(), gout["status"].cpu().tolist(), gres["stop"].cpu().tolist()
        assert gstatus == [0, 0]
        for k, (im, b, r, o) in enumerate(zip(ims, batch, gres["images"], outs)):
            want = parse_rst(enc.write(_left_by_the_smoothing(im, b["coefs"], r, gstop[k]), 0, 1))["segment"]
            assert o.view[:glen[k]].cpu().numpy().tobytes() == want, f"replay {rep}, image {k} (stop {gstop[k]})"
            o.check()
        seen.add(tuple(gstop))
    assert seen == {(0, 0), (0, 1)}                             # the geometry, and with it the interval, changed


def test_capacity_and_status(tq, enc, std):
    dc, ac = std
    im = synth_scan_image(np.random.default_rng(9), (141, 93), [2, 1, 1], [2, 1, 1], 3)
    want = parse_rst(enc.write(im, 4, 0))["segment"]
    n = len(want)
    cut = want.index(b"\xff\xd2") + 1                               # between the two bytes of a marker
    a, b = dc_range_images()
    ims = [im, im, im, a, a, b, b]
    ri = [4, 4, 4, 0, 2, 0, 2]
    caps = [n, n - 1, cut, 64, 64, 64, 64]
    segs, lens, status, outs = _scan(tq, ims, ri, None, caps=caps)
    assert status == [0, 2, 2, 0, 1, 1, 0]
    assert lens == [n, n, n, len(segs[3]), 0, 0, len(segs[6])]
    assert segs[0] == want
    for o, c in zip(outs[:3], caps):
        assert o.view.cpu().numpy().tobytes() == want[:c]           # the part that fits, and nothing beyond it
    assert segs[3] == parse_rst(enc.write(a, 0, 0))["segment"] and segs[6] == parse_rst(enc.write(b, 2, 0))["segment"]
    for bad, r in ((a, 2), (b, 0)):
        with pytest.raises(LibjpegError):
            enc.write(bad, r, 0)
    big = [Guarded(n + 1000) for _ in range(3)]
    up = Uploaded(ims[:3])
    tq.encode_scan_batch(up.batch, outs=[g.view[:c] for g, c in zip(big, caps)], restart_interval=4)
    torch.cuda.synchronize()
    for g, c in zip(big, caps):
        g.check(untouched_from=c)


def test_a_caller_table_without_a_needed_symbol_is_still_status_3(tq, enc):
    a = synth_scan_image(np.random.default_rng(1), (24, 24), [1], [1], 1, amp=3)
    b = synth_scan_image(np.random.default_rng(2), (24, 24), [1], [1], 1, amp=900)
    f = parse_rst(enc.write(a, 2, 0, optimize=True))
    assert set(np.flatnonzero(histogram(b, (0,))[2][:256])) - set(f["ac"][0][1])
    segs, lens, status, _ = _scan(tq, [a, b, a], [2, 2, 2], None, huffman=dict(dc=f["dc"], ac=f["ac"]))
    assert status == [0, 3, 0] and lens[1] == 0
    assert segs[0] == f["segment"] and segs[2] == f["segment"]


def test_histogram_and_optimized_files(tq, enc):
    """the device histogram of a restart scan is the restatement's, and optimize=True gives libjpeg's optimize_coding
    file byte for byte (tests/test_encode_rst_host.py asserts that these tables differ from the no-restart ones)"""
    cases = optimize_cases()
    up = Uploaded([im for im, _ri, _rows in cases])
    ri, rows = [c[1] for c in cases], [c[2] for c in cases]
    r = tq.encode_histogram_batch(up.batch, restart_interval=ri, restart_in_rows=rows)
    torch.cuda.synchronize()
    got = r["counts"].cpu().numpy()
    assert r["status"].cpu().tolist() == [0] * len(cases)
    for k, ((im, i, w), h) in enumerate(zip(cases, got)):
        want = histogram_rst(im, _tbl(im), interval_of(im, i, w))
        assert np.array_equal(h[:, :256], want[:, :256]), f"case {k}"
        assert not np.array_equal(h[:2, :256], histogram(im, _tbl(im))[:2, :256]), f"case {k}"
    files = tq.encode_batch(up.batch, optimize=True, restart_interval=ri, restart_in_rows=rows)
    for k, ((im, i, w), f) in enumerate(zip(cases, files)):
        assert f == enc.write(im, i, w, optimize=True), f"case {k}"
    up.check()


def test_a_workspace_the_run_does_not_know(tq):
    """the run finds what to launch under the address prepare saw.  A copy of a prepared workspace elsewhere runs as a
    workspace without restart jobs: the same bytes when it has none, status 4 and no length for a job whose descriptor
    has an interval (never a segment that silently lacks its markers); another number of jobs is QS_HIP_EINVAL"""
    rng = np.random.default_rng(6)
    ims = [synth_scan_image(rng, (67, 35), [2, 1, 1], [2, 1, 1], 3), synth_scan_image(rng, (40, 24), [1], [1], 1)]
    up = Uploaded(ims)
    plain = tq.encode_scan_batch(up.batch)
    rst = tq.encode_scan_batch(up.batch, restart_interval=[2, 0])
    torch.cuda.synchronize()
    assert rst["status"].cpu().tolist() == [0, 0] and int(rst["len"][0]) > int(plain["len"][0])
    for r, want in ((plain, [0, 0]), (rst, [4, 0])):
        ws = r["workspace"]
        moved = tq.Workspace(buf=ws.buf.clone(), key=ws.key)
        got = tq.encode_scan_batch(up.batch, workspace=moved, restart_interval=None if r is plain else [2, 0])
        torch.cuda.synchronize()
        assert got["status"].cpu().tolist() == want
        for k, st in enumerate(want):
            n = int(plain["len"][k])
            assert int(got["len"][k]) == (0 if st else n)
            if not st:
                assert torch.equal(got["segments"][k][:n], plain["segments"][k][:n])
        h = tq.encode_histogram_batch(up.batch, workspace=tq.Workspace(buf=ws.buf.clone(), key=ws.key),
                                      restart_interval=None if r is plain else [2, 0])
        assert h["status"].cpu().tolist() == want
    hip = pkg.HipQS()
    jobs, dev, _stop = tq._encode_jobs(up.batch, None, "test", torch)
    ws = rst["workspace"]
    length, status = torch.empty(1, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    with pytest.raises(pkg.QsHipError) as e:
        hip.encode_batch(jobs[:1], None, [rst["segments"][0].data_ptr()], [int(rst["segments"][0].numel())],
                         length.data_ptr(), status.data_ptr(), ws.buf.data_ptr(), ws.nbytes,
                         torch.cuda.current_stream(dev).cuda_stream)
    assert e.value.code == -2 and "prepared for 2 jobs" in str(e.value)
    up.check()
