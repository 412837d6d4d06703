"""The workspace rules of torch_qs, stage by stage, on the smallest batch that takes every branch -- one 16x16 gray
image and one 32x16 4:2:0 image: a workspace passed again is not prepared again, one that was prepared for another
geometry or by another stage is prepared exactly once, and a buffer that is too small is replaced in place (in a new
Workspace by the smoothing calls).  HipQS.*_prepare is counted; results are compared with a call on a fresh workspace."""
import numpy as np
import pytest

import jpegqs_pkg
from compress_oracle import pixels
from decode_oracle import synth_image
from encode_oracle import synth_scan_image

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
tq, jpeg_file = pkg.torch_qs, pkg.jpeg_file

GEOMETRY = [((16, 16), [1], [1], 1), ((32, 16), [2, 1, 1], [2, 1, 1], 3)]
BATCH, SWAPPED, SMALL = (0, 1), (1, 0), (0,)
FLAGS = pkg.flags_for_quality(4)


def _kw(im):
    return dict(hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"], image_size=im["image_size"])


def _upload(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _on_device(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


@pytest.fixture(scope="module")
def src():
    """the host inputs of every stage, made once: coefficient arrays from each stage's own generator, pixels, and the
    files of the readers (written by the device coders, with a restart interval)"""
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible to torch")
    rng = np.random.default_rng(2024)
    gray, quant = pkg.synth.synth_gray(16, 16, 50)
    ycc = pkg.synth.synth_ycc(32, 16, 2, 2, quality=50, seed=5)
    s = dict(smooth=[dict(coefs=[gray], quants=[quant], hsamp=[1], vsamp=[1], colorspace=1, image_size=(16, 16)),
                     dict(coefs=ycc["coefs"], quants=ycc["quants"], hsamp=[2, 1, 1], vsamp=[2, 1, 1], colorspace=3,
                          image_size=(32, 16))],
             decode=[synth_image(rng, *g) for g in GEOMETRY], scan=[synth_scan_image(rng, *g) for g in GEOMETRY],
             pixels=[pixels(rng, g[0], len(g[1])) for g in GEOMETRY], files=[], progressive=[])
    for im in s["scan"]:
        s["files"].append(tq.encode(_upload(im["coefs"]), im["quants"], **_kw(im), restart_interval=1))
        n = len(im["coefs"])
        script = jpeg_file.simple_progression(3, 3) if n == 3 else jpeg_file.spectral_script(1)
        r = tq.encode_file(_upload(im["coefs"]), im["quants"], **_kw(im), scans=script, refinement=True, restart_interval=1)
        assert int(r["status"][0]) == 0
        s["progressive"].append(r["file"][:int(r["len"][0])].cpu().numpy().tobytes())
    return s


def _images(items, idx):
    return [dict(coefs=_upload(items[k]["coefs"]), quants=items[k]["quants"], **_kw(items[k])) for k in idx]


def _cut(bufs, r):
    """the bytes written, the lengths and whatever else the coder reports, after a look at the statuses"""
    assert r["status"].cpu().tolist() == [0] * len(bufs)
    return [b[:n] for b, n in zip(bufs, r["len"].cpu().tolist())] + [r["len"]]


def _smooth(src, idx, ws):
    images = _images(src["smooth"], idx)                                # (fresh arrays: the call rewrites them)
    r = tq.quantsmooth_batch_(images, FLAGS, 1, workspace=ws)
    return [t for im in images for t in im["coefs"]] + [r["stop"]], r["workspace"]


def _decode(src, idx, ws):
    r = tq.decode_batch(_images(src["decode"], idx), workspace=ws)
    return r["images"], r["workspace"]


def _scan(src, idx, ws):
    r = tq.encode_scan_batch(_images(src["scan"], idx), workspace=ws)
    return _cut(r["segments"], r), r["workspace"]


def _files(src, idx, ws):
    r = tq.encode_file_batch(_images(src["scan"], idx), optimize=True, workspace=ws)
    return _cut(r["files"], r) + [r["tables"]], r["workspace"]


def _scripts(src, idx, ws):
    scripts = [jpeg_file.spectral_script(len(src["scan"][k]["coefs"])) for k in idx]
    r = tq.encode_file_batch(_images(src["scan"], idx), scans=scripts, workspace=ws)
    return _cut(r["files"], r), r["workspace"]


def _read_with(call, files, **kw):
    def run(src, idx, ws):
        r = call([_on_device(src[files][k]) for k in idx], workspace=ws, **kw)
        assert r["status"].cpu().tolist() == [0] * len(idx)
        return [t for im in r["images"] for t in im["coefs"]], r["workspace"]
    return run


def _compress(src, idx, ws):
    images = [dict(pixels=torch.from_numpy(src["pixels"][k]).cuda(), quality=50, hsamp=GEOMETRY[k][1], vsamp=GEOMETRY[k][2])
              for k in idx]
    r = tq.compress_batch(images, workspace=ws)
    return [t for im in r["images"] for t in im["coefs"]], r["workspace"]


# stage -> (its run, the HipQS prepare it goes through, the stage whose workspace it is handed in the foreign test)
STAGES = {
    "quantsmooth_batch_": (_smooth, "device_batch_prepare", "decode_batch"),
    "decode_batch": (_decode, "decode_batch_prepare", "encode_scan_batch"),
    "encode_scan_batch": (_scan, "encode_batch_prepare", "decode_batch"),
    "encode_file_batch-optimize": (_files, "encode_batch_prepare", "read_batch"),
    "encode_file_batch-scans": (_scripts, "encode_progressive_prepare", "encode_file_batch-optimize"),
    "read_batch": (_read_with(tq.read_batch, "files"), "read_batch_prepare", "read_batch-split"),
    "read_batch-split": (_read_with(tq.read_batch, "files", split=True), "read_batch_prepare", "read_progressive_batch"),
    "read_progressive_batch": (_read_with(tq.read_progressive_batch, "progressive"), "read_prog_batch_prepare", "compress_batch"),
    "compress_batch": (_compress, "compress_batch_prepare", "quantsmooth_batch_"),
}
IN_PLACE = [s for s in STAGES if s != "quantsmooth_batch_"]


@pytest.fixture
def prepares(monkeypatch, stage):
    """the calls of the stage's HipQS prepare, counted on their way through"""
    name = STAGES[stage][1]
    inner, calls = getattr(pkg.HipQS, name), []

    def counted(self, *a, **kw):
        calls.append(name)
        return inner(self, *a, **kw)
    monkeypatch.setattr(pkg.HipQS, name, counted)
    return calls


def _same(got, want):
    return len(got) == len(want) and all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("stage", list(STAGES))
def test_a_workspace_passed_again_is_not_prepared_again(src, stage, prepares):
    run = STAGES[stage][0]
    first, ws = run(src, BATCH, None)
    assert len(prepares) == 1 and ws.key is not None
    again, ws2 = run(src, BATCH, ws)
    assert len(prepares) == 1 and _same(again, first)
    assert ws2 is ws or stage not in IN_PLACE


@pytest.mark.parametrize("stage", list(STAGES))
def test_another_geometry_prepares_once(src, stage, prepares):
    run = STAGES[stage][0]
    want, _ws = run(src, SWAPPED, None)
    _out, ws = run(src, BATCH, None)
    key, n = ws.key, len(prepares)
    got, ws2 = run(src, SWAPPED, ws)
    assert len(prepares) == n + 1 and _same(got, want) and ws2.key != key
    assert ws2 is ws or stage not in IN_PLACE


@pytest.mark.parametrize("stage", list(STAGES))
def test_a_workspace_of_another_stage_is_prepared_once(src, stage, prepares):
    run, _name, donor = STAGES[stage]
    want, fresh = run(src, BATCH, None)
    _out, ws = STAGES[donor][0](src, BATCH, None)
    assert ws.key != fresh.key
    n = len(prepares)
    got, ws2 = run(src, BATCH, ws)
    assert len(prepares) == n + 1 and _same(got, want) and ws2.key == fresh.key
    assert ws2 is ws or stage not in IN_PLACE


@pytest.mark.parametrize("stage", list(STAGES))
def test_a_buffer_too_small_is_replaced(src, stage, prepares):
    """in place by every stage but the smoothing, which returns a new Workspace and leaves the passed one as it was"""
    run = STAGES[stage][0]
    want, fresh = run(src, BATCH, None)
    _out, ws = run(src, SMALL, None)
    buf, size, key = ws.buf, ws.nbytes, ws.key
    assert size < fresh.nbytes, "the batch of one must need less than the batch of two"
    n = len(prepares)
    got, ws2 = run(src, BATCH, ws)
    assert len(prepares) == n + 1 and _same(got, want) and ws2.nbytes >= fresh.nbytes and ws2.key == fresh.key
    if stage in IN_PLACE:
        assert ws2 is ws and ws.buf is not buf
    else:
        assert ws2 is not ws and ws.buf is buf and ws.nbytes == size and ws.key == key
