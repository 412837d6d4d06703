"""The crafted streams of tests/crafted_streams.py on the GPU -- one file per refusal rule of the three scan readers and
its accepted twin on the boundary, green on the host builds of the same headers in tests/test_reader_rules_host.py
before this runs anywhere: per route one batch longer than a launch chunk in which refused and accepted files alternate,
through the C ABI with every file, array, status buffer and workspace between sentinel margins (the Batch helpers of the
three reader modules check them), and through torch_qs.read_batch / read_progressive_batch.  The statuses are those of
tests/golden/reader_rules.json, the accepted arrays libjpeg 9's; a refused job leaves its neighbours alone."""
import json

import numpy as np
import pytest

import jpegqs_pkg
from crafted_streams import FIXTURE, OK, all_cases, read_case
from read_oracle import LibjpegReader
from test_gpu_read import Batch as IntervalBatch
from test_gpu_read_prog import Batch as ProgBatch
from test_gpu_read_split import Batch as SplitBatch

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
CHUNK = 32                         # QS_RD_CHUNK / QS_HIP_READ_CHUNK: jobs per launch chunk


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    lj = LibjpegReader(tmp_path_factory.mktemp("gpurules"))
    rows = json.loads(FIXTURE.read_text())
    out = [dict(read_case(lj, c), status=r["status"]) for c, r in zip(all_cases(), rows)]
    assert [c["name"] for c in out] == [r["name"] for r in rows]
    return out


@pytest.fixture(scope="module")
def tq():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible to torch")
    return pkg.torch_qs


def _alternating(cases):
    """refused, accepted, refused, ...: every refused file between two accepted ones, longer than a launch chunk"""
    bad, good = [c for c in cases if c["want_status"] != OK], [c for c in cases if c["want_status"] == OK]
    out = [good[-1]]
    for k, c in enumerate(bad):
        out += [c, good[k % len(good)]]
    assert len(out) > CHUNK and all(a["want_status"] == OK or b["want_status"] == OK for a, b in zip(out, out[1:]))
    return out


def _check(batch, route, status, arrs):
    for c, s, a in zip(batch, status, arrs):
        assert s == c["status"][route] == c["want_status"], (route, c["name"], s)
        if s == OK:
            for ci, (got, want) in enumerate(zip(a, c["want"])):
                assert np.array_equal(got, want), f"{route}: {c['name']}: component {ci} differs from libjpeg's"


@pytest.mark.parametrize("route", ["interval", "split", "progressive"])
def test_c_abi_reports_the_fixture_status_and_leaves_neighbours_alone(cases, route):
    """one batch per route, then once more over arrays filled with 0x5a5a"""
    batch = _alternating([c for c in cases if route in c["status"]])
    b = {"interval": IntervalBatch, "split": SplitBatch, "progressive": ProgBatch}[route](batch)
    _check(batch, route, *b.run())
    b.fill(0x5a5a)
    _check(batch, route, *b.run())


@pytest.mark.parametrize("route", ["interval", "split", "progressive"])
def test_torch_layer_reports_the_fixture_status(tq, cases, route):
    """the same files as bytes through the wrappers, whose parsers accept every one of them"""
    batch = _alternating([c for c in cases if route in c["status"]])
    datas = [c["data"] for c in batch]
    r = tq.read_progressive_batch(datas) if route == "progressive" else tq.read_batch(datas, split=route == "split")
    torch.cuda.synchronize()
    status = r["status"].cpu().tolist()
    true = [[t.cpu().numpy() for t in im["coefs"]] for im in r["images"]]
    _check(batch, route, status, true)
