"""The table kernel (torch_qs.huff_optimal_device, qs_hip_huff_optimal_device) on the GPU against the host entry point
qs_hip_huff_optimal, which runs the same header (csrc/qs_huff.h) in its host form and is pinned to libjpeg in
tests/test_huff_host.py."""
import numpy as np
import pytest

import jpegqs_pkg
from helpers import Guarded
from huff_oracle import edge_histograms, seeded_histograms

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tq():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible to torch")
    return pkg.torch_qs


@pytest.fixture(scope="module")
def reference():
    """the histograms (the CPU list's and 300 seeded ones) and what the host function makes of each: (bits, huffval), or
    None where it refuses -- computed once"""
    hip = pkg.HipQS()
    hs = [h for _n, h in edge_histograms()] + seeded_histograms(300, 20)
    want = []
    for h in hs:
        try:
            want.append(hip.huff_optimal(h))
        except pkg.hipqs.QsHipError as e:
            assert e.code == -2
            want.append(None)
    assert sum(w is None for w in want) > 3 and want[0] == ([0] * 17, [])
    return hs, want


@pytest.mark.parametrize("ntables", [1, 4, 129])
def test_table_kernel_equals_the_host_function(tq, reference, ntables):
    """1, 4 and 129 tables in a launch (a partly filled last workgroup), every histogram in turn; entry 256 of the counts
    holds junk, which is ignored; outputs between sentinel margins"""
    hip = pkg.HipQS()
    hs, want = reference
    rng = np.random.default_rng(ntables)
    for first in range(0, len(hs), ntables):
        idx = [(first + k) % len(hs) for k in range(ntables)]
        counts = np.zeros((ntables, 257), np.uint32)
        for row, i in enumerate(idx):
            counts[row, :256] = hs[i]
        counts[:, 256] = rng.integers(0, 2 ** 32, ntables, dtype=np.uint64).astype(np.uint32)
        gc, gt, gs = Guarded(ntables * 257, torch.int32), Guarded(ntables * 273), Guarded(ntables, torch.int32)
        gc.view.copy_(torch.from_numpy(counts.view(np.int32).reshape(-1)))
        hip.huff_optimal_device(gc.view.data_ptr(), ntables, gt.view.data_ptr(), gs.view.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for g in (gc, gt, gs):
            g.check()
        assert np.array_equal(gc.view.cpu().numpy().view(np.uint32).reshape(ntables, 257), counts)
        tables, status = gt.view.cpu().numpy().reshape(ntables, 273), gs.view.cpu().tolist()
        for row, i in enumerate(idx):
            bits, vals = tables[row, :17].tolist(), tables[row, 17:].tolist()
            if want[i] is None:
                assert status[row] == 5 and not any(bits) and not any(vals), f"histogram {i}"
            else:
                assert status[row] == 0 and (bits, vals[:sum(bits)]) == want[i] and not any(vals[sum(bits):]), f"histogram {i}"


def test_tensor_call(tq, reference):
    hs, want = reference
    counts = torch.from_numpy(np.stack([np.append(h, 1) for h in hs[:40]]).astype(np.uint32).view(np.int32)).cuda()
    r = tq.huff_optimal_device(counts.view(10, 4, 257))
    torch.cuda.synchronize()
    assert r["bits"].shape == (40, 17) and r["huffval"].shape == (40, 256) and r["status"].shape == (40,)
    for k in range(40):
        bits = r["bits"][k].cpu().tolist()
        if want[k] is None:
            assert int(r["status"][k]) == 5
        else:
            assert int(r["status"][k]) == 0 and (bits, r["huffval"][k].cpu().tolist()[:sum(bits)]) == want[k]
    with pytest.raises(ValueError):
        tq.huff_optimal_device(counts.view(-1))
