"""CPU tests of the device-resident job route (include/jpegqs_hip.h: qs_hip_device_job_info, qs_hip_device_job_prepare,
qs_hip_do_quantsmooth_device) and its torch front end (torch_qs.quantsmooth_): what can be decided without a GPU --
the plan against the goldens, the workspace size and argument checking."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import golden_names, load_golden

ROOT = Path(__file__).resolve().parent.parent
EINVAL, ENODEV = -2, -1


def _job(hip, j, ptr=0x10000, coef_up=None):
    """a qs_hip_job over (fake) device addresses with the golden's geometry: the info call never touches them"""
    shapes = [c.shape[:2] for c in j["coefs"]]
    return hip.device_job([ptr + 0x1000000 * ci for ci in range(len(shapes))], shapes, j["quants"], coef_up=coef_up,
                          **j["kw"])


def test_abi_version_is_7(hip):
    assert hip.lib.qs_hip_abi_version() == 7
    hdr = (ROOT / "include" / "jpegqs_hip.h").read_text()
    assert int(re.search(r"#define QS_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 7


def test_device_info_layout_matches_the_header(tmp_path):
    from jpeg_quantsmooth_amd import hipqs
    fs = [f[0] for f in hipqs.DeviceInfo._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "jpegqs_hip.h"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(qs_hip_device_info));']
    src += [f'  printf("{f} %zu\\n", offsetof(qs_hip_device_info, {f}));' for f in fs]
    src += ['  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    out = dict(line.split() for line in subprocess.run([str(tmp_path / "l")], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(hipqs.DeviceInfo)
    for f in fs:
        assert int(out[f]) == getattr(hipqs.DeviceInfo, f).offset, f


@pytest.mark.parametrize("name", golden_names())
def test_info_matches_golden(hip, name):
    """geometry of the replacement chroma, output sampling factors and the table-decided stop, as the reference
    produced them; the workspace holds at least a pixel plane and a snapshot per smoothed component"""
    j, want = load_golden(name)
    info = hip.device_job_info(_job(hip, j), j["flags"], j["niter"])
    big_table = any(q is not None and int(np.max(q)) >= 0x800 for q in j["quants"])
    assert info["static_stop"] == int(big_table)
    if big_table:
        assert want["ret"] == 1
    if want["ret"] == 0 or big_table:                       # (a tripped range check is decided on the device)
        assert (info["up_wblk"] > 0) == want["up"]
        assert (info["out_hsamp0"], info["out_vsamp0"]) == (want["hsamp0"], want["vsamp0"])
        if want["up"]:
            assert (info["up_hblk"], info["up_wblk"]) == want["coefs"][1].shape[:2] == want["coefs"][2].shape[:2]
    if not big_table and j["niter"] > 0 and all(q is not None and int(np.max(q)) > 1 for q in j["quants"]):
        need = sum(hip.plane_bytes(c.shape[1], c.shape[0]) + c.nbytes for c in j["coefs"])
        assert info["workspace_bytes"] >= need


def test_info_early_out_and_rejects(hip, pkg, synth):
    coef, quant = synth.synth_gray(64, 48, 50)
    job = hip.device_job([0x10000], [coef.shape[:2]], [quant])
    info = hip.device_job_info(job, 1, 0)                    # niter 0: the reference's early out (:2458)
    assert info["static_stop"] == 0 and info["up_wblk"] == 0 and info["workspace_bytes"] > 0
    assert hip.device_job_info(job, 1, 3)["workspace_bytes"] > info["workspace_bytes"]
    bad = hip.device_job([0x10000], [(0, 8)], [quant])
    with pytest.raises(pkg.QsHipError) as ei:
        hip.device_job_info(bad, 1, 3)
    assert ei.value.code == EINVAL


def test_run_rejects_bad_arguments(hip, pkg):
    """EINVAL for a short workspace, a null stop word and missing coef_up -- checked before anything is enqueued"""
    j, _ = load_golden("ycc420_141x93_q6_n2")
    job = _job(hip, j)
    info = hip.device_job_info(job, j["flags"], j["niter"])
    assert info["up_wblk"] > 0
    n = info["workspace_bytes"]
    cases = [(n - 1, 0x8000, None), (n, 0, None), (n, 0x8000, None), (n, 0x8000, (0x9000, None))]
    for nbytes, d_stop, up in cases:
        job = _job(hip, j, coef_up=up)
        with pytest.raises(pkg.QsHipError) as ei:
            hip.do_quantsmooth_device(job, j["flags"], j["niter"], 0x20000, nbytes, d_stop)
        assert ei.value.code == EINVAL, (nbytes, d_stop, up)
    with pytest.raises(pkg.QsHipError) as ei:
        hip.do_quantsmooth_device(_job(hip, j, coef_up=(0x9000, 0xa000)), j["flags"], j["niter"], 0, n, 0x8000)
    assert ei.value.code == EINVAL
    with pytest.raises(pkg.QsHipError) as ei:
        hip.device_job_prepare(_job(hip, j), j["flags"], j["niter"], 0x20000, n - 1)
    assert ei.value.code == EINVAL


def test_run_without_device_is_enodev(hip, pkg):
    """valid arguments and no device: ENODEV, nothing computed on the CPU"""
    if hip.device_count() > 0:
        pytest.skip("a GPU is present: the fake device addresses of this test must not reach it")
    j, _ = load_golden("ycc420_141x93_q6_n2")
    job = _job(hip, j, coef_up=(0x9000, 0xa000))
    n = hip.device_job_info(job, j["flags"], j["niter"])["workspace_bytes"]
    with pytest.raises(pkg.QsHipError) as ei:
        hip.do_quantsmooth_device(job, j["flags"], j["niter"], 0x20000, n, 0x8000)
    assert ei.value.code == ENODEV
    with pytest.raises(pkg.QsHipError) as ei:
        hip.device_job_prepare(job, j["flags"], j["niter"], 0x20000, n)
    assert ei.value.code == ENODEV


def test_torch_front_end_checks_tensors(pkg):
    """CPU, wrong dtype, non-contiguous and wrongly shaped tensors are refused before the library is called"""
    import torch
    from jpeg_quantsmooth_amd import torch_qs
    q = np.full(64, 16, dtype=np.uint16)
    with pytest.raises(ValueError, match="CUDA"):
        torch_qs.quantsmooth_([torch.zeros((4, 4, 64), dtype=torch.int16)], [q], 0, 3)
    def fake(shape, dtype=torch.int16, contiguous=True):      # (host tensors: these checks come before the device's)
        t = torch.zeros(shape, dtype=dtype)
        return t.transpose(0, 1) if not contiguous else t
    with pytest.raises(TypeError, match="int16"):
        torch_qs.quantsmooth_([fake((4, 4, 64), dtype=torch.int32)], [q], 0, 3)
    with pytest.raises(ValueError, match="contiguous"):
        torch_qs.quantsmooth_([fake((4, 5, 64), contiguous=False)], [q], 0, 3)
    with pytest.raises(ValueError, match="shape"):
        torch_qs.quantsmooth_([fake((4, 4, 63))], [q], 0, 3)
    with pytest.raises(ValueError, match="shape"):
        torch_qs.quantsmooth_([fake((4, 64))], [q], 0, 3)
    with pytest.raises(TypeError, match="torch.Tensor"):
        torch_qs.quantsmooth_([np.zeros((4, 4, 64), np.int16)], [q], 0, 3)


def test_package_import_does_not_import_torch():
    r = subprocess.run([sys.executable, "-c", "import sys, jpegqs_pkg; p = jpegqs_pkg.load(); p.quantsmooth_; "
                        "print('torch' in sys.modules)"], cwd=ROOT, capture_output=True, text=True, check=True)
    assert r.stdout.strip() == "False"
