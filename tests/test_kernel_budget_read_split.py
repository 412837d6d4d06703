"""csrc/check_kernel_budget.py --no-scratch, the build guard of the scan reader's split kernels
(csrc/qs_kernels_read_split.hip): each of them is in the code-object metadata, and none uses scratch."""
import subprocess
import sys

from test_kernel_budget import CSRC, _asm, _record

KERNELS = ("qrs_map", "qrs_decode", "qrs_count", "qrs_tile_scan", "qrs_write", "qrs_dc_tiles", "qrs_dc_write")


def _name(k):
    return f"_ZN12_GLOBAL__N_1{len(k)}{k}E7QrsArgs"


def _run(tmp_path, text):
    f = tmp_path / "k.s"
    f.write_text(text)
    return subprocess.run([sys.executable, str(CSRC / "check_kernel_budget.py"), "--no-scratch", "qrs_", str(f)],
                          capture_output=True, text=True, timeout=60)


def test_no_scratch_met(tmp_path):
    other = _record("_ZN12_GLOBAL__N_19qr_decodeE6QrArgs", vgprs=60, scratch=104, lds=7400)   # none of its business
    r = _run(tmp_path, _asm([other] + [_record(_name(k), vgprs=60, lds=9624) for k in KERNELS]))
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("0 B scratch") == len(KERNELS)


def test_scratch_or_a_missing_kernel_fails(tmp_path):
    recs = [_record(_name(k), vgprs=45, lds=7440) for k in KERNELS]
    r = _run(tmp_path, _asm(recs[:4] + [_record(_name("qrs_write"), vgprs=60, scratch=104, lds=9624)] + recs[5:]))
    assert r.returncode == 1 and "qrs_write" in r.stderr and "scratch" in r.stderr
    r = _run(tmp_path, _asm(recs[:-1]))
    assert r.returncode == 1 and "expected the metadata of one kernel qrs_dc_write" in r.stderr


def test_makefile_checks_the_split_kernels_and_the_source_defines_them():
    mk = (CSRC / "Makefile").read_text()
    assert "check_kernel_budget.py --no-scratch qrs_ qs_kernels_read_split.isa.s" in mk
    src = (CSRC / "qs_kernels_read_split.hip").read_text()
    for k in KERNELS:
        assert f") {k}(QrsArgs x)" in src, k
