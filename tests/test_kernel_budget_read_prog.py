"""csrc/check_kernel_budget.py --no-scratch, the build guard of the kernels of the scan reader's progressive route
(csrc/qs_kernels_read_prog.hip): each of them is in the code-object metadata, and none uses scratch."""
import subprocess
import sys

from test_kernel_budget import CSRC, _asm, _record

KERNELS = ("qrp_init", "qrp_check", "qrp_decode")


def _name(k):
    return f"_ZN12_GLOBAL__N_1{len(k)}{k}E7QrpArgs"


def _run(tmp_path, text):
    f = tmp_path / "k.s"
    f.write_text(text)
    return subprocess.run([sys.executable, str(CSRC / "check_kernel_budget.py"), "--no-scratch", "qrp_", str(f)],
                          capture_output=True, text=True, timeout=60)


def test_no_scratch_met(tmp_path):
    other = _record("_ZN12_GLOBAL__N_19qr_decodeE6QrArgs", vgprs=60, scratch=104, lds=7400)   # none of its business
    r = _run(tmp_path, _asm([other] + [_record(_name(k), vgprs=93, lds=3856) for k in KERNELS]))
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("0 B scratch") == len(KERNELS)


def test_scratch_or_a_missing_kernel_fails(tmp_path):
    recs = [_record(_name(k), vgprs=93, lds=3856) for k in KERNELS]
    r = _run(tmp_path, _asm(recs[:2] + [_record(_name("qrp_decode"), vgprs=81, scratch=64, lds=3856)]))
    assert r.returncode == 1 and "qrp_decode" in r.stderr and "scratch" in r.stderr
    r = _run(tmp_path, _asm(recs[:-1]))
    assert r.returncode == 1 and "expected the metadata of one kernel qrp_decode" in r.stderr


def test_makefile_checks_the_kernels_and_the_source_defines_them():
    mk = (CSRC / "Makefile").read_text()
    assert "check_kernel_budget.py --no-scratch qrp_ qs_kernels_read_prog.isa.s" in mk
    assert "qs_kernels_read_prog.o qs_read_prog_job.o" in mk            # linked: a build without them does not link
    src = (CSRC / "qs_kernels_read_prog.hip").read_text()
    for k in KERNELS:
        assert f") {k}(QrpArgs a)" in src, k
