"""csrc/check_kernel_budget.py, the build guard of the recovery kernels' register / scratch / LDS budget: reads the
code-object metadata block of a device assembly and nothing else."""
import subprocess
import sys
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "jpeg-quantsmooth_amd" / "csrc"
NAMES = ("_Z22qs_smooth_plane_kernelILb1EEvPK8QsConstsPsPKhPhiiiiiiii", "_Z22qs_smooth_plane_kernelILb0EEvPK8QsConstsPsPKhPhiiiiiiii",
         "_Z20qs_smooth_set_kernelILb1EEv10QsPlaneSeti", "_Z20qs_smooth_set_kernelILb0EEv10QsPlaneSeti")


def _record(name, vgprs=161, scratch=0, lds=53760):
    return f"""  - .args:
      - .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .group_segment_fixed_size: {lds}
    .kernarg_segment_align: 8
    .language_version:
      - 2
      - 0
    .name:           {name}
    .private_segment_fixed_size: {scratch}
    .sgpr_count:     106
    .symbol:         {name}.kd
    .vgpr_count:     {vgprs}
    .vgpr_spill_count: 0
"""


def _asm(records):
    # an instruction that would trip a scan of the code stands in front: the guard must not look at it
    return ("\t.text\n\tv_mov_b32 v200, 0\n\t.amdgpu_metadata\n---\namdhsa.kernels:\n"
            + "".join(records) + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\n\t.end_amdgpu_metadata\n")


def _run(tmp_path, text):
    f = tmp_path / "k.s"
    f.write_text(text)
    return subprocess.run([sys.executable, str(CSRC / "check_kernel_budget.py"), str(f)], capture_output=True, text=True, timeout=60)


def test_budget_met(tmp_path):
    other = _record("_Z15qs_clamp_kernelPsm", vgprs=13, scratch=64, lds=0)      # other kernels are none of its business
    r = _run(tmp_path, _asm([other] + [_record(n, vgprs=168, lds=54612) for n in NAMES]))
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("168 VGPRs, 0 B scratch") == 4


@pytest.mark.parametrize("kw,why", [({"scratch": 4}, "scratch"), ({"vgprs": 169}, "169 VGPRs > 168"), ({"lds": 54614}, "LDS > 54613")])
def test_budget_missed(tmp_path, kw, why):
    recs = [_record(n) for n in NAMES[:3]] + [_record(NAMES[3], **kw)]
    r = _run(tmp_path, _asm(recs))
    assert r.returncode == 1 and why in r.stderr and NAMES[3] in r.stderr


def test_budget_needs_all_four_kernels(tmp_path):
    r = _run(tmp_path, _asm([_record(n) for n in NAMES[:3]]))
    assert r.returncode == 1 and "expected the metadata of 4 recovery kernels" in r.stderr


def test_makefile_asks_for_the_budget_check():
    mk = (CSRC / "Makefile").read_text()
    assert "QS_BUDGET_CHECK=1" in mk and "check_kernel_budget.py" in mk
    assert "check_kernel_budget.py" in (CSRC / "build_stripped.sh").read_text()
