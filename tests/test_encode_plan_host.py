"""The registry of prepared workspaces and the restart rule the two encoder drivers share (csrc/qs_encode_plan.h), compiled
for the host without HIP (tests/encode_plan_host.cpp) and run as a program of its own: once plain, once under the address
and undefined-behaviour sanitizers.  A registry of cap 3 evicts the entry stored longest ago on the fourth store, storing
an address again refreshes its age, an evicted or unknown address misses, and a value a lookup handed out stays valid
after its address is stored again; the restart rule gives the values written out in the program."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
CSRC = HERE.parent / "jpeg-quantsmooth_amd" / "csrc"


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_registry_and_restart_rule_on_the_host(flags, tmp_path):
    exe = tmp_path / "encode_plan_host"
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, f"-I{CSRC}", "-o", str(exe),
                        str(HERE / "encode_plan_host.cpp")], capture_output=True, text=True)
    if r.returncode or not exe.exists():
        pytest.fail(f"tests/encode_plan_host.cpp did not build:\n{r.stderr}")
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert (run.returncode, run.stdout.strip(), run.stderr.strip()) == (0, "ok", "")
