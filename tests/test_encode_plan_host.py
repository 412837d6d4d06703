"""The registry of prepared workspaces and the restart rule the two encoder drivers share (csrc/qs_encode_plan.h), compiled
for the host without HIP (tests/encode_plan_host.cpp) and run as a program of its own: once plain, once under the address
and undefined-behaviour sanitizers.  A registry of cap 3 evicts the entry stored longest ago on the fourth store, storing
an address again refreshes its age, an evicted or unknown address misses, and a value a lookup handed out stays valid
after its address is stored again; the restart rule gives the values written out in the program."""
import subprocess

import pytest

from host_tools import build


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_registry_and_restart_rule_on_the_host(sanitize):
    exe = build("encode_plan_host.cpp", flags=["-Wextra", "-Werror"], sanitize=sanitize)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert (run.returncode, run.stdout.strip(), run.stderr.strip()) == (0, "ok", "")
