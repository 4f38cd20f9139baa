"""Where the dropping shade runs, on the host (no GPU): pt::choose_kernels' WfChoice::escape_drop_depths
(ptsharp_amd/csrc/pt_pass_plan.cpp), checked by tests/native/escape_plan_check.cpp from the inputs alone: only under
the head family, the lean shade, a black untextured environment and PT_ESCAPE_DROP not 0; the camera hits only by
default, every depth under PT_ESCAPE_DROP=all; no other field of the choice moves.  Once more under AddressSanitizer
and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

import pytest

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


@pytest.mark.parametrize("target,exe,env", [
    ("escape_plan_check", "escape_plan_check", {}),
    ("asan", "escape_plan_check_asan", {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}),
])
def test_escape_plan_check(target, exe, env):
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "escape.mk", target], check=True)
    r = subprocess.run([os.path.join(NATIVE, "_build", exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "escape_plan_check: 0 failures"
    rows, on = map(int, re.match(r"rows (\d+), dropping shade in (\d+)", lines[-2]).groups())
    assert 0 < on < rows
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
