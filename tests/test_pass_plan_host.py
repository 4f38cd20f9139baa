"""The render-pass plan on the host (no GPU): ptsharp_amd/csrc/pt_pass_plan.cpp, what pt_render_pass decides before it
allocates or launches anything (engine, chunks, queue capacities, batch split, side stream, every refusal), driven by
tests/native/pass_plan_check.cpp.  tests/golden/pass_plan_v1.json holds the plans and refusals of the commit before
the plan moved out of pt_api.hip, taken from that commit's own arithmetic: every row reproduces exactly.  The
program's sweep checks each plan of a dense grid of valid inputs against what the queues must hold.  The same
stand-alone program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
EXE = os.path.join(NATIVE, "_build", "pass_plan_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "pass_plan_check_asan")
N_IN = 20   # columns tag .. side_stream are the inputs, the rest the plan

REFUSALS = {
    "spp must be >= 1", "bad sampler", "SpecularModeAll with MaxBounces > 32", "bad light/specular mode",
    "counted passes run one at a time (passes = 1)", "negative extra samples",
    "adaptive / firefly phases run on the wavefront engine",
    "wavefront queues cannot hold one camera sample of this sampler (use the megakernel)", "bad engine",
    "adaptive samples exceed one wavefront chunk", "firefly samples exceed one wavefront chunk"}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "pass_plan_v1.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", NATIVE, "pass_plan_check"], check=True)
    return EXE


def requests(golden):
    """The golden table as the program's request lines, and the answer line each must get."""
    req, want = [], []
    for row in golden["rows"]:
        req.append("plan " + " ".join(str(v) for v in row[1:N_IN]))
        out = dict(zip(golden["columns"][N_IN:], row[N_IN:]))
        want.append(" ".join(str(out[k]) for k in ("rc", "out_engine", "chunk", "chunk_extra", "root_children", "children",
                                                   "lights_per_child", "cap", "scap", "side", "passes_per_launch",
                                                   "split_step")) + "\t" + out["message"])
    for budget, cap in golden["wf_cap_for_budget"]:
        req.append(f"budget {budget}")
        want.append(str(cap))
    for entries, cap in golden["wf_cap_for_limit"]:
        req.append(f"limit {entries}")
        want.append(str(cap))
    for total, per_pass, knob, passes in golden["batch_passes_for"]:
        req.append(f"batch {total} {per_pass} {knob}")
        want.append(str(passes))
    return req, want


def answers(exe, req, env=None):
    r = subprocess.run([exe, "--rows"], input="\n".join(req) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.split("\n")[:-1], r.stderr


def test_golden_table_covers_what_it_should(golden):
    """Every refusal is in the table, and every plan value that selects a path in pt_api.hip."""
    cols = golden["columns"]
    rows = [dict(zip(cols, r)) for r in golden["rows"]]
    assert len(cols) == 33 and cols[N_IN] == "rc" and all(len(r) == 33 for r in golden["rows"])
    assert len({r["tag"] for r in rows}) == len(rows) >= 300
    assert {r["message"] for r in rows if r["rc"]} == REFUSALS
    ok = [r for r in rows if r["rc"] == 0]
    assert {r["out_engine"] for r in ok} == {1, 2} and {r["engine"] for r in rows} >= {0, 1, 2}
    assert {r["wf_max_cap"] for r in rows} >= {8192, 1 << 16, 1 << 20, 1 << 22, 1 << 29}
    assert {r["side_stream"] for r in rows} == {-1, 0, 1} and {r["side"] for r in ok} == {0, 1}
    assert any(r["split_step"] == 1 for r in ok) and any(r["split_step"] > 1 for r in ok)
    assert any(r["passes_per_launch"] > 1 and r["split_step"] == 0 for r in ok)
    assert any(r["chunk_extra"] > r["chunk"] for r in ok) and any(r["stratified"] for r in ok)


def test_every_golden_row_reproduces(built, golden):
    req, want = requests(golden)
    got, _ = answers(built, req)
    assert len(got) == len(want)
    bad = [(q, w, g) for q, w, g in zip(req, want, got) if w != g]
    assert not bad, "\n".join(f"{q}\n  golden {w!r}\n  now    {g!r}" for q, w, g in bad[:10])


def test_plan_sweep_from_first_principles(built):
    r = subprocess.run([built], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    assert r.stdout.strip().endswith("pass_plan_check: 0 failures")
    counts = dict(zip(("plans", "wavefront", "several", "split", "refused"), map(int, re.findall(r"\d+", r.stdout.splitlines()[-2]))))
    assert counts["plans"] > 1_000_000 and counts["wavefront"] > 100_000 and counts["several"] > 100_000
    assert counts["split"] > 100_000


def test_plan_check_sanitized(golden):
    subprocess.run(["make", "-s", "-C", NATIVE, "pass_plan_check_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE_ASAN], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("pass_plan_check: 0 failures")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    req, want = requests(golden)
    got, err = answers(EXE_ASAN, req, env)
    assert got == want
    assert "runtime error" not in err and "AddressSanitizer" not in err
