"""Which kernels a wavefront pass launches, on the host (no GPU): pt::choose_kernels (ptsharp_amd/csrc/pt_pass_plan.cpp),
driven by tests/native/pass_plan_check.cpp, against tests/wf_choice_ref.py, the restatement of depth_loop's predicates
and launch ladders as they stood before the choice moved out of pt_wavefront.hip.  tests/golden/wf_kernel_choice_v1.json
holds named rows of that restatement: every distinct outcome and both sides of every boundary.  The program's own sweep
checks every choice of the whole grid against what must hold of it, and runs once more under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import json
import os
import re
import subprocess

import pytest

import wf_choice_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
EXE = os.path.join(NATIVE, "_build", "pass_plan_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "pass_plan_check_asan")
N_IN = 1 + len(ref.COLUMNS)   # the tag, then the inputs

# The grid: every combination of these values (full_geom at most full).  31 850 496 rows; the C++ sweep visits all
# of them, the comparison with the Python restatement every STRIDE-th one in the order below (the last column
# fastest).  STRIDE is prime and every column has 2, 3 or 4 values, so every value of every column, and every pair of
# values of two columns, is met many times over; the golden table adds each boundary from both sides by name.
GRID = (("tri_num_nodes", (0, 1, ref.K_LANES_MIN_NODES, ref.K_LANES_MIN_NODES + 1)),
        ("ana_count", (0, ref.K_LIN_RECS, ref.K_LIN_RECS + 1)),
        ("num_planes", (0, ref.K_LIN_PLANES, ref.K_LIN_PLANES + 1)),
        ("num_lights", (1, ref.K_LDS_LIGHTS, ref.K_LDS_LIGHTS + 1)),
        ("ana_num_nodes", (0, 3)),
        (("full", "full_geom"), ((0, 0), (1, 0), (1, 1))),
        ("ana_linear", (0, 1)), ("lights_lean", (0, 1)), ("shade_route", (0, 1)), ("env_tex", (-1, 0)),
        ("sdf_lds", (0, 64)), ("vol_lds", (0, 64)), ("num_sdf", (0, 2)), ("num_vol", (0, 1)),
        ("volq", (0, 1)), ("volq_sh", (0, 1)),
        ("lanes", (-1, 0, 1)), ("head", (0, 1)), ("linear", (-1, 0)), ("tail_early", (0, 1)), ("counted", (0, 1)))
GRID_ROWS = 31_850_496
STRIDE = 251

BOUNDARIES = (("tri_num_nodes", 0, 1), ("tri_num_nodes", ref.K_LANES_MIN_NODES, ref.K_LANES_MIN_NODES + 1),
              ("ana_count", ref.K_LIN_RECS, ref.K_LIN_RECS + 1), ("num_planes", ref.K_LIN_PLANES, ref.K_LIN_PLANES + 1),
              ("num_lights", ref.K_LDS_LIGHTS, ref.K_LDS_LIGHTS + 1), ("ana_num_nodes", 0, 3), ("env_tex", -1, 0),
              ("sdf_lds", 0, 64), ("vol_lds", 0, 64), ("num_sdf", 0, 2), ("num_vol", 0, 1))


def grid_row(i):
    """Row i of the grid, in ref.COLUMNS' order."""
    r = {}
    for name, values in reversed(GRID):
        i, k = divmod(i, len(values))
        if isinstance(name, tuple):
            r.update(zip(name, values[k]))
        else:
            r[name] = values[k]
    return [r[c] for c in ref.COLUMNS]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "wf_kernel_choice_v1.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", NATIVE, "pass_plan_check"], check=True)
    return EXE


def sweep_counts(exe, env=None):
    """The program's sweep: it must pass; the counts of its `choices` line."""
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("pass_plan_check: 0 failures")
    line = r.stdout.splitlines()[-3]
    assert line.startswith("choices ")
    total, distinct = map(int, re.match(r"choices (\d+): distinct (\d+);", line).groups())
    trace, shadow = (dict((n, int(v)) for n, v in re.findall(r"(\w+) (\d+)", part)) for part in line.split(";")[1:])
    return total, distinct, trace, shadow, r.stderr


@pytest.fixture(scope="module")
def swept(built):
    return sweep_counts(built)


def answers(exe, rows, env=None):
    req = "".join("choice " + " ".join(map(str, r)) + "\n" for r in rows)
    r = subprocess.run([exe, "--rows"], input=req, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.split("\n")[:-1], r.stderr


def test_grid_is_the_whole_product():
    n = 1
    for _, values in GRID:
        n *= len(values)
    assert n == GRID_ROWS
    assert grid_row(0) != grid_row(1) and grid_row(GRID_ROWS - 1)[-1] == 1
    assert all(f >= g for f, g in (grid_row(i)[:2] for i in range(0, GRID_ROWS, 65_537)))


def test_choice_equals_the_restated_ladders(built):
    rows = [grid_row(i) for i in range(0, GRID_ROWS, STRIDE)]
    for k, (name, values) in enumerate(GRID):   # every value of every column is among them
        cols = [ref.COLUMNS.index(c) for c in (name if isinstance(name, tuple) else (name,))]
        seen = {tuple(r[c] for c in cols) for r in rows}
        assert seen == {v if isinstance(v, tuple) else (v,) for v in values}, name
    got, _ = answers(built, rows)
    assert len(got) == len(rows)
    bad = [(r, ref.choose(*r), g) for r, g in zip(rows, got) if ref.choose(*r) != g]
    assert not bad, "\n".join(f"{r}\n  restated {w!r}\n  now      {g!r}" for r, w, g in bad[:10])


def test_golden_table_covers_what_it_should(golden, swept):
    """Every distinct outcome of the whole grid at least once, and each boundary from both sides: a pair of rows that
    differ in that input alone and choose differently."""
    cols = golden["columns"]
    assert cols == ["tag"] + list(ref.COLUMNS) + list(ref.OUT_COLUMNS)
    rows = golden["rows"]
    assert all(len(r) == len(cols) for r in rows)
    assert len({r[0] for r in rows}) == len(rows) and 200 <= len(rows) <= 500
    outcomes = {tuple(r[N_IN:]) for r in rows}
    assert len(outcomes) == swept[1]
    out = [dict(zip(ref.OUT_COLUMNS, r[N_IN:])) for r in rows]
    families = {"lockstep", "full", "lanes", "head", "linear", "split"}
    assert {o["trace"] for o in out} == families == {o["shadow"] for o in out}
    assert {o["shade"] for o in out} == {"lean", "full", "routed"}
    for k in ("vol_hits", "sdf_hits", "vol_shadow", "sdf_shadow"):
        assert {o[k] for o in out} == {"none", "plain", "staged"}
    for k in ("early", "ldsl", "head_ldsl", "shade_miss"):
        assert {o[k] for o in out} == {0, 1}
    named = {g for o in out for g in (o["trace_grid0"], o["trace_grid1"], o["shadow_grid0"], o["shadow_grid1"])}
    assert named == set(ref.GRIDS) - {"shade"}
    for name, values in GRID:   # every value of the grid, so every switch in every position
        ix = [cols.index(c) for c in (name if isinstance(name, tuple) else (name,))]
        assert {tuple(r[i] for i in ix) for r in rows} >= {v if isinstance(v, tuple) else (v,) for v in values}, name
    by_inputs = {tuple(r[1:N_IN]): tuple(r[N_IN:]) for r in rows}
    for name, lo, hi in BOUNDARIES:
        c = ref.COLUMNS.index(name)
        pairs = [(k, k[:c] + (hi,) + k[c + 1:]) for k in by_inputs if k[c] == lo]
        assert any(b in by_inputs and by_inputs[a] != by_inputs[b] for a, b in pairs), name


def test_every_golden_row_reproduces(built, golden):
    rows = [r[1:N_IN] for r in golden["rows"]]
    want = [" ".join(map(str, r[N_IN:])) for r in golden["rows"]]
    assert [ref.choose(*r) for r in rows] == want
    got, _ = answers(built, rows)
    bad = [(r[0], w, g) for r, w, g in zip(golden["rows"], want, got) if w != g]
    assert len(got) == len(want) and not bad, "\n".join(f"{t}\n  golden {w!r}\n  now    {g!r}" for t, w, g in bad[:10])


def test_choice_sweep_from_first_principles(swept):
    total, distinct, trace, shadow, _ = swept
    assert total == GRID_ROWS
    assert sum(trace.values()) == total == sum(shadow.values())
    assert all(v > 0 for v in trace.values()) and all(v > 0 for v in shadow.values()) and len(trace) == len(shadow) == 6
    assert shadow["split"] < trace["split"] and shadow["head"] == trace["head"] and shadow["linear"] == trace["linear"]


def test_choice_check_sanitized(golden):
    """The sanitized program's answers (its sweep, the choices included, runs in
    test_pass_plan_host.py::test_plan_check_sanitized)."""
    subprocess.run(["make", "-s", "-C", NATIVE, "pass_plan_check_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    rows = [r[1:N_IN] for r in golden["rows"]]
    got, err = answers(EXE_ASAN, rows, env)
    assert got == [" ".join(map(str, r[N_IN:])) for r in golden["rows"]]
    assert "runtime error" not in err and "AddressSanitizer" not in err
