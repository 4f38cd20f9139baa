"""The arithmetic of pt_rebuild_meshes on the host (no GPU): tests/native/rebuild_check.cpp drives
ptsharp_amd/csrc/pt_rebuild.h (the order by std::stable_sort, the topology) and pt_refit.h leaves-then-levels, as the
kernels do, against the scene compile: structure, containment, records, the light, the fixed point and the cost gates
(DESIGN.md §4g).  The same stand-alone program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer.
tests/rebuild_ref.py, the numpy restatement the GPU tests compare the device against, is checked here word for word
against the program's `--dump`."""
import os
import re
import subprocess

import numpy as np
import pytest

import rebuild_ref

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
EXE = os.path.join(NATIVE, "_build", "rebuild_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "rebuild_check_asan")
SIZES = (1, 2, 3, 4, 24, 25, 192, 193, 1537, 6400)
POSES = ("rest", "sine", "twist", "offset")


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "rebuild.mk", "rebuild_check"], check=True)
    return EXE


def test_rebuild_check(built):
    r = subprocess.run([built], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("rebuild_check: 0 failures")
    lines = [line.split() for line in out.splitlines()]
    for p in SIZES:
        for pose in POSES:
            assert ["P", str(p), "pose", pose, "ok"] in lines, out
    # the refit and pose workspaces' layouts: every P from 1 to 6400, SIZES among them
    assert "layouts 6400 of P 1..6400 ok".split() in lines, out
    # the cost gates on the 6,400-triangle sphere: the program asserts them; the figures are printed
    cost = {m.group(1): (float(m.group(2)), float(m.group(3)))
            for m in re.finditer(r"cost (\w+) +refit ([\d.]+) rebuilt ([\d.]+)", out)}
    print(cost)
    assert cost["offset"][1] <= cost["offset"][0] / 3
    assert cost["twist"][1] <= 0.8 * cost["twist"][0]


def test_rebuild_check_sanitized():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "rebuild.mk", "asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE_ASAN], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("rebuild_check: 0 failures")
    # this build samples the layout sweep (every P up to 400, every 61st after that, 1537 and 6400): all 6400
    # compiles take minutes under the sanitizers; test_rebuild_check sweeps every P
    assert "layouts 500 of P 1..6400 ok" in r.stdout, r.stdout[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_plan_and_topology():
    assert rebuild_ref.plan(0) == (0, 0, [])
    assert rebuild_ref.plan(3) == (1, 1, [1])
    assert rebuild_ref.plan(24) == (1, 8, [1])
    assert rebuild_ref.plan(25) == (2, 9, [1, 2])
    assert rebuild_ref.plan(193) == (3, 65, [1, 2, 9])
    assert rebuild_ref.plan(6400) == (4, 2134, [1, 5, 34, 267])
    nodes, chunks = rebuild_ref.topology(25)
    assert nodes[0, 3] == 0x22000000 and nodes[0, 4] == 1 and nodes[0, 5] == 0x80000000
    assert nodes[1, 3] == 0x80000000 and nodes[1, 5] == 0x80000000 and nodes[1, 6] == 0xAAAA
    assert nodes[2, 3] == 0x10000000 and nodes[2, 5] == 0x80000008 and nodes[2, 6] == 0
    assert chunks[8, 0] == 24 and chunks[7, 0] == (21 | (2 << 29))


@pytest.mark.parametrize("p,pose", [(1, "rest"), (4, "twist"), (25, "offset"), (193, "sine"), (1537, "twist"), (6400, "offset")])
def test_rebuild_ref_matches_native(built, tmp_path, p, pose):
    r = subprocess.run([built, "--dump", str(tmp_path), str(p), pose], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr

    def load(name, dtype, cols):
        return np.fromfile(os.path.join(tmp_path, name), dtype).reshape(-1, cols)

    recs0 = load("recs0.u32", np.uint32, 32)
    src0 = np.fromfile(os.path.join(tmp_path, "src0.i32"), np.int32)
    arrays = [load(f"{n}.f32", np.float32, 3) for n in ("v1", "v2", "v3", "n1", "n2", "n3")]
    assert len(src0) == p == len(recs0)
    (nodes, chunks, recs, box), src = rebuild_ref.rebuild(recs0, src0, *arrays)
    assert np.array_equal(src, np.fromfile(os.path.join(tmp_path, "src1.i32"), np.int32))
    assert np.array_equal(nodes, load("nodes1.u32", np.uint32, 32))
    assert np.array_equal(chunks, load("chunks1.u32", np.uint32, 32))
    assert np.array_equal(recs, load("recs1.u32", np.uint32, 32))
    assert np.array_equal(box.view(np.uint32), np.fromfile(os.path.join(tmp_path, "box1.f32"), np.uint32))
    want = np.fromfile(os.path.join(tmp_path, "cost1.f64"), np.float64)
    got = np.array(rebuild_ref.cost(nodes))
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), (got, want)
    if p > 24:
        assert not np.array_equal(src, src0)
