"""The arithmetic of pt_rebuild_blas and pt_blas_cost on the host (no GPU): tests/native/blas_rebuild_check.cpp drives
ptsharp_amd/csrc/pt_blas_rebuild.h with std::stable_sort, then the BLAS refit and the shape refit, as the kernels do,
against the scene compile: BLASes of every tested size at four poses (every triangle once, containment, the stack need,
child > parent, recs / shade / uv against a fresh compile, the fixed point, the fallback), the tail tables, the cost
gates and non-finite vertices.  The same stand-alone program runs once more under AddressSanitizer and
UndefinedBehaviorSanitizer.  tests/blas_rebuild_ref.py, the numpy restatement the GPU tests compare the device against,
is checked here word for word against the program's `--dump` of a rebuilt scene."""
import os
import subprocess

import numpy as np
import pytest

import blas_rebuild_ref as RB

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
EXE = os.path.join(NATIVE, "_build", "blas_rebuild_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "blas_rebuild_check_asan")
PAIRS = ((1, 288), (4, 5), (16, 17), (64, 65), (288, 65), (1025, 17), (4097, 5), (6400, 64))
SIZES = (1, 4, 5, 16, 17, 64, 65, 288, 1025, 4097, 6400)
POSES = ("rest", "sine", "twist", "offset")


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "blas_rebuild.mk", "blas_rebuild_check"], check=True)
    return EXE


def test_blas_rebuild_check(built):
    r = subprocess.run([built], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "blas_rebuild_check: 0 failures"
    assert {n for p in PAIRS for n in p} >= set(SIZES)
    for a, b in PAIRS:
        for pose in POSES:
            assert any(ln.startswith(f"pair {a} {b} {pose} ") and ln.endswith(": ok") for ln in lines), r.stdout
    assert "forced fallback ok" in lines and "nonfinite ok" in lines
    # the table DESIGN.md §4j quotes: no n in 1..400 falls back
    assert any(ln.startswith("fallback n:") and ln.endswith("(0 of 400)") for ln in lines), r.stdout
    # the cost gates ran on both poses, and the rebuilt tree is cheaper than the refitted one
    for pose in ("twist", "offset"):
        ln = next(l for l in lines if l.startswith(f"cost sphere {pose}:")).split()
        fresh, refit, rebuilt = float(ln[ln.index("fresh") + 1]), float(ln[ln.index("refit") + 1]), float(ln[ln.index("rebuilt") + 1])
        assert rebuilt < refit and fresh > 0, ln


def test_blas_rebuild_check_sanitized():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "blas_rebuild.mk", "asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE_ASAN], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("blas_rebuild_check: 0 failures")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_plan_of_every_size():
    for n in list(range(1, 401)) + [1024, 1025, 4096, 4097, 6400]:
        h, leaves, counts = RB.plan(n)
        assert 4 * 4 ** h >= n and (h == 1 or 4 * 4 ** (h - 1) < n)
        assert counts[0] == 1 and counts[-1] == (leaves + 3) // 4 and 3 * h <= 32
        refs = RB.node_refs(n)
        inner = refs[(refs != RB.EMPTY) & (refs < 0x80000000)]
        assert sorted(inner) == list(range(1, len(refs)))   # every node but the root is one slot's child
        leaf = refs[(refs != RB.EMPTY) & (refs >= 0x80000000)]
        assert sum(int((r >> 29) & 3) + 1 for r in leaf) == n and sorted(int(r & 0x1FFFFFFF) for r in leaf) == list(range(0, n, 4))
        for i, row in enumerate(refs):
            assert all(int(r) > i for r in row if r != RB.EMPTY and r < 0x80000000)


def test_blas_rebuild_ref_matches_native(built, tmp_path):
    r = subprocess.run([built, "--dump", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr

    def load(name, dtype, cols=None):
        a = np.fromfile(os.path.join(tmp_path, name), dtype)
        return a if cols is None else a.reshape(-1, cols)

    desc = load("desc.i32", np.int32, 4)
    nodes0, recs0, shade0 = load("nodes0.u32", np.uint32, 32), load("recs0.u32", np.uint32, 12), load("shade0.u32", np.uint32, 12)
    assert len(desc) == 2 and desc[1, 0] > 0 and desc[1, 2] > 0 and list(desc[:, 3]) == [288, 65]
    v = [load(f"v{k}.f32", np.float32, 3) for k in (1, 2, 3)]
    n = [load(f"n{k}.f32", np.float32, 3) for k in (1, 2, 3)]
    blas1, nodes, recs, shade, boxes, src = RB.rebuild(desc, nodes0, recs0, shade0, load("src_of_pos.i32", np.int32), *v, normals=n)
    desc1 = load("desc1.i32", np.int32, 4)
    assert np.array_equal(blas1[:, :3], desc1[:, :3]) and list(desc1[:, 1]) == [26, 8]
    assert np.array_equal(src, load("src_of_pos1.i32", np.int32))
    assert np.array_equal(nodes, load("nodes1.u32", np.uint32, 32))
    assert np.array_equal(recs, load("recs1.u32", np.uint32, 12))
    assert np.array_equal(shade, load("shade1.u32", np.uint32, 12))
    assert np.array_equal(boxes, load("boxes1.f32", np.float32, 6))
    assert not np.array_equal(nodes[:, 24:], nodes0[:, 24:]) and not np.array_equal(src, load("src_of_pos.i32", np.int32))
    want = load("cost1.f64", np.float64, 3)
    got = RB.cost(blas1, nodes)
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (got, want)
    # a BLAS whose capacity is too small keeps its topology and order
    b2, nodes2, _, _, _, src2 = RB.rebuild(desc, nodes0, recs0, shade0, load("src_of_pos.i32", np.int32), *v, normals=n, node_cap=[25, 16])
    assert list(b2[:, 1]) == [desc[0, 1], 8] and np.array_equal(nodes2[:desc[0, 1], 24:], nodes0[:desc[0, 1], 24:])
    assert np.array_equal(src2[:288], load("src_of_pos.i32", np.int32)[:288])
