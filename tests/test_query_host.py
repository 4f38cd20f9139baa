"""pt_intersect_hits' host side (no GPU).

tests/native/query_tables_check.cpp checks the identity tables the scene compile makes (the slot of every source
triangle, analytic record and plane; the position tables of the world BVH and the BLASes against pt_scene_desc; a
rebuild's permutation) from first principles; the same stand-alone program runs once more under AddressSanitizer and
UndefinedBehaviorSanitizer.  The reference the GPU tests compare with (tests/query_ref.py) is checked against itself:
the oracle's k-d walk and its loop over every shape agree on (t, kind, index) for the camera-ray cases, its slots are
those of the scene description, and the reported primitive's own intersect gives the reported t."""
import os
import subprocess

import numpy as np
import pytest

import features_ref as F
import query_ref as Q
from ptsharp_amd import _abi

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
EXE = os.path.join(NATIVE, "_build", "query_tables_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "query_tables_check_asan")


def test_query_tables_check():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "query.mk", "query_tables_check"], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "query_tables_check: 0 failures"
    assert any(l.startswith("case fixed ok") for l in lines) and any(l.startswith("case shared ok") for l in lines), r.stdout


def test_query_tables_check_sanitized():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "query.mk", "asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE_ASAN], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("query_tables_check: 0 failures")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@pytest.mark.parametrize("name", list(F.SCENES))
def test_the_walk_and_the_loop_agree_on_camera_rays(name):
    """The expected arrays take t, kind and index from the loop over every shape and Hit.Info from the k-d walk
    (or_hit_info walks): on these rays the two choose the same primitive, so the arrays describe one hit."""
    for w, h in F.SIZES:
        o, d, want = Q.camera_case(name, w, h)
        walk = Q.expected(F.oracle_of(name), o, d, brute=False, info=False)
        for what in ("t", "kind", "index", "shape", "prim"):
            a, b = want[what], walk[what]
            same = a.view(np.int64) == b.view(np.int64) if what == "t" else a == b
            assert same.all(), f"{name} {w}x{h}: walk and loop differ in {what} on rays {np.flatnonzero(~same)[:5]}"
        hit = want["kind"] >= 0
        print(f"{name} {w}x{h}: {int(hit.sum())} hits of {len(o)}, kinds {sorted(set(want['kind'][hit].tolist()))}")
        assert ((want["shape"] >= 0) == hit).all() and ((want["material"] >= 0) == hit).all()
        assert not Q.valid_index_failures(F.oracle_of(name).flat, want, o, d)


def test_slots_of_a_scene_description():
    """`shape` names the slot whose (shape_kind, shape_index) is the hit's, and a mesh triangle's its mesh's."""
    flat = F.oracle_of("mixed").flat
    tri_slot, by_kind = Q.slots(flat)
    kinds, idxs = np.asarray(flat.shape_kind), np.asarray(flat.shape_index)
    for k, table in by_kind.items():
        for j, slot in enumerate(table):
            if slot >= 0:
                assert kinds[slot] == k and idxs[slot] == j
                assert not ((kinds[:slot] == k) & (idxs[:slot] == j)).any()
    for t, slot in enumerate(tri_slot):
        assert slot >= 0
        if kinds[slot] == _abi.SHAPE_TRIANGLE:
            assert idxs[slot] == t
        else:
            m = idxs[slot]
            assert kinds[slot] == _abi.SHAPE_MESH and flat.mesh_first[m] <= t < flat.mesh_first[m] + flat.mesh_count[m]
