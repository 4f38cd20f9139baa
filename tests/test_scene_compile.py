"""The host-only scene compile (ptsharp_amd/csrc/pt_scene_compile.cpp: what pt_upload_scene uploads), host build
(tests/native/scene_compile_check.cpp) on scenes built in C++ (tests/native/scene_fixture.h): the traversal lines'
layout, every triangle once in the BVH order and once in the leaf chunks, record kinds and indices with the first
occurrence named by the lights, one BLAS shared by two instances, the light list in Scene.Shapes order with its
phantoms, the heavy records, every routing flag against its defining expression, the three upload options, the
error cases with their codes and messages, and identical bytes from two compiles."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
EXE = os.path.join(NATIVE, "_build", "scene_compile_check")


def build():
    subprocess.run(["make", "-s", "-C", NATIVE, "scene_compile_check"], check=True)


def test_scene_compile_from_first_principles():
    build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("scene_compile_check: 0 failures")


def test_scene_compile_digest_lists_every_array_and_follows_the_options():
    build()

    def digest(*args):
        r = subprocess.run([EXE, "--digest", *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.splitlines()

    d = digest("big")
    assert [l.split()[0] for l in d[:24]] == [
        "lines", "tri_sh", "ana_recs", "planes", "mats", "lights", "tex_data", "texs", "sdf_prog", "sdf_params",
        "sdf_shapes", "vox", "windows", "vol_runs", "vol_cells", "volumes", "xforms", "ext_recs", "blas", "blas_nodes",
        "blas_recs", "blas_shade", "blas_uv", "heavy"]
    assert [l.split()[0] for l in d[24:]] == ["nodes", "counts", "flags", "env", "stats"]
    assert d == digest("big")   # the same bytes from another process
    flags = lambda lines: dict(zip(lines[26].split()[1::2], map(int, lines[26].split()[2::2])))  # noqa: E731
    assert flags(d)["route"] == 1 and flags(d)["vol_lds"] > 0
    r0, l0, c0 = digest("big", "route0"), digest("big", "lds0"), digest("big", "cells0")
    assert flags(r0)["route"] == 0 and [a for a, b in zip(d, r0) if a != b] == [d[26]]
    assert flags(l0)["vol_lds"] == 0 and [a for a, b in zip(d, l0) if a != b] == [d[26]]
    assert c0[14].split()[2] == "0" and d[14].split()[2] != "0"   # no cell-major corners
    assert [a.split()[0] for a, b in zip(d, c0) if a != b] == ["vol_cells", "volumes"]
