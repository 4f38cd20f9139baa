"""The keyed traversal-stack entries on the host (no GPU): tests/native/stack_key_check.cpp drives
ptsharp_amd/csrc/pt_stack_key.h, the one definition the kernels, the scene compile and tools/bvh_quality.cpp share.
For every key length the packed pop-time compare never culls an entry the exact test keeps, pack and unpack
round-trip at the largest index, the host's choice of the key length never overlaps the leaf bit or the index,
and a zero-length key leaves the bare ref."""
import os
import subprocess

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def test_stack_key_check():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "stack_key.mk", "stack_key_check"], check=True)
    r = subprocess.run([os.path.join(NATIVE, "_build", "stack_key_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "stack_key_check: 0 failures"
    for k in range(1, 16):
        assert any(l.startswith(f"K {k:2d} ok:") for l in lines), r.stdout


def test_scene_compile_picks_the_key_field():
    """compile_scene's DevScene::stack_key_mask on compiled scenes of 200, 4000 and 70,000 triangles, under the
    default and capped CompileOptions::pop_cull_bits: pt_stack_key.h's choice for the scene's counts, clear of
    the leaf flag and of every ref the triangle BVH's nodes hold."""
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "stack_key.mk", "scene"], check=True)
    r = subprocess.run([os.path.join(NATIVE, "_build", "stack_key_scene_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "stack_key_scene_check: 0 failures"
    assert sum(l.endswith(" ok") for l in lines) == 21, r.stdout
