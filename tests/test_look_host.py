"""The host side of pt_update_materials and pt_update_textures (no GPU): tests/native/look_check.cpp runs the light
and flag derivation that pt_upload_scene and pt_update_materials share (pt_scene_compile.h look_lights, look_flags) on
the tables of an original compile with an edited material table, and compares the lights, their side tables and the
flags byte for byte with a fresh compile of the edited scene, for the native fixture scenes (every shape kind, two
Volumes, instanced meshes, a routed scene) and a set of edits (recolour, dim, off, all off, each material switched on,
NaN and negative emittances, texture slots taken and given), and again after the shapes and a loose triangle moved.
It then runs pt_texture.h's decode in the kernel's lane order against lut[byte] for 2x2, 3x5, 67x33 and 256x2 in both
8-bit formats at every alignment of source and destination.  The same stand-alone program runs once more under
AddressSanitizer and UndefinedBehaviorSanitizer.

Every scene of ptsharp_amd/scenes.py (SCENES, as they are registered: the 1M-triangle frames included) goes through the
same comparison: this file flattens the scene, writes its pt_scene_desc into a temporary file and `look_check --scene`
reads it and runs the edits restated for any material table (recolour, dim, all off, each material toggled by itself,
all on, NaN and negative emittances, the texture slots taken away and one given).  The scenes of at most 100,000
triangles run under the sanitizers as well."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from ptsharp_amd import scenes

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
EXE = os.path.join(NATIVE, "_build", "look_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "look_check_asan")
SCENES = ("fixed-two-volumes", "fixed-one-volume", "big")
EDITS = ("none", "recolour", "dim", "light-off", "all-off", "white-on", "textured-on", "glass-on", "all-on",
         "nan-and-negative", "after-motion")
TEXTURE_EDITS = ("texture-off", "texture-on")   # the scenes with textures
DECODE = ("2x2", "3x5", "67x33", "256x2")


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "look.mk", "look_check"], check=True)
    return EXE


def test_look_check(built):
    r = subprocess.run([built], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "look_check: 0 failures"
    ok = [ln.split(":")[0] for ln in lines]
    for s in SCENES:
        for e in EDITS + (TEXTURE_EDITS if s != "big" else ()):
            assert f"case {s} {e} ok" in ok, r.stdout
    for d in DECODE:
        assert f"case decode {d} ok" in lines, r.stdout
    # the edits do what they are named for: the flags flip and the list grows and shrinks
    row = {ln.split(":")[0]: ln.split(":")[1].split() for ln in lines if ln.startswith("case fixed") or ln.startswith("case big")}
    assert row["case fixed-two-volumes none ok"][1] == "5" and row["case fixed-two-volumes all-off ok"][1] == "0"
    assert row["case fixed-two-volumes glass-on ok"][3] == "0"        # lights_lean 1 -> 0
    assert row["case fixed-two-volumes texture-off ok"][7] == "1"     # shade_route 0 -> 1
    assert row["case big none ok"][5] == "1" and row["case big glass-on ok"][5] == "0"   # route 1 -> 0


def test_look_check_sanitized():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "look.mk", "asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE_ASAN], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("look_check: 0 failures")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ------------------------------------------------------------------ every scene of scenes.py
def dump_scene(flat, path):
    """The FlatScene's pt_scene_desc as look_check.cpp's scene_file reads it: counts as int32 pairs, arrays raw, each
    padded to 8 bytes."""
    d = flat.desc
    out = []

    def ints(*v):
        out.append(struct.pack(f"<{len(v)}i", *v))

    def raw(a, count=None):
        b = a.tobytes() if isinstance(a, np.ndarray) else bytes(a)
        if count is not None:
            b = b[:count]
        out.append(b + b"\0" * (-len(b) % 8))

    from ptsharp_amd import _abi
    ints(0x4B4F4F4C, C.sizeof(_abi.pt_scene_desc))
    ints(d.num_materials, 0); raw(flat.materials, d.num_materials * C.sizeof(_abi.pt_material))
    ints(d.num_shapes, 0); raw(flat.shape_kind); raw(flat.shape_index)
    ints(d.num_spheres, 0); raw(flat.sphere_center); raw(flat.sphere_radius); raw(flat.sphere_material)
    ints(d.num_cubes, 0); raw(flat.cube_min); raw(flat.cube_max); raw(flat.cube_material)
    ints(d.num_planes, 0); raw(flat.plane_point); raw(flat.plane_normal); raw(flat.plane_material)
    ints(d.num_triangles, 0)
    for a in (flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3, flat.tri_material,
              flat.tri_t1, flat.tri_t2, flat.tri_t3):
        raw(a)
    ints(d.num_meshes, 0); raw(flat.mesh_first); raw(flat.mesh_count)
    out.append(struct.pack("<4d", *d.env_color, d.env_texture_angle))
    ints(d.env_texture, d.num_textures)
    for t in flat.texture_list:
        ints(t.Width, t.Height); raw(t.Data)
    nch = len(flat.sdf_children) if d.num_sdf_nodes else 0
    ints(d.num_sdf_nodes, nch); raw(flat.sdf_nodes, d.num_sdf_nodes * C.sizeof(_abi.pt_sdf_node)); raw(flat.sdf_children[:nch])
    ints(d.num_sdf_shapes, 0); raw(flat.sdf_shapes, d.num_sdf_shapes * C.sizeof(_abi.pt_sdf_shape))
    ints(d.num_volumes, 0)
    for i in range(d.num_volumes):
        v = flat.volumes[i]
        ints(v.w, v.h, v.d, v.num_windows)
        out.append(struct.pack("<d6f", v.zscale, *v.box_min, *v.box_max))
        raw(flat.volume_objects[i].Data)
        raw(flat._vol_keep[i][1], v.num_windows * C.sizeof(_abi.pt_volume_window))
    ints(d.num_transformed, 0); raw(flat.transformed, d.num_transformed * C.sizeof(_abi.pt_transformed_shape))
    with open(path, "wb") as f:
        f.write(b"".join(out))


@pytest.mark.parametrize("name", list(scenes.SCENES))
def test_every_scene_of_scenes_py(built, tmp_path, name):
    flat = scenes.SCENES[name]()[0].Compile()
    path = str(tmp_path / "scene.bin")
    dump_scene(flat, path)
    nm = len(flat.material_list)
    exes = [built]
    if flat.num_triangles <= 100_000:
        subprocess.run(["make", "-s", "-C", NATIVE, "-f", "look.mk", "asan"], check=True)
        exes.append(EXE_ASAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for exe in exes:
        r = subprocess.run([exe, "--scene", name, path], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == f"look_check {name}: 0 failures"
        ok = [ln.split(":")[0] for ln in lines]
        edits = ["none", "recolour", "dim", "all-off", "all-on", "nan-and-negative"] + [f"toggle-{i}" for i in range(nm)]
        edits += ["texture-off", "texture-on"] if flat.texture_list else []
        for e in edits:
            assert f"case {name} {e} ok" in ok, r.stdout[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        row = {ln.split(":")[0]: ln.split(":")[1].split() for ln in lines if ln.startswith("case ")}
        assert row[f"case {name} all-off ok"][1] == "0"   # the edits reach the derivation: no light left
