"""The normals pt_update_triangles_normals derives, restated from its description in include/ptsharp_hip.h and
DESIGN.md §4c with what the package already has on the host:

  face     Triangle.FixNormals on zeroed normals (scene.fix_normals_arrays): the face normal at every corner;
  smooth   the face normals, then Mesh.SmoothNormals (pt_mesh_smooth_normals, host only) on each mesh's
           mesh_first / mesh_count range by itself; triangles outside every range keep the face normal.

`normals(v1, v2, v3, mesh_first, mesh_count, mode)` returns n1, n2, n3, [n, 3] float32.  Checked on the CPU against
tests/native/normals_check.cpp's dump (tests/test_normals_host.py); the GPU tests compare the device against it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ptsharp_amd import _abi
from ptsharp_amd.scene import fix_normals_arrays

F32 = np.float32


def face(v1, v2, v3):
    v1, v2, v3 = (np.ascontiguousarray(a, F32).reshape(-1, 3) for a in (v1, v2, v3))
    z = np.zeros_like(v1)
    with np.errstate(all="ignore"):
        return [np.ascontiguousarray(n, F32) for n in fix_normals_arrays(v1, v2, v3, z, z, z)]


def smooth_range(v1, v2, v3, n1, n2, n3):
    """Mesh.SmoothNormals on one mesh: new n1, n2, n3."""
    arrs = [np.ascontiguousarray(a, F32).copy() for a in (v1, v2, v3, n1, n2, n3)]
    if len(arrs[0]):
        lib = _abi.load_library()
        rc = lib.pt_mesh_smooth_normals(len(arrs[0]), *[a.ctypes.data_as(C.POINTER(C.c_float)) for a in arrs])
        assert rc == 0, lib.pt_obj_last_error()
    return arrs[3:]


def normals(v1, v2, v3, mesh_first, mesh_count, mode):
    n = face(v1, v2, v3)
    if mode == "face":
        return n
    assert mode == "smooth"
    v = [np.ascontiguousarray(a, F32).reshape(-1, 3) for a in (v1, v2, v3)]
    for f, c in zip(mesh_first, mesh_count):
        r = slice(int(f), int(f) + int(c))
        for dst, src in zip(n, smooth_range(*[a[r] for a in v], *[a[r] for a in n])):
            dst[r] = src
    return n


def same_bits(got, want, what=""):
    """Equal bit for bit; where the reference is a NaN, a NaN (payloads are not compared)."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    nan = np.isnan(want)
    bad = np.argwhere((np.isnan(got) != nan) | (~nan & (got.view(np.uint32) != want.view(np.uint32))))
    assert not bad.size, (f"{what}: {len(bad)} of {got.size} components differ, first at {bad[0]}: "
                          f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")
