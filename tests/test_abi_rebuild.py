"""pt_rebuild_meshes and pt_tri_bvh_cost at the ABI, without a GPU: the symbols exist in the header, the library, the
ctypes table and the C# drop-in, the ABI version is still 10, and the error paths that need no device answer
PT_ERR_INVALID_ARG with a message (a NULL out with a live context is tests/test_gpu_rebuild.py's)."""
import ctypes as C
import os
import re

from ptsharp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pt_rebuild_meshes", "pt_tri_bvh_cost")


def test_symbols_and_version():
    lib = _abi.load_library()
    header = open(os.path.join(ROOT, "include", "ptsharp_hip.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "HipRenderer.cs")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert re.search(rf"static extern int {name}\(", cs), name
    assert lib.pt_get_version() == _abi.ABI_VERSION == 10
    assert "#define PT_ABI_VERSION 10" in header
    from ptsharp_amd import Renderer
    assert callable(Renderer.RebuildMeshes) and callable(Renderer.TriBvhCost)


def test_null_arguments():
    lib = _abi.load_library()
    ms = C.c_double(-1.0)
    u = _abi.pt_mesh_update()
    assert lib.pt_rebuild_meshes(None, C.byref(u), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
    assert b"NULL" in lib.pt_last_error()
    assert lib.pt_rebuild_meshes(None, None, None) == _abi.PT_ERR_INVALID_ARG
    assert ms.value == -1.0
    out = (C.c_double * 3)(7.0, 7.0, 7.0)
    assert lib.pt_tri_bvh_cost(None, out) == _abi.PT_ERR_INVALID_ARG
    assert b"NULL" in lib.pt_last_error()
    assert lib.pt_tri_bvh_cost(None, None) == _abi.PT_ERR_INVALID_ARG
    assert list(out) == [7.0, 7.0, 7.0]
