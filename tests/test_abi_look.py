"""pt_update_materials, pt_read_materials, pt_update_textures and pt_read_texture: exported with C linkage, declared in
the header and in the Python and C# bindings field for field, and their NULL and `reserved` refusals returned without
a device (the checks that need a context are in tests/test_gpu_look.py)."""
import ctypes as C
import re
import subprocess

import pytest

import test_abi as A
from ptsharp_amd import _abi

NAMES = ("pt_update_materials", "pt_read_materials", "pt_update_textures", "pt_read_texture")
STRUCTS = ("pt_material_update", "pt_look_info", "pt_texture_image", "pt_texture_update")


def test_symbols_exported():
    lib = _abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    for name in NAMES:
        assert name in A.declared_functions() and name in _abi.SIGNATURES and hasattr(lib, name)
        assert re.search(rf"\bT {name}\b", out), f"{name} not exported with C linkage"
        assert re.search(rf"static extern int {name}\(", cs), f"{name} has no DllImport"
    assert "public unsafe double UpdateMaterials(" in cs and "public double UpdateTextures(" in cs
    assert lib.pt_get_version() == 10 and _abi.ABI_VERSION == 10   # functions and structs were added: no new version


@pytest.mark.parametrize("name", STRUCTS)
def test_structs_match_header_in_both_bindings(name):
    A.test_python_binding_matches_header(name)
    A.test_csharp_binding_matches_header(name)


def test_struct_sizes():
    p = C.sizeof(C.c_void_p)
    assert C.sizeof(_abi.pt_material_update) == 16 + p + 24 + 8 + 8
    assert _abi.pt_material_update.materials.offset == 16 and _abi.pt_material_update.env_color.offset == 16 + p
    assert _abi.pt_material_update.env_texture.offset == 40 + p and _abi.pt_material_update.env_texture_angle.offset == 48 + p
    assert C.sizeof(_abi.pt_look_info) == 8 * 4 + 4 * 8
    assert C.sizeof(_abi.pt_texture_image) == 16 + 2 * p
    assert C.sizeof(_abi.pt_texture_update) == 16 + p
    assert (_abi.LOOK_ENV, _abi.TEXELS_F64, _abi.TEXELS_RGB8, _abi.TEXELS_RGBA8) == (1, 0, 1, 2)
    header = open(A.HEADER).read()
    assert re.search(r"#define PT_LOOK_ENV 1\b", header)
    assert re.search(r"PT_TEXELS_F64 = 0, PT_TEXELS_RGB8 = 1, PT_TEXELS_RGBA8 = 2", header)


def test_signatures_match_header():
    header = re.sub(r"/\*.*?\*/", "", open(A.HEADER).read(), flags=re.S)
    sig = lambda n: " ".join(re.search(rf"int {n}\((.*?)\);", header, re.S).group(1).split())
    assert sig("pt_update_materials") == "void* ctx, const pt_material_update* u, double* out_kernel_ms"
    assert sig("pt_read_materials") == ("void* ctx, pt_look_info* info, pt_material* materials, int32_t* light_rows, "
                                        "double* light_spheres")
    assert sig("pt_update_textures") == "void* ctx, const pt_texture_update* u, double* out_kernel_ms"
    assert sig("pt_read_texture") == "void* ctx, int32_t index, int32_t info[4], double* data"
    d, i = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert _abi.SIGNATURES["pt_update_materials"] == (C.c_int, [C.c_void_p, C.POINTER(_abi.pt_material_update), d])
    assert _abi.SIGNATURES["pt_read_materials"] == (C.c_int, [C.c_void_p, C.POINTER(_abi.pt_look_info),
                                                              C.POINTER(_abi.pt_material), i, d])
    assert _abi.SIGNATURES["pt_update_textures"] == (C.c_int, [C.c_void_p, C.POINTER(_abi.pt_texture_update), d])
    assert _abi.SIGNATURES["pt_read_texture"] == (C.c_int, [C.c_void_p, C.c_int32, i, d])
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    assert re.search(r"extern int pt_update_materials\(IntPtr ctx, ref pt_material_update u, out double kernelMs\);", cs)
    assert re.search(r"extern int pt_read_materials\(IntPtr ctx, out pt_look_info info, \[In, Out\] pt_material\[\] "
                     r"materials, int\[\] lightRows, double\[\] lightSpheres\);", cs)
    assert re.search(r"extern int pt_update_textures\(IntPtr ctx, ref pt_texture_update u, out double kernelMs\);", cs)
    assert re.search(r"extern int pt_read_texture\(IntPtr ctx, int index, int\[\] info, double\[\] data\);", cs)


def test_renderer_has_the_methods():
    from ptsharp_amd import Renderer
    for m in ("UpdateMaterials", "ReadMaterials", "UpdateTextures", "ReadTexture"):
        assert callable(getattr(Renderer, m))


def test_null_and_reserved_refusals_without_a_device():
    lib = _abi.load_library()
    ms = C.c_double(-7.0)
    fake = C.c_void_p(1)   # never dereferenced: these refusals come before the context is read
    mu, tu = _abi.pt_material_update(), _abi.pt_texture_update()
    for fn, u in ((lib.pt_update_materials, mu), (lib.pt_update_textures, tu)):
        assert fn(None, C.byref(u), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert b"NULL" in lib.pt_last_error()
        assert fn(fake, None, C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert b"NULL" in lib.pt_last_error()
    for k in range(2):
        mu = _abi.pt_material_update()
        mu.reserved[k] = 1
        assert lib.pt_update_materials(fake, C.byref(mu), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert b"reserved" in lib.pt_last_error()
    for flags in (2, 3, -1):
        mu = _abi.pt_material_update()
        mu.flags = flags
        assert lib.pt_update_materials(fake, C.byref(mu), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert b"flags" in lib.pt_last_error()
    for k in range(3):
        tu = _abi.pt_texture_update()
        tu.reserved[k] = 1
        assert lib.pt_update_textures(fake, C.byref(tu), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert b"reserved" in lib.pt_last_error()
    assert lib.pt_read_materials(None, None, None, None, None) == _abi.PT_ERR_INVALID_ARG
    assert lib.pt_read_texture(None, 0, None, None) == _abi.PT_ERR_INVALID_ARG
    assert ms.value == -7.0


def test_texture_table_reproduces_data():
    """ColorTexture keeps an 8-bit source and yields the table NewTexture, Pow and MulScalar compose into: Data is
    what it was, and equals Table()[byte] bit for bit."""
    import numpy as np
    from ptsharp_amd.scene import ColorTexture
    rng = np.random.default_rng(5)
    for shape in ((2, 2, 3), (5, 3, 4), (33, 67, 3), (2, 256, 4)):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        if shape[1] == 256:
            a[:, :, :3] = np.arange(256, dtype=np.uint8)[None, :, None]   # every byte value in every channel
        plain = ((a[:, :, :3].astype(np.float64) / 255) ** float(np.float32(2.2))) ** 1.3 * 0.5   # Data as it was before
        t = ColorTexture.NewTexture(a).Pow(1.3).MulScalar(0.5)
        assert t.Data.tobytes() == plain.reshape(-1, 3).tobytes()
        assert t.Source8 is not None and t.Source8.shape == shape
        assert t.Table()[a[:, :, :3]].reshape(-1, 3).tobytes() == t.Data.tobytes()
    assert ColorTexture(2, 2, np.zeros((4, 3))).Table() is None
