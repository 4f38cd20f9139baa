"""pt_shape_update and the two entry points of pt_update_shapes across the three bindings (no GPU): the struct
matches field for field between include/ptsharp_hip.h, ptsharp_amd/_abi.py and csharp/HipRenderer.cs (test_abi.py's
parsers, by import), its size is what the C declaration gives, and the argument errors that need no context are
reported with their message."""
import ctypes as C
import os

import test_abi
from ptsharp_amd import _abi

NAME = "pt_shape_update"


def test_python_binding_matches_header():
    test_abi.test_python_binding_matches_header(NAME)


def test_csharp_binding_matches_header():
    test_abi.test_csharp_binding_matches_header(NAME)


def test_struct_size_and_offsets():
    assert C.sizeof(_abi.pt_shape_update) == 16 + 6 * 8
    assert _abi.pt_shape_update.sphere_center.offset == 16 and _abi.pt_shape_update.xform_inverse.offset == 56
    fields = [f for f, _ in _abi.pt_shape_update._fields_]
    assert fields == ["num_spheres", "num_cubes", "num_transformed", "reserved", "sphere_center", "sphere_radius",
                      "cube_min", "cube_max", "xform_matrix", "xform_inverse"]


def test_entry_points_declared_everywhere():
    names = test_abi.declared_functions()
    assert "pt_update_shapes" in names and "pt_read_shape_bvh" in names
    assert "pt_update_shapes" in _abi.SIGNATURES and "pt_read_shape_bvh" in _abi.SIGNATURES
    cs = open(os.path.join(test_abi.ROOT, "csharp", "HipRenderer.cs")).read()
    assert "pt_update_shapes(IntPtr ctx, ref pt_shape_update u, out double kernelMs)" in cs
    assert "public double UpdateShapes(" in cs
    assert _abi.load_library().pt_get_version() == 10   # functions and one struct added: the version stays


def test_argument_errors_without_a_device():
    lib = _abi.load_library()
    ms = C.c_double(-1.0)
    three = (C.c_float * 3)(1, 2, 3)
    one = (C.c_double * 1)(1.0)
    sixteen = (C.c_double * 16)()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)

    def call(u):
        return lib.pt_update_shapes(None, None if u is None else C.byref(u), C.byref(ms)), lib.pt_last_error()

    rc, msg = call(None)
    assert rc == _abi.PT_ERR_INVALID_ARG and b"u is NULL" in msg
    rc, msg = call(_abi.pt_shape_update(0, 0, 0, 1))
    assert rc == _abi.PT_ERR_INVALID_ARG and b"reserved" in msg
    rc, msg = call(_abi.pt_shape_update(0, 1, 0, 0, cube_min=C.cast(three, fp)))
    assert rc == _abi.PT_ERR_INVALID_ARG and b"cube_min and cube_max" in msg
    rc, msg = call(_abi.pt_shape_update(0, 1, 0, 0, cube_max=C.cast(three, fp)))
    assert rc == _abi.PT_ERR_INVALID_ARG and b"cube_min and cube_max" in msg
    rc, msg = call(_abi.pt_shape_update(0, 0, 1, 0, xform_matrix=C.cast(sixteen, dp)))
    assert rc == _abi.PT_ERR_INVALID_ARG and b"xform_matrix and xform_inverse" in msg
    rc, msg = call(_abi.pt_shape_update(0, 0, 1, 0, xform_inverse=C.cast(sixteen, dp)))
    assert rc == _abi.PT_ERR_INVALID_ARG and b"xform_matrix and xform_inverse" in msg
    rc, msg = call(_abi.pt_shape_update(1, 0, 0, 0, sphere_radius=C.cast(one, dp)))
    assert rc == _abi.PT_ERR_INVALID_ARG and b"sphere_radius needs sphere_center" in msg
    rc, msg = call(_abi.pt_shape_update(1, 0, 0, 0, sphere_center=C.cast(three, fp)))   # well formed: the context is missing
    assert rc == _abi.PT_ERR_INVALID_ARG and b"ctx is NULL" in msg
    assert ms.value == -1.0   # no error path writes the time
    assert lib.pt_read_shape_bvh(None, None, None, None, None, None) == _abi.PT_ERR_INVALID_ARG
    assert b"ctx is NULL" in lib.pt_last_error()
