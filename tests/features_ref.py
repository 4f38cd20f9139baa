"""The expected first-hit features of a scene (pt_render_features), built pixel by pixel with the CPU
oracle's exported pieces: test infrastructure, like oracle_lib.

Per pixel (x, y) of a w x h frame:
  or_cast_ray(camera with aperture_radius 0, x, y, w, h, 0.5, 0.5, key 0)   the ray, no lens, no random number
  or_intersect                                                               t and the shape kind (or a miss)
  or_hit_info                                                                the shading normal after the flip, the material id
  or_hit_surface                                                             the Material.MaterialAt colour
  or_environment                                                             the albedo of a miss

  features(scene, camera, w, h, brute=False) -> (albedo [h,w,3] f64, normal [h,w,3] f32, depth [h,w] f64,
                                                 kind [h,w] i32, material [h,w] i32)
A miss has kind −1, depth 1e9 (Hit.INF), normal (0,0,0), material −1.  `brute` makes or_intersect test
every shape instead of walking the tree (the self-consistency check of the reference itself).

SCENES and SIZES are the cases of the GPU comparison (test_gpu_features.py) and of that self-consistency
check (test_features_host.py); expected(name, w, h) computes a case once.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import oracle_lib as O
from ptsharp_amd import _abi, scenes

HIT_INF = 1e9
# k_features' wave is an 8x8 pixel tile and its block 16x16: 67x45 is off every 8-, 16- and 64-pixel boundary
SIZES = [(67, 45), (9, 2)]
SCENES = {
    "gopher3": scenes.gopher3,
    "simplesphere": scenes.simplesphere,                    # a plane
    "textured": lambda: scenes.textured(mesh_tris=2000),    # colour, normal, bump and gloss textures
    "transformed": scenes.transformed,
    "sdf": scenes.sdf,
    "volume": scenes.volume,
    "mixed": lambda: scenes.mixed(3000, seed=5),            # environment texture, a Volume in a TransformedShape
}


def _lib():
    L = O.lib()
    vp, f3, i32p, dp = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    L.or_cast_ray.restype = None
    L.or_cast_ray.argtypes = [C.POINTER(_abi.pt_camera), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                              C.c_double, C.c_uint64, f3, f3]
    L.or_hit_info.restype = C.c_int32
    L.or_hit_info.argtypes = [vp, f3, f3, f3, f3, i32p, i32p]
    L.or_hit_surface.restype = C.c_int32
    L.or_hit_surface.argtypes = [vp, f3, f3, dp, dp]
    L.or_environment.restype = None
    L.or_environment.argtypes = [vp, f3, dp]
    return L


def features(scene, camera, w: int, h: int, brute: bool = False, oscene: O.OracleScene = None):
    L = _lib()
    os_ = oscene or O.OracleScene(scene)
    cam = camera.to_c()
    cam.aperture_radius = 0.0
    albedo = np.zeros((h, w, 3), np.float64)
    normal = np.zeros((h, w, 3), np.float32)
    depth = np.full((h, w), HIT_INF, np.float64)
    kind = np.full((h, w), -1, np.int32)
    material = np.full((h, w), -1, np.int32)
    o, d, pos, nrm = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)()
    k, idx, inside, mat = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    col, gloss = (C.c_double * 3)(), C.c_double()
    for y in range(h):
        for x in range(w):
            L.or_cast_ray(C.byref(cam), x, y, w, h, 0.5, 0.5, 0, o, d)
            t = L.or_intersect(os_.h, o, d, int(brute), C.byref(k), C.byref(idx))
            if t < HIT_INF:
                assert L.or_hit_info(os_.h, o, d, pos, nrm, C.byref(inside), C.byref(mat)) == 1
                assert L.or_hit_surface(os_.h, o, d, col, C.byref(gloss)) == 1
                depth[y, x], kind[y, x], material[y, x] = t, k.value, mat.value
                normal[y, x] = nrm[:]
                albedo[y, x] = col[:]
            else:
                L.or_environment(os_.h, d, col)
                albedo[y, x] = col[:]
    return albedo, normal, depth, kind, material


@functools.lru_cache(maxsize=None)
def scene_of(name):
    """(scene, camera, sampler) of SCENES[name], built once."""
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    return O.OracleScene(scene_of(name)[0])


@functools.lru_cache(maxsize=None)
def expected(name, w, h):
    """features() of SCENES[name] at w x h, computed once and read-only."""
    s, c, _ = scene_of(name)
    out = features(s, c, w, h, oscene=oracle_of(name))
    for a in out:
        a.setflags(write=False)
    return out
