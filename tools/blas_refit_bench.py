#!/usr/bin/env python3
"""pt_update_meshes against pt_upload_scene on one GPU in one process: what deforming an instanced mesh costs.

The scene is the C3 mesh (scenes.blob_mesh(69,451), smooth normals, fitted as bunny_frame fits it) instanced 64 times
(an 8 x 8 field, each instance under its own rotation, non-uniform scale and translation) over a floor cube under a
sphere light, at 1920x1080.  The mesh is in no other shape: the scene has one BLAS and no world triangle BVH.  The pose
is DESIGN.md §4c's sine displacement of the mesh's own vertices (z += 0.3 sin(5x) cos(3y), object space).  Each figure is
the median of `--reps` calls after `--warmup` untimed ones, with min and max:

  update     pt_update_meshes of the posed vertices, the normals kept: the wall time of the call (the three arrays
             copied in, the kernels, the mesh box back, the lights) and its out_kernel_ms (device time between two
             hipEvents around every kernel: the BLAS triangles, bounds and levels, then the shape refit);
  upload     the wall time of pt_upload_scene of the same deformed scene (the host compile with the BLAS build, every
             array copied in).  Every timed upload is a geometry the process has not seen (the amplitude differs in
             its last digits), as the frames of an animation are;
  rays       one 16-spp step at the refitted pose against the same step after a fresh upload of that pose: rays
             (pt_stats) per second of device time.  The refit keeps the topology the build chose for the rest pose;
             this is what that costs.

`--upload-only --lib PATH` measures only `upload`, through another build of the library (one without pt_update_meshes,
where an upload is the only way to move such a mesh).  One JSON document goes to --out.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ptsharp_amd import TransformedShape, Vector, _abi, scenes  # noqa: E402
from ptsharp_amd.geometry import Box, Colour, Matrix, Util  # noqa: E402
from ptsharp_amd.scene import Camera, Cube, DefaultSampler, Material, Scene, SpecularMode, Sphere  # noqa: E402

W, H, SPP = 1920, 1080, 16
SIDE = 8   # SIDE^2 instances


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def sine_pose(v, amplitude=0.3):
    f = np.float32
    out = v.copy()
    out[:, 2] = v[:, 2] + (f(amplitude) * np.sin(f(5) * v[:, 0]) * np.cos(f(3) * v[:, 1])).astype(f)
    return np.ascontiguousarray(out, f)


def field(tris):
    mesh = scenes.blob_mesh(tris)
    mesh.SetMaterial(Material.GlossyMaterial(Colour.HexColor(0xF2EBC7), 1.5, Util.Radians(0)))
    mesh.SmoothNormals()
    mesh.FitInside(Box(Vector(-1, 0, -1), Vector(1, 2, 1)), Vector(0.5, 0, 0.5))
    scene = Scene()
    rng = np.random.default_rng(64)
    for i in range(SIDE * SIDE):
        at = Vector(2.5 * (i % SIDE - (SIDE - 1) / 2), 0, 2.5 * (i // SIDE - (SIDE - 1) / 2))
        m = Matrix.TranslateM(at).Mul(Matrix.RotateM(Vector(0, 1, 0), rng.uniform(0, 6.28))).Mul(
            Matrix.ScaleM(Vector(*rng.uniform(0.6, 1.1, size=3))))
        scene.Add(TransformedShape.NewTransformedShape(mesh, m))
    scene.Add(Cube.NewCube(Vector(-10000, -10000, -10000), Vector(10000, 0, 10000),
                           Material.GlossyMaterial(Colour.HexColor(0x33332D), 1.2, Util.Radians(20))))
    scene.Add(Sphere.NewSphere(Vector(0, 14, 0), 3, Material.LightMaterial(Colour.White, 10)))
    camera = Camera.LookAt(Vector(-6, 9, 16), Vector(0, 0.75, 0), Vector(0, 1, 0), 50)
    sampler = DefaultSampler.NewSampler(4, 4)
    sampler.SetSpecularMode(SpecularMode.SpecularModeFirst)
    return scene, camera, sampler


def load(path):
    """The library at `path` with the prototypes of the entry points it has."""
    lib = C.CDLL(path)
    for name, (res, args) in _abi.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def check(lib, code, where):
    if code != _abi.PT_OK:
        raise RuntimeError(f"{where}: {code} {lib.pt_last_error().decode()}")


def set_pose(flat, rest, amplitude):
    for dst, src in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3), rest):
        dst[...] = sine_pose(src, amplitude)


def timed_uploads(lib, ctx, flat, rest, reps, warmup):
    wall = []
    for i in range(warmup + reps):
        set_pose(flat, rest, 0.3 + 1e-5 * (i + 1))   # a geometry of its own
        t0 = time.perf_counter()
        check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            wall.append(dt)
    return {"wall_ms": summary(wall)}


def step(lib, ctx, camera, sampler, reps, warmup):
    cam, smp = camera.to_c(), sampler.to_c()
    ms, rays = [], []
    for i in range(warmup + reps):
        pp = _abi.pt_pass_params(SPP, 0, 1234, i + 1, 0, C.POINTER(C.c_int32)(), _abi.ENGINE_AUTO, 0, 0, 0, 1)
        check(lib, lib.pt_render_pass(ctx, C.byref(cam), C.byref(smp), C.byref(pp)), "pt_render_pass")
        s = _abi.pt_stats()
        check(lib, lib.pt_stats_get(ctx, C.byref(s)), "pt_stats_get")
        if i >= warmup:
            ms.append(s.last_pass_ms)
            rays.append(int(s.rays))
    check(lib, lib.pt_reset_buffer(ctx), "pt_reset_buffer")
    m = statistics.median(ms)
    return {"step_ms": summary(ms), "rays_per_step": int(statistics.median(rays)),
            "rays_per_s": round(statistics.median(rays) / (m * 1e-3), 0)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--tris", type=int, default=69_451)
    ap.add_argument("--lib", default=_abi.LIB_PATH)
    ap.add_argument("--upload-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blas_refit_bench.json"))
    a = ap.parse_args()
    lib = load(a.lib)
    scene, camera, sampler = field(a.tris)
    flat = scene.Compile()
    rest = [flat.tri_v1.copy(), flat.tri_v2.copy(), flat.tri_v3.copy()]
    n = len(flat.tri_material)
    doc = {"tool": "tools/blas_refit_bench.py", "scene": f"blob_mesh({a.tris}) instanced {SIDE * SIDE} times, floor, sphere light",
           "triangles": n, "instances": SIDE * SIDE, "pose": "z += 0.3 sin(5x) cos(3y), object space", "reps": a.reps,
           "warmup": a.warmup, "step": f"{W}x{H} at {SPP} spp",
           "library": os.path.relpath(a.lib, ROOT) if a.lib.startswith(ROOT) else os.path.basename(a.lib)}
    ctx = C.c_void_p()
    opts = _abi.pt_device_opts(0, W, H)
    check(lib, lib.pt_create(C.byref(opts), C.byref(ctx)), "pt_create")
    try:
        if not a.upload_only:
            check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")   # the rest pose
            moved = [sine_pose(v) for v in rest]
            fp = C.POINTER(C.c_float)
            u = _abi.pt_mesh_update(n, 0, (C.c_int32 * 2)(0, 0), *[v.ctypes.data_as(fp) for v in moved])
            wall, kernel = [], []
            for i in range(a.warmup + a.reps):
                ms = C.c_double(0.0)
                t0 = time.perf_counter()
                check(lib, lib.pt_update_meshes(ctx, C.byref(u), C.byref(ms)), "pt_update_meshes")
                dt = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    wall.append(dt)
                    kernel.append(ms.value)
            counts = (C.c_int64 * 3)()
            check(lib, lib.pt_read_blas(ctx, counts, None, None, None, None, None), "pt_read_blas")
            doc["update"] = {"wall_ms": summary(wall), "kernel_ms": summary(kernel), "blases": int(counts[0]),
                             "blas_nodes": int(counts[1]), "blas_triangles": int(counts[2]), "input_bytes": 36 * n,
                             "written_bytes_min": 48 * int(counts[2]) + 96 * int(counts[1])}
            doc["rays_refitted"] = step(lib, ctx, camera, sampler, a.step_reps, 1)
        doc["upload"] = timed_uploads(lib, ctx, flat, rest, a.reps, a.warmup)
        if not a.upload_only:
            set_pose(flat, rest, 0.3)
            check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")
            doc["rays_fresh_upload"] = step(lib, ctx, camera, sampler, a.step_reps, 1)
            doc["upload_over_update_wall"] = round(doc["upload"]["wall_ms"]["median"] / doc["update"]["wall_ms"]["median"], 1)
            doc["refitted_over_fresh_rays_per_s"] = round(doc["rays_refitted"]["rays_per_s"] / doc["rays_fresh_upload"]["rays_per_s"], 4)
    finally:
        lib.pt_destroy(ctx)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
