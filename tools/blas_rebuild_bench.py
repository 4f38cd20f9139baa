#!/usr/bin/env python3
"""pt_rebuild_blas against pt_update_meshes and pt_upload_scene on one GPU in one process: what re-sorting the BLAS of a
deformed instanced mesh costs, and what it buys.

The scene is tools/blas_refit_bench.py's: the C3 mesh (scenes.blob_mesh(69,451)) instanced 64 times over a floor under
a sphere light, at 1920x1080, one BLAS and no world triangle BVH.  The poses move the mesh's own vertices in object
space: `sine` is that tool's (z += 0.3 sin(5x) cos(3y)), `twist` turns every vertex about the y axis by 2 y radians.
Each figure is the median of `--reps` calls after `--warmup` untimed ones, with min and max:

  rebuild        pt_rebuild_blas(PT_REBUILD_BLAS) of the posed vertices, the normals kept: the wall time of the call and
                 its out_kernel_ms; `rebuild_no_tail` the same with PT_BLAS_TAIL=0 (every round a device sort).  The
                 sorts are oblivious to the order they start from, so repeating the call at one pose times the same work;
  update         pt_update_meshes of the same arrays, in the same run;
  upload         pt_upload_scene of the deformed scene, every timed upload a geometry the process has not seen;
  props          64 distinct 2,000-triangle meshes (blob_mesh(2000, seed i)), one instance each: the rebuild with the
                 default tail and with PT_BLAS_TAIL=0;
  steps          one 16-spp step at each pose for three trees (refitted, rebuilt, fresh upload): rays (pt_stats) per
                 second of device time, with pt_blas_cost beside each.

`--upload-only --lib PATH` measures only `upload`, through another build of the library (one without pt_rebuild_blas).
One JSON document goes to --out.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from blas_refit_bench import H, SIDE, SPP, W, check, field, load, sine_pose, step, summary  # noqa: E402
from ptsharp_amd import TransformedShape, Vector, _abi, scenes  # noqa: E402
from ptsharp_amd.geometry import Colour, Matrix, Util  # noqa: E402
from ptsharp_amd.scene import Camera, Cube, DefaultSampler, Material, Scene, SpecularMode, Sphere  # noqa: E402

f32 = np.float32


def twist_pose(v, rate=2.0):
    out = v.copy()
    ang = (f32(rate) * v[:, 1]).astype(f32)
    c, s = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
    out[:, 0] = (c * v[:, 0] - s * v[:, 2]).astype(f32)
    out[:, 2] = (s * v[:, 0] + c * v[:, 2]).astype(f32)
    return np.ascontiguousarray(out, f32)


POSES = {"sine": sine_pose, "twist": twist_pose}


def props(count=64, tris=2000):
    scene = Scene()
    rng = np.random.default_rng(7)
    side = int(np.ceil(np.sqrt(count)))
    for i in range(count):
        mesh = scenes.blob_mesh(tris, seed=100 + i, amplitude=0.15)
        mesh.SetMaterial(Material.GlossyMaterial(Colour.HexColor(0xF2EBC7), 1.5, Util.Radians(0)))
        at = Vector(2.5 * (i % side - (side - 1) / 2), 1, 2.5 * (i // side - (side - 1) / 2))
        scene.Add(TransformedShape.NewTransformedShape(mesh, Matrix.TranslateM(at).Mul(Matrix.RotateM(Vector(0, 1, 0), rng.uniform(0, 6.28)))))
    scene.Add(Cube.NewCube(Vector(-10000, -10000, -10000), Vector(10000, 0, 10000),
                           Material.GlossyMaterial(Colour.HexColor(0x33332D), 1.2, Util.Radians(20))))
    scene.Add(Sphere.NewSphere(Vector(0, 14, 0), 3, Material.LightMaterial(Colour.White, 10)))
    camera = Camera.LookAt(Vector(-6, 9, 16), Vector(0, 0.75, 0), Vector(0, 1, 0), 50)
    sampler = DefaultSampler.NewSampler(4, 4)
    sampler.SetSpecularMode(SpecularMode.SpecularModeFirst)
    return scene, camera, sampler


def mesh_update(moved):
    fp = C.POINTER(C.c_float)
    return _abi.pt_mesh_update(len(moved[0]), 0, (C.c_int32 * 2)(0, 0), *[v.ctypes.data_as(fp) for v in moved])


def timed(lib, call, reps, warmup, tail=None):
    """Wall and kernel time of call(ms_ref); PT_BLAS_TAIL set to `tail` around the calls."""
    old = os.environ.pop("PT_BLAS_TAIL", None)
    if tail is not None:
        os.environ["PT_BLAS_TAIL"] = tail
    try:
        wall, kernel = [], []
        for i in range(warmup + reps):
            ms = C.c_double(0.0)
            t0 = time.perf_counter()
            call(ms)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= warmup:
                wall.append(dt)
                kernel.append(ms.value)
    finally:
        os.environ.pop("PT_BLAS_TAIL", None)
        if old is not None:
            os.environ["PT_BLAS_TAIL"] = old
    return {"wall_ms": summary(wall), "kernel_ms": summary(kernel)}


def blas_cost(lib, ctx):
    counts = (C.c_int64 * 3)()
    check(lib, lib.pt_read_blas(ctx, counts, None, None, None, None, None), "pt_read_blas")
    out = np.zeros((int(counts[0]), 3), np.float64)
    check(lib, lib.pt_blas_cost(ctx, int(counts[0]), out.ctypes.data_as(C.POINTER(C.c_double))), "pt_blas_cost")
    return {"inner": round(float(out[0, 0]), 4), "leaf": round(float(out[0, 1]), 4), "root_area": round(float(out[0, 2]), 4),
            "nodes": int(counts[1])}


def timed_uploads(lib, ctx, flat, rest, reps, warmup):
    wall = []
    for i in range(warmup + reps):
        for dst, src in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3), rest):
            dst[...] = sine_pose(src, 0.3 + 1e-5 * (i + 1))   # a geometry of its own
        t0 = time.perf_counter()
        check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            wall.append(dt)
    return {"wall_ms": summary(wall)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--tris", type=int, default=69_451)
    ap.add_argument("--lib", default=_abi.LIB_PATH)
    ap.add_argument("--upload-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blas_rebuild_bench.json"))
    a = ap.parse_args()
    lib = load(a.lib)
    scene, camera, sampler = field(a.tris)
    flat = scene.Compile()
    rest = [flat.tri_v1.copy(), flat.tri_v2.copy(), flat.tri_v3.copy()]
    n = len(flat.tri_material)
    doc = {"tool": "tools/blas_rebuild_bench.py", "scene": f"blob_mesh({a.tris}) instanced {SIDE * SIDE} times, floor, sphere light",
           "triangles": n, "instances": SIDE * SIDE, "poses": {"sine": "z += 0.3 sin(5x) cos(3y)", "twist": "about y by 2 y rad"},
           "reps": a.reps, "warmup": a.warmup, "step": f"{W}x{H} at {SPP} spp",
           "library": os.path.relpath(a.lib, ROOT) if a.lib.startswith(ROOT) else os.path.basename(a.lib)}
    ctx = C.c_void_p()
    opts = _abi.pt_device_opts(0, W, H)
    check(lib, lib.pt_create(C.byref(opts), C.byref(ctx)), "pt_create")
    try:
        if a.upload_only:
            doc["upload"] = timed_uploads(lib, ctx, flat, rest, a.reps, a.warmup)
        else:
            upload = lambda: check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")
            rebuild = lambda u: lambda ms: check(lib, lib.pt_rebuild_blas(ctx, C.byref(u), _abi.REBUILD_BLAS, C.byref(ms)), "pt_rebuild_blas")
            update = lambda u: lambda ms: check(lib, lib.pt_update_meshes(ctx, C.byref(u), C.byref(ms)), "pt_update_meshes")
            upload()   # the rest pose
            doc["cost_rest"] = blas_cost(lib, ctx)
            moved = [twist_pose(v) for v in rest]
            u = mesh_update(moved)
            doc["update"] = timed(lib, update(u), a.reps, a.warmup)
            doc["rebuild"] = timed(lib, rebuild(u), a.reps, a.warmup)
            upload()
            doc["rebuild_no_tail"] = timed(lib, rebuild(u), a.reps, a.warmup, tail="0")
            doc["steps"] = {}
            for pname, fn in POSES.items():
                moved = [fn(v) for v in rest]
                u = mesh_update(moved)
                for dst, src in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3), rest):
                    dst[...] = src
                upload()   # the rest pose's tree
                update(u)(C.c_double())
                row = {"refitted": dict(step(lib, ctx, camera, sampler, a.step_reps, 1), cost=blas_cost(lib, ctx))}
                rebuild(u)(C.c_double())
                row["rebuilt"] = dict(step(lib, ctx, camera, sampler, a.step_reps, 1), cost=blas_cost(lib, ctx))
                for dst, src in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3), moved):
                    dst[...] = src
                upload()
                row["fresh_upload"] = dict(step(lib, ctx, camera, sampler, a.step_reps, 1), cost=blas_cost(lib, ctx))
                for k in ("refitted", "rebuilt"):
                    row[k + "_over_fresh_rays_per_s"] = round(row[k]["rays_per_s"] / row["fresh_upload"]["rays_per_s"], 4)
                doc["steps"][pname] = row
            doc["upload"] = timed_uploads(lib, ctx, flat, rest, a.reps, a.warmup)
            # the props: every BLAS fits one tail workgroup or two
            pscene, _, _ = props()
            pflat = pscene.Compile()
            check(lib, lib.pt_upload_scene(ctx, C.byref(pflat.desc)), "pt_upload_scene")
            pmoved = [twist_pose(v) for v in (pflat.tri_v1, pflat.tri_v2, pflat.tri_v3)]   # (the struct holds bare pointers)
            pu = mesh_update(pmoved)
            doc["props"] = {"scene": "64 distinct blob_mesh(2000) props, one instance each", "triangles": len(pflat.tri_material),
                            "update": timed(lib, update(pu), a.reps, a.warmup),
                            "rebuild": timed(lib, rebuild(pu), a.reps, a.warmup)}
            check(lib, lib.pt_upload_scene(ctx, C.byref(pflat.desc)), "pt_upload_scene")
            doc["props"]["rebuild_no_tail"] = timed(lib, rebuild(pu), a.reps, a.warmup, tail="0")
    finally:
        lib.pt_destroy(ctx)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
