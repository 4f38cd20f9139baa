#!/usr/bin/env python3
"""pt_update_shapes against pt_upload_scene on one GPU in one process: what moving spheres costs.

The scene is the frame of the reference's beads loop (Example.cs:163-223): 80 strands of 399 spheres of radius 0.1
(31,920) under one sphere light, each strand a walk of 0.1 steps along low-pass-filtered noise (LowPassNoise restated
in numpy under a fixed seed: the reference draws from an unseedable generator), sphere i of a strand at
positions[i] + (positions[i + 1] - positions[i]) t.  The scene is uploaded at t = 0 and moved to t = 0.5; each figure
is the median of `--reps` calls after `--warmup` untimed ones, with min and max:

  update     pt_update_shapes of the t = 0.5 centres: the wall time of the call (the parameters copied in, the
             kernels, the lights) and its out_kernel_ms (device time between two hipEvents around the kernels);
  upload     the wall time of pt_upload_scene of the moved scene (the host compile with its analytic BVH build,
             every array copied in);
  rays       one 1920x1080 step at the refitted pose against the same step after a fresh upload of that pose: rays
             (pt_stats) per second of device time.  The refit keeps the topology the build chose for t = 0; this is
             what that costs.

`--upload-only --lib PATH` measures only `upload`, through another build of the library (one without
pt_update_shapes, to record what the only path cost there).  One JSON document goes to --out.
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
from ptsharp_amd import _abi  # noqa: E402
from ptsharp_amd.geometry import Colour, Util, Vector  # noqa: E402
from ptsharp_amd.scene import Camera, DefaultSampler, Material, Scene, SpecularMode, Sphere  # noqa: E402

W, H = 1920, 1080
STRANDS, N = 80, 400


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def low_pass_noise(rng, n, alpha, iterations):
    """Example.cs LowPassNoise: uniform noise in [-1, 1), `iterations` one-pole low-pass filters, normalised to [-1, 1]."""
    v = rng.random(n) * 2 - 1
    for _ in range(iterations):
        out, y = np.empty(n), 0.0
        for i in range(n):
            y -= alpha * (y - v[i])
            out[i] = y
        v = out
    return -1 + (v - v.min()) / (v.max() - v.min()) * 2


def strands(seed):
    """positions [STRANDS, N, 3] float32 (each strand's walk from the origin) and a material index per strand."""
    rng = np.random.default_rng(seed)
    f = np.float32
    pos = np.zeros((STRANDS, N, 3), f)
    mats = rng.integers(0, 3, STRANDS)
    for a in range(STRANDS):
        xyz = np.stack([low_pass_noise(rng, N, 0.25, 4) for _ in range(3)], axis=1)
        v = (xyz.astype(f) / np.linalg.norm(xyz, axis=1, keepdims=True).astype(f)).astype(f)
        step = (v * f(0.1)).astype(f)
        p = np.zeros(3, f)
        for i in range(N):
            pos[a, i] = p
            p = (p + step[i]).astype(f)
    return pos, mats


def centres(pos, t):
    a, b = pos[:, :-1], pos[:, 1:]
    return np.ascontiguousarray((a + ((b - a).astype(np.float32) * np.float32(t)).astype(np.float32)).reshape(-1, 3), np.float32)


def beads(seed=1234):
    pos, mats = strands(seed)
    rng = np.random.default_rng(seed + 1)
    materials = [Material.GlossyMaterial(Colour(*rng.random(3)), 1.3, Util.Radians(20)) for _ in range(3)]
    scene = Scene()
    c0 = centres(pos, 0.0)
    for k, c in enumerate(c0):
        scene.Add(Sphere.NewSphere(Vector(float(c[0]), float(c[1]), float(c[2])), float(np.float32(0.1)), materials[mats[k // (N - 1)]]))
    scene.Add(Sphere.NewSphere(Vector(4, 4, 20), 2, Material.LightMaterial(Colour.HexColor(0xFFFFFF), 30)))
    camera = Camera.LookAt(Vector(4, 2, 8), Vector(0, 0, 0), Vector(0, 0, 1), 40)
    sampler = DefaultSampler.NewSampler(4, 4)
    sampler.SpecularMode = SpecularMode.SpecularModeFirst
    return scene, camera, sampler, pos


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


def timed_uploads(lib, ctx, flat, reps, warmup):
    wall = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            wall.append(dt)
    return {"wall_ms": summary(wall)}


def step(lib, ctx, camera, sampler, spp, reps, warmup):
    cam, smp = camera.to_c(), sampler.to_c()
    ms, rays = [], []
    for i in range(warmup + reps):
        pp = _abi.pt_pass_params(spp, 0, 1234, i + 1, 0, C.POINTER(C.c_int32)(), _abi.ENGINE_AUTO, 0, 0, 0, 1)
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
    ap.add_argument("--upload-reps", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--lib", default=_abi.LIB_PATH)
    ap.add_argument("--upload-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shapes_bench.json"))
    a = ap.parse_args()
    lib = load(a.lib)
    scene, camera, sampler, pos = beads()
    flat = scene.Compile()
    ns = len(flat.sphere_radius)
    assert ns == STRANDS * (N - 1) + 1
    rest = flat.sphere_center.copy()
    moved = rest.copy()
    moved[:-1] = centres(pos, 0.5)
    doc = {"tool": "tools/shapes_bench.py", "scene": "beads frame (Example.cs:163-223), seeded", "spheres": ns,
           "pose": "t = 0 uploaded, t = 0.5 moved to", "reps": a.reps, "warmup": a.warmup, "upload_reps": a.upload_reps,
           "step": f"{W}x{H} at {a.spp} spp, NewSampler(4,4)",
           "library": os.path.relpath(a.lib, ROOT) if a.lib.startswith(ROOT) else os.path.basename(a.lib)}
    ctx = C.c_void_p()
    opts = _abi.pt_device_opts(0, W, H)
    check(lib, lib.pt_create(C.byref(opts), C.byref(ctx)), "pt_create")
    try:
        if not a.upload_only:
            check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")   # t = 0
            poses = [moved, rest]   # the timed calls alternate between the two poses; the last one is `moved`
            wall, kernel = [], []
            total = a.warmup + a.reps
            for i in range(total):
                c = poses[(total - 1 - i) % 2]
                u = _abi.pt_shape_update(ns, 0, 0, 0, c.ctypes.data_as(C.POINTER(C.c_float)))
                ms = C.c_double(0.0)
                t0 = time.perf_counter()
                check(lib, lib.pt_update_shapes(ctx, C.byref(u), C.byref(ms)), "pt_update_shapes")
                dt = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    wall.append(dt)
                    kernel.append(ms.value)
            counts = (C.c_int64 * 4)()
            check(lib, lib.pt_read_shape_bvh(ctx, counts, None, None, None, None), "pt_read_shape_bvh")
            doc["update"] = {"wall_ms": summary(wall), "kernel_ms": summary(kernel), "nodes": int(counts[0]),
                             "records": int(counts[1]), "input_bytes": 12 * ns}
            doc["rays_refitted"] = step(lib, ctx, camera, sampler, a.spp, a.step_reps, 1)
        flat.sphere_center[...] = moved
        doc["upload"] = timed_uploads(lib, ctx, flat, a.upload_reps, 1)
        if not a.upload_only:
            doc["rays_fresh_upload"] = step(lib, ctx, camera, sampler, a.spp, a.step_reps, 1)
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
