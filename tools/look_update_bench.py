#!/usr/bin/env python3
"""pt_update_materials and pt_update_textures against pt_upload_scene on one GPU in one process: what editing the
look of a scene costs.

The scene is the C4 frame (scenes.bunny_frame at 1M triangles: the mesh, a floor cube, two light spheres) with one
4096x2048 environment texture added.  Each figure is the median of `--reps` calls after `--warmup` untimed ones, with
min and max, wall time of the call in ms:

  material_row     pt_update_materials with one changed row (a colour; the calls alternate between two);
  light_on         pt_update_materials that switches the floor's material on as a light, and off again the next call;
  texture_rgba8    pt_update_textures of the environment texture as RGBA8 with the table of NewTexture (33.5 MB over
                   the bus, decoded on the device), with the decode kernel's out_kernel_ms;
  texture_f64      the same image as PT_TEXELS_F64 (201 MB over the bus, a copy into place);
  upload           pt_upload_scene of the descriptor with the changed row: what a caller without these calls does.

`--upload-only --lib PATH` measures only `upload`, through another build of the library (the parent commit's, which has
none of these entry points: what the only path cost there); --out then names that document.

With --step, one 16-spp pass of the frame is timed after an update and after the equivalent fresh upload (neither route
changes a kernel).  One JSON document goes to --out."""
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
from ptsharp_amd import Renderer, _abi, scenes  # noqa: E402
from ptsharp_amd.geometry import Colour  # noqa: E402
from ptsharp_amd.scene import ColorTexture  # noqa: E402

TW, TH = 4096, 2048


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def timed(fn, reps, warmup):
    out, extra = [], []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        e = fn(k)
        dt = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            out.append(dt)
            if e is not None:
                extra.append(e)
    return out, extra


def load(path):
    """The library at `path` with the prototypes of the entry points it has."""
    lib = C.CDLL(path)
    for name, (res, args) in _abi.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def big_scene(tris):
    scene, cam, smp = scenes.bunny_frame(tris)
    px = np.random.default_rng(3).integers(0, 256, (TH, TW, 4), dtype=np.uint8)
    scene.Texture = ColorTexture.NewTexture(px)
    return scene, cam, smp, px


def upload_only(a):
    lib = load(a.lib or _abi.LIB_PATH)
    scene = big_scene(a.tris)[0]
    flat = scene.Compile()
    ctx = C.c_void_p()
    opts = _abi.pt_device_opts(0, 1920, 1080)
    assert lib.pt_create(C.byref(opts), C.byref(ctx)) == _abi.PT_OK, lib.pt_last_error()

    def upload(k):
        flat.materials[0].color[0] = 0.25 + 0.5 * (k & 1)
        assert lib.pt_upload_scene(ctx, C.byref(flat.desc)) == _abi.PT_OK, lib.pt_last_error()

    t0 = time.perf_counter()
    upload(0)
    doc = {"scene": f"bunny_frame({a.tris}) + {TW}x{TH} environment texture", "reps": a.reps, "warmup": a.warmup,
           "library": "another build (--lib)" if a.lib else "this build", "has_pt_update_materials": hasattr(lib, "pt_update_materials"),
           "unit": "ms, wall time of the call", "first_upload_ms": round((time.perf_counter() - t0) * 1e3, 2)}
    doc["upload"] = summary(timed(upload, a.reps, a.warmup)[0])
    lib.pt_destroy(ctx)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--upload-only", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "look_update_bench.json"))
    a = ap.parse_args()
    if a.upload_only:
        return upload_only(a)
    scene, cam, smp, px = big_scene(a.tris)
    r = Renderer.NewRenderer(scene, cam, smp, 1920, 1080, True, device=0)
    r.SamplesPerPixel, r.Seed, r.Engine = 16, 1234, _abi.ENGINE_WAVEFRONT
    flat = scene.Compile()
    doc = {"scene": f"bunny_frame({a.tris}) + {TW}x{TH} environment texture", "reps": a.reps, "warmup": a.warmup,
           "materials": len(flat.material_list), "unit": "ms, wall time of the call"}
    lib = r._lib
    t0 = time.perf_counter()
    _abi.check(lib.pt_upload_scene(r._ctx, C.byref(flat.desc)), "pt_upload_scene")
    doc["first_upload_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    r._uploaded = flat

    def upload(k):
        flat.materials[0].color[0] = 0.25 + 0.5 * (k & 1)
        _abi.check(lib.pt_upload_scene(r._ctx, C.byref(flat.desc)), "pt_upload_scene")

    doc["upload"] = summary(timed(upload, a.reps, a.warmup)[0])
    base = list(flat.material_list)
    floor = [i for i, m in enumerate(base) if m.Emittance == 0][0]

    def row(k):
        r.UpdateMaterials({floor: base[floor].with_(Color=Colour(0.25 + 0.5 * (k & 1), 0.5, 0.5))}, mirror=False)

    def light(k):
        r.UpdateMaterials({floor: base[floor].with_(Emittance=0.0 if k & 1 else 2.0)}, mirror=False)

    lut = scene.Texture.Table()
    f64 = np.ascontiguousarray(lut[px[:, :, :3]])
    doc["material_row"] = summary(timed(row, a.reps, a.warmup)[0])
    doc["light_on"] = summary(timed(light, a.reps, a.warmup)[0])
    r.UpdateMaterials({floor: base[floor]}, mirror=False)
    wall, kern = timed(lambda k: r.UpdateTextures({0: (px, lut)}, mirror=False), a.reps, a.warmup)
    doc["texture_rgba8"] = dict(summary(wall), kernel_ms=summary(kern), bus_bytes=int(px.nbytes + 2048),
                                written_bytes=int(TW * TH * 24))
    doc["texture_f64"] = dict(summary(timed(lambda k: r.UpdateTextures({0: f64}, mirror=False), a.reps, a.warmup)[0]),
                              bus_bytes=int(f64.nbytes))
    got = r.ReadTexture(0)
    doc["texels_equal_host"] = bool(np.array_equal(got.view(np.uint64), f64.view(np.uint64)))
    if a.step:
        def step():
            r.ResetBuffer()
            t0 = time.perf_counter()
            r.RenderParallel()
            r.Synchronize()
            return (time.perf_counter() - t0) * 1e3
        r.UpdateMaterials({floor: base[floor].with_(Color=Colour(0.3, 0.6, 0.4))}, mirror=False)
        after_update = [step() for _ in range(5)][1:]
        flat.materials[floor].color[0], flat.materials[floor].color[1], flat.materials[floor].color[2] = 0.3, 0.6, 0.4
        _abi.check(lib.pt_upload_scene(r._ctx, C.byref(flat.desc)), "pt_upload_scene")
        after_upload = [step() for _ in range(5)][1:]
        doc["step_16spp_after_update"] = summary(after_update)
        doc["step_16spp_after_upload"] = summary(after_upload)
    r.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
