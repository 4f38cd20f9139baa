#!/usr/bin/env python3
"""pt_update_volumes against pt_upload_scene on one GPU in one process: what editing a Volume costs.

The scene is scenes.mixed at 1M triangles (the C5 kind: the mesh frame, an SDF shape, a Volume inside a
TransformedShape) with its Volume at 256x256x128: 64 MB of voxels, a 545 MB cell-major corners table (under
PT_VOL_CELLS_MAX) and 8.5 MB of sign bytes.  Each figure is the median of `--reps` calls after `--warmup` untimed
ones, with min and max:

  data       pt_update_volumes with new voxels: the wall time of the call (64 MB copied in, the kernel) and its
             out_kernel_ms (device time between two hipEvents around the kernel); the calls alternate between two grids;
  windows    pt_update_volumes with new windows only (120 B copied in): wall and kernel time likewise;
  upload     the wall time of pt_upload_scene of the edited scene: the host compile (the triangle BVH comes from the
             process-wide cache after the first upload, the Volume tables are built by the host loops every time)
             and every array copied in.  The only path a build without pt_update_volumes has.

The kernel's rate is its algorithmic bytes over out_kernel_ms: data = voxels read once + corners and signs written,
windows = corners read once + signs written; as a fraction of --hbm-gbs (the device's peak, 8000 GB/s by default).

`--upload-only --lib PATH` measures only `upload`, through another build of the library (one without
pt_update_volumes, to record what the only path cost there).  One JSON document goes to --out.
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
from ptsharp_amd import TransformedShape, _abi, scenes  # noqa: E402

VW, VH, VD = 256, 256, 128


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


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


def big_mixed(n_tris):
    """scenes.mixed with its Volume replaced by one of VW x VH x VD voxels under the same transform."""
    scene, camera, sampler = scenes.mixed(n_tris)
    inst = scene.Shapes[-1]
    vol = scenes.volume(VW, VH, VD, seed=5)[0].Shapes[0]
    scene.Shapes[-1] = TransformedShape.NewTransformedShape(vol, inst.Matrix)
    scene._flat = None
    return scene, vol


def other_grid(vol, seed):
    sl = np.stack(scenes.volume_slices(vol.W, vol.H, vol.D, seed))
    return np.ascontiguousarray(np.roll(sl, 5, axis=2).astype(np.float64).reshape(-1) / 255)


def timed(fn, reps, warmup):
    wall, kernel = [], []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        ms = fn(i)
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            wall.append(dt)
            kernel.append(ms)
    return wall, kernel


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--upload-reps", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--lib", default=_abi.LIB_PATH)
    ap.add_argument("--upload-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_update_bench.json"))
    a = ap.parse_args()
    lib = load(a.lib)
    scene, vol = big_mixed(a.tris)
    flat = scene.Compile()
    cells = (VW + 1) * (VH + 1) * (VD + 1)
    voxel_bytes, cell_bytes = 8 * VW * VH * VD, 64 * cells
    doc = {"tool": "tools/volume_update_bench.py", "scene": f"scenes.mixed({a.tris}) with its Volume at {VW}x{VH}x{VD}",
           "voxel_bytes": voxel_bytes, "cells": cells, "cells_table_bytes": cell_bytes, "runs_table_bytes": cells,
           "windows": len(vol.Windows), "reps": a.reps, "warmup": a.warmup, "upload_reps": a.upload_reps,
           "library": os.path.relpath(a.lib, ROOT) if a.lib.startswith(ROOT) else os.path.basename(a.lib)}
    ctx = C.c_void_p()
    opts = _abi.pt_device_opts(0, 64, 64)
    check(lib, lib.pt_create(C.byref(opts), C.byref(ctx)), "pt_create")
    try:
        t0 = time.perf_counter()
        check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")
        doc["first_upload_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)   # with the triangle BVH build
        grids = [other_grid(vol, 31), vol.Data.copy()]
        if not a.upload_only:
            info = (C.c_int64 * 8)()
            check(lib, lib.pt_read_volume(ctx, 0, info, None, None, None, None), "pt_read_volume")
            assert list(info[:3]) == [VW, VH, VD] and info[5] == 1 and info[6] == cells, list(info)
            dp, wp = C.POINTER(C.c_double), C.POINTER(_abi.pt_volume_window)
            nwin = len(vol.Windows)
            rows = [(_abi.pt_volume_window * nwin)(*[_abi.pt_volume_window(w.lo + s, w.hi + s, w.material, 0)
                                                      for w in flat.volumes[0].windows[:nwin]]) for s in (0.04, 0.0)]

            def update(data, wins):
                d1 = (dp * 1)(data.ctypes.data_as(dp)) if data is not None else None
                w1 = (wp * 1)(C.cast(wins, wp)) if wins is not None else None
                u = _abi.pt_volume_update(1, (C.c_int32 * 3)(), C.cast(d1, C.POINTER(dp)) if d1 else None,
                                          C.cast(w1, C.POINTER(wp)) if w1 else None)
                ms = C.c_double(0.0)
                check(lib, lib.pt_update_volumes(ctx, C.byref(u), C.byref(ms)), "pt_update_volumes")
                return ms.value

            total = a.warmup + a.reps   # the timed calls alternate; the last leaves the other grid and the dragged windows
            wall, kernel = timed(lambda i: update(grids[(total - 1 - i) % 2], None), a.reps, a.warmup)
            moved = voxel_bytes + cell_bytes + cells
            k = statistics.median(kernel)
            doc["data"] = {"wall_ms": summary(wall), "kernel_ms": summary(kernel), "input_bytes": voxel_bytes,
                           "kernel_bytes": moved, "kernel_gbs": round(moved / (k * 1e-3) / 1e9, 1),
                           "fraction_of_hbm": round(moved / (k * 1e-3) / 1e9 / a.hbm_gbs, 3)}
            wall, kernel = timed(lambda i: update(None, rows[(total - 1 - i) % 2]), a.reps, a.warmup)
            moved = cell_bytes + cells
            k = statistics.median(kernel)
            doc["windows_only"] = {"wall_ms": summary(wall), "kernel_ms": summary(kernel), "input_bytes": 24 * nwin,
                                   "kernel_bytes": moved, "kernel_gbs": round(moved / (k * 1e-3) / 1e9, 1),
                                   "fraction_of_hbm": round(moved / (k * 1e-3) / 1e9 / a.hbm_gbs, 3)}
            for w, r in zip(flat.volumes[0].windows[:nwin], rows[0]):
                w.lo, w.hi = r.lo, r.hi
        vol.Data[...] = grids[0]   # the edited scene: the array the FlatScene's pt_volume points at
        wall = []
        for i in range(1 + a.upload_reps):
            t0 = time.perf_counter()
            check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
        doc["upload"] = {"wall_ms": summary(wall)}
        if not a.upload_only:
            up = doc["upload"]["wall_ms"]["median"]
            doc["upload_over_data_update_wall"] = round(up / doc["data"]["wall_ms"]["median"], 1)
            doc["upload_over_windows_update_wall"] = round(up / doc["windows_only"]["wall_ms"]["median"], 1)
            doc["bar_held"] = bool(doc["data"]["wall_ms"]["median"] < up and doc["windows_only"]["wall_ms"]["median"] < up)
    finally:
        lib.pt_destroy(ctx)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
