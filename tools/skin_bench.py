#!/usr/bin/env python3
"""pt_skin_meshes against the host skin plus pt_update_meshes on one GPU in one process: what a frame of a deforming
mesh costs when it sends a matrix per bone instead of every vertex.

On the bench's default scene (scenes.bunny_frame, the 1M-triangle frame of bench.py's c4 workload: one mesh) with
`--bones` bones (default 32) stacked along y, every corner blended from the four bones around its height with cubic
B-spline weights, and a twist about y that grows from bone to bone, each figure the median of `--reps` calls after
`--warmup` untimed ones, with min and max:

  skin       (a) pt_skin_meshes, no readback (what Renderer.SkinMeshes(mirror=False) calls): the wall time of the call
             and its out_kernel_ms (the skin kernel and the refits); before it pt_set_rest_pose and pt_set_skin once,
             each timed on its own;
  host       (b) the host's numpy blend over every corner (the same arithmetic, so the words agree), then
             pt_update_meshes with the normals given: the pass, the call's wall time and out_kernel_ms (the refits
             alone), and their sum;
  skin_kernel  the skin kernel's own time, the bytes it moves (220 per triangle: 72 read of the rest pose, the group
             word, 72 of the skin, 72 written) and their rate against the 8 TB/s HBM peak.  The time comes from a
             kernel trace taken in a run of its own (rocprofv3 --kernel-trace --stats --output-format csv -- python3
             tools/skin_bench.py --step-reps 0 --out elsewhere.json); `--add-kernel-stats trace_kernel_stats.csv` then
             adds it to the document at --out and does nothing else (no GPU needed);
  step_*     one 16-spp 1920x1080 step after (a) and after (b).  The words on the device are equal (the triangle
             BVH's nodes and chunks are compared here), so the two agree up to run-to-run noise; `steps_agree` says
             whether the medians differ by no more than the repetitions' spread.

`--skin-only` measures only (a).  `--host-only --lib PATH` measures only (b), through another build of the library
(one without pt_skin_meshes, to record what the only path cost there).  One JSON document goes to --out.
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
from ptsharp_amd import Vector, _abi, scenes  # noqa: E402
from ptsharp_amd.geometry import Matrix  # noqa: E402

W, H, SPP = 1920, 1080, 16
HBM_PEAK = 8.0e12
SKIN_BYTES_PER_TRIANGLE = 220
F32, F64 = np.float32, np.float64


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


def rig(rest, num_bones):
    """The bones' matrices and the skin: bones stacked along y over the mesh's height, bone b a turn of 0.02 b about y
    and a small lift; a corner at height f (in bones) takes bones floor(f) - 1 .. floor(f) + 2 (clamped) with the
    uniform cubic B-spline weights of f's fraction, which sum to 1."""
    mats = [Matrix.TranslateM(Vector(0, 0.002 * b, 0)).Mul(Matrix.RotateM(Vector(0, 1, 0), 0.02 * b)) for b in range(num_bones)]
    lo = min(float(v[:, 1].min()) for v in rest[:3])
    hi = max(float(v[:, 1].max()) for v in rest[:3])
    bones, weights = [], []
    for v in rest[:3]:
        f = (v[:, 1].astype(F64) - lo) / max(hi - lo, 1e-30) * (num_bones - 1)
        i = np.floor(f)
        t = f - i
        w = np.stack([(1 - t) ** 3, 3 * t ** 3 - 6 * t ** 2 + 4, -3 * t ** 3 + 3 * t ** 2 + 3 * t + 1, t ** 3], axis=1) / 6.0
        b = np.clip(i[:, None] + np.arange(-1, 3)[None, :], 0, num_bones - 1)
        bones.append(np.ascontiguousarray(b, np.int32))
        weights.append(np.ascontiguousarray(w, F32))
    return mats, bones, weights


def host_skin(rest, group, bones, weights, mats):
    """pt_skin_meshes' arithmetic in numpy (include/ptsharp_hip.h): the six arrays an update takes."""
    m = np.ascontiguousarray([k.m for k in mats], F64).reshape(-1, 16)
    out = [a.copy() for a in rest]
    mesh = group >= 0

    def blend(v, b, w, translate):
        x, y, z = (v[:, k].astype(F64) for k in range(3))
        acc = np.zeros((len(v), 3), F64)
        started = np.zeros(len(v), bool)
        for k in range(4):
            live = w[:, k] != 0
            mk = m[np.where(live, b[:, k], 0)]
            wk = w[:, k].astype(F64)
            term = np.empty((len(v), 3), F64)
            for r in range(3):
                s = (mk[:, 4 * r] * x + mk[:, 4 * r + 1] * y) + mk[:, 4 * r + 2] * z
                term[:, r] = wk * (s + mk[:, 4 * r + 3] if translate else s)
            first, more = live & ~started, live & started
            acc[first] = term[first]
            acc[more] += term[more]
            started |= live
        return acc, started

    with np.errstate(all="ignore"):
        for c in range(3):
            acc, live = blend(rest[c], bones[c], weights[c], True)
            sel = mesh & live
            out[c][sel] = acc[sel].astype(F32)
            acc, _ = blend(rest[3 + c], bones[c], weights[c], False)
            d = acc[sel].astype(F32)
            l = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F32)
            out[3 + c][sel] = (d / l[:, None]).astype(F32)
    return out


def step(lib, ctx, camera, sampler, reps, warmup):
    cam, smp = camera.to_c(), sampler.to_c()
    ms = []
    for i in range(warmup + reps):
        pp = _abi.pt_pass_params(SPP, 0, 1234, i + 1, 0, C.POINTER(C.c_int32)(), _abi.ENGINE_AUTO, 0, 0, 0, 1)
        check(lib, lib.pt_render_pass(ctx, C.byref(cam), C.byref(smp), C.byref(pp)), "pt_render_pass")
        s = _abi.pt_stats()
        check(lib, lib.pt_stats_get(ctx, C.byref(s)), "pt_stats_get")
        if i >= warmup:
            ms.append(s.last_pass_ms)
    check(lib, lib.pt_reset_buffer(ctx), "pt_reset_buffer")
    return {"step_ms": summary(ms)}


def tri_bvh_words(lib, ctx):
    counts = (C.c_int64 * 3)()
    check(lib, lib.pt_read_tri_bvh(ctx, counts, None, None, None, None), "pt_read_tri_bvh")
    nodes, chunks = np.zeros((int(counts[0]), 32), np.uint32), np.zeros((int(counts[1]), 32), np.uint32)
    up = C.POINTER(C.c_uint32)
    check(lib, lib.pt_read_tri_bvh(ctx, counts, nodes.ctypes.data_as(up), chunks.ctypes.data_as(up), None, None), "pt_read_tri_bvh")
    return nodes, chunks


def add_kernel_stats(out, csv_path):
    """k_skin_meshes' row of a rocprofv3 kernel-stats CSV into the document at `out`."""
    import csv
    with open(out) as f:
        doc = json.load(f)
    with open(csv_path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "k_skin_meshes" in r["Name"]]
    if len(rows) != 1:
        raise SystemExit(f"{csv_path}: {len(rows)} k_skin_meshes rows")
    r = rows[0]
    avg = float(r["AverageNs"]) * 1e-9
    moved_bytes = SKIN_BYTES_PER_TRIANGLE * doc["triangles"]
    doc["skin_kernel"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own", "kernel": r["Name"].split("(")[0],
                          "calls": int(r["Calls"]), "average_us": round(avg * 1e6, 3), "min_us": round(float(r["MinNs"]) * 1e-3, 3),
                          "max_us": round(float(r["MaxNs"]) * 1e-3, 3), "bytes_per_triangle": SKIN_BYTES_PER_TRIANGLE,
                          "bytes": moved_bytes, "bytes_per_s": round(moved_bytes / avg, 0),
                          "of_hbm_peak_8e12": round(moved_bytes / avg / HBM_PEAK, 4)}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["skin_kernel"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-reps", type=int, default=3, help="timed 16-spp steps after each path (0: none)")
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--bones", type=int, default=32)
    ap.add_argument("--lib", default=_abi.LIB_PATH)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--skin-only", action="store_true", help="only (a): the run a kernel trace is taken of")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skin_bench.json"))
    ap.add_argument("--add-kernel-stats", metavar="CSV", help="add k_skin_meshes' time from a rocprofv3 kernel-stats CSV to --out and exit")
    a = ap.parse_args()
    if a.add_kernel_stats:
        return add_kernel_stats(a.out, a.add_kernel_stats)
    lib = load(a.lib)
    scene, camera, sampler = scenes.bunny_frame(a.tris)
    flat = scene.Compile()
    rest = [x.copy() for x in (flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3)]
    n, nm, nb = len(flat.tri_material), len(flat.mesh_first), a.bones
    group = np.full(n, -1, np.int32)
    for j in range(nm):
        group[int(flat.mesh_first[j]):int(flat.mesh_first[j]) + int(flat.mesh_count[j])] = j
    mats, bones, weights = rig(rest, nb)
    doc = {"tool": "tools/skin_bench.py", "scene": f"bunny_frame({a.tris})", "triangles": n, "meshes": nm, "bones": nb,
           "rig": "bones stacked along y, bone b = translate(0, 0.002 b, 0) * rotate(y, 0.02 b); four B-spline weights per corner",
           "reps": a.reps, "warmup": a.warmup, "step": f"{W}x{H} at {SPP} spp",
           "library": os.path.relpath(a.lib, ROOT) if a.lib.startswith(ROOT) else os.path.basename(a.lib)}
    ip, fp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    ctx = C.c_void_p()
    opts = _abi.pt_device_opts(0, W, H)
    check(lib, lib.pt_create(C.byref(opts), C.byref(ctx)), "pt_create")
    try:
        check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")   # the rest pose
        words_skin = None
        if not a.host_only:
            t0 = time.perf_counter()
            check(lib, lib.pt_set_rest_pose(ctx, n, *[x.ctypes.data_as(fp) for x in rest]), "pt_set_rest_pose")
            doc["set_rest_pose_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
            d = _abi.pt_skin_desc(n, nb, (C.c_int32 * 2)(0, 0), *[x.ctypes.data_as(ip) for x in bones],
                                  *[x.ctypes.data_as(fp) for x in weights])
            t0 = time.perf_counter()
            check(lib, lib.pt_set_skin(ctx, C.byref(d)), "pt_set_skin")
            doc["set_skin_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
            m = np.ascontiguousarray([k.m for k in mats], np.float64).reshape(-1, 16)
            u = _abi.pt_mesh_skin(nb, 0, (C.c_int32 * 2)(0, 0), m.ctypes.data_as(dp))
            wall, kernel = [], []
            for i in range(a.warmup + a.reps):
                ms = C.c_double(0.0)
                t0 = time.perf_counter()
                check(lib, lib.pt_skin_meshes(ctx, C.byref(u), C.byref(ms)), "pt_skin_meshes")
                dt = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    wall.append(dt)
                    kernel.append(ms.value)
            doc["skin"] = {"wall_ms": summary(wall), "kernel_ms": summary(kernel), "input_bytes": 128 * nb}
            words_skin = tri_bvh_words(lib, ctx)
            if a.step_reps:
                doc["step_after_skin"] = step(lib, ctx, camera, sampler, a.step_reps, 1)
        host, wall, kernel, total = [], [], [], []
        for i in range(0 if a.skin_only else a.warmup + a.reps):
            ms = C.c_double(0.0)
            t0 = time.perf_counter()
            moved = host_skin(rest, group, bones, weights, mats)
            t1 = time.perf_counter()
            uu = _abi.pt_mesh_update(n, 0, (C.c_int32 * 2)(0, 0), *[x.ctypes.data_as(fp) for x in moved])
            check(lib, lib.pt_update_meshes(ctx, C.byref(uu), C.byref(ms)), "pt_update_meshes")
            t2 = time.perf_counter()
            if i >= a.warmup:
                host.append((t1 - t0) * 1e3)
                wall.append((t2 - t1) * 1e3)
                total.append((t2 - t0) * 1e3)
                kernel.append(ms.value)
        if not a.skin_only:
            doc["host"] = {"host_pass_ms": summary(host), "update_wall_ms": summary(wall), "wall_ms": summary(total),
                           "kernel_ms": summary(kernel), "input_bytes": 72 * n}
        if words_skin is not None and not a.skin_only:
            words_host = tri_bvh_words(lib, ctx)
            doc["words_equal"] = bool(all(np.array_equal(x, y) for x, y in zip(words_skin, words_host)))
            doc["host_over_skin_wall"] = round(doc["host"]["wall_ms"]["median"] / doc["skin"]["wall_ms"]["median"], 1)
        if a.step_reps and not a.skin_only:
            doc["step_after_host"] = step(lib, ctx, camera, sampler, a.step_reps, 1)
            if "step_after_skin" in doc:
                sa, sb = doc["step_after_skin"]["step_ms"], doc["step_after_host"]["step_ms"]
                spread = max(sa["max"] - sa["min"], sb["max"] - sb["min"])
                doc["steps_agree"] = bool(abs(sa["median"] - sb["median"]) <= spread)
    finally:
        lib.pt_destroy(ctx)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    if doc.get("words_equal") is False:
        raise SystemExit("the BVH words after pt_skin_meshes and after the host skin differ")


if __name__ == "__main__":
    main()
