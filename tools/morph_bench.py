#!/usr/bin/env python3
"""pt_morph_meshes against the host morph plus pt_update_meshes on one GPU in one process: what a frame of a mesh with
morph targets costs when it sends a weight per target instead of every vertex.

On the bench's default scene (scenes.bunny_frame, the 1M-triangle frame of bench.py's c4 workload: one mesh) with
`--targets` targets (default 16), each covering a contiguous eighth of the triangles (all three corners) with a smooth
bump along the rest normal and a small normal delta, so that neighbouring targets overlap by half, and `--live` of the
weights (default 4) non-zero, each figure the median of `--reps` calls after `--warmup` untimed ones, with min and max:

  morph      (a) pt_morph_meshes, no readback (what Renderer.MorphMeshes(mirror=False) calls): the wall time of the
             call and its out_kernel_ms (the morph kernel and the refits); before it pt_set_rest_pose and pt_set_morph
             once, each timed on its own, and pt_read_morph's counts (targets, deltas, padded entries);
  morph_skin (b) the same call with skin_matrices: `--bones` bones (default 32), tools/skin_bench.py's rig;
  host       (c) the host's numpy morph over the live targets (the same arithmetic, so the words agree), then
             pt_update_meshes with the normals given: the pass, the call's wall time and out_kernel_ms (the refits
             alone), and their sum.  The copy-and-refit call is the fair comparison: any host morpher still pays it;
  morph_kernel  (d) the morph kernel's own time and the bytes of its layout, padding included: per triangle 72 read of
             the rest pose, 72 written and the group word; per step of a slice 128 B of targets and 768 B of position
             deltas, 768 B more of normal deltas; 12 B per slice.  (An upper bound on what moves: a lane whose target
             is dead skips its delta loads, so delta lines whose 64 lanes are all dead or padding are never read.)
             The time comes from a kernel trace taken in a run of its own (rocprofv3 --kernel-trace --stats
             --output-format csv -- python3 tools/morph_bench.py --morph-only --step-reps 0 --out elsewhere.json);
             `--add-kernel-stats trace_kernel_stats.csv` then adds it to the document at --out and does nothing else
             (no GPU needed);
  step_*     one 16-spp 1920x1080 step after (a) and after (c).  The words on the device are equal (the triangle
             BVH's nodes and chunks are compared here, after (a) against (c), and after (b) against one host pass of
             skin(morph(rest))), so the two agree up to run-to-run noise.

`--morph-only` measures only (a) and (b).  `--host-only --lib PATH` measures only (c), through another build of the
library (one without pt_morph_meshes, to record what the only path cost there).  One JSON document goes to --out.
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
from ptsharp_amd import _abi, scenes  # noqa: E402
from skin_bench import HBM_PEAK, H, SPP, W, check, host_skin, load, rig, step, summary, tri_bvh_words  # noqa: E402

F32, F64 = np.float32, np.float64


def face(rest, num_targets):
    """The targets in pt_morph_desc's form: target k names every corner of the triangles [k n / T, k n / T + n / 8)
    (clipped at n), with dpos = 0.02 sin^2(pi u) N_rest (u the triangle's place in the range) and dnrm = 0.1 dpos."""
    n = len(rest[0])
    span = max(1, n // 8)
    first, corner, dpos, dnrm = [0], [], [], []
    for k in range(num_targets):
        lo = k * n // num_targets
        hi = min(n, lo + span)
        t = np.arange(lo, hi)
        u = (t - lo + 0.5) / span
        amp = (0.02 * np.sin(np.pi * u) ** 2)[:, None, None]
        nrm = np.stack([rest[3][lo:hi], rest[4][lo:hi], rest[5][lo:hi]], axis=1).astype(F64)     # [m, 3 corners, 3]
        d = (amp * nrm).astype(F32).reshape(-1, 3)
        corner.append((3 * t[:, None] + np.arange(3)[None, :]).reshape(-1).astype(np.int32))
        dpos.append(d)
        dnrm.append((0.1 * d.astype(F64)).astype(F32))
        first.append(first[-1] + len(d))
    return (np.ascontiguousarray(first, np.int64), np.ascontiguousarray(np.concatenate(corner)),
            np.ascontiguousarray(np.concatenate(dpos)), np.ascontiguousarray(np.concatenate(dnrm)))


def host_morph(rest, group, first, corner, dpos, dnrm, weights):
    """pt_morph_meshes' arithmetic in numpy (include/ptsharp_hip.h): the six arrays an update takes."""
    n = len(rest[0])
    acc_p = np.stack(rest[:3], axis=1).reshape(3 * n, 3).astype(F64)
    acc_n = np.stack(rest[3:], axis=1).reshape(3 * n, 3).astype(F64)
    live = np.zeros(3 * n, bool)
    for k, w in enumerate(weights):
        if not (w != 0):
            continue
        q = corner[first[k]:first[k + 1]]
        acc_p[q] = acc_p[q] + F64(w) * dpos[first[k]:first[k + 1]].astype(F64)
        acc_n[q] = acc_n[q] + F64(w) * dnrm[first[k]:first[k + 1]].astype(F64)
        live[q] = True
    live &= np.repeat(group >= 0, 3)
    out = [a.copy() for a in rest]
    sel = np.flatnonzero(live)
    p = acc_p[sel].astype(F32)
    d = acc_n[sel].astype(F32)
    l = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F32)
    d = (d / l[:, None]).astype(F32)
    for c in range(3):
        mine = sel % 3 == c
        out[c][sel[mine] // 3] = p[mine]
        out[3 + c][sel[mine] // 3] = d[mine]
    return out


def layout_bytes(n, slices, padded, has_dnrm):
    steps = padded // 64
    return 148 * n + steps * (128 + 768 * (2 if has_dnrm else 1)) + 12 * slices


def add_kernel_stats(out, csv_path):
    """k_morph_meshes' row of a rocprofv3 kernel-stats CSV into the document at `out`."""
    import csv
    with open(out) as f:
        doc = json.load(f)
    with open(csv_path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "k_morph_meshes" in r["Name"]]
    if len(rows) != 1:
        raise SystemExit(f"{csv_path}: {len(rows)} k_morph_meshes rows")
    r = rows[0]
    avg = float(r["AverageNs"]) * 1e-9
    moved_bytes = doc["morph_layout_bytes"]
    doc["morph_kernel"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own (morph alone and morph with skin launch the same kernel)",
                           "kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "average_us": round(avg * 1e6, 3),
                           "min_us": round(float(r["MinNs"]) * 1e-3, 3), "max_us": round(float(r["MaxNs"]) * 1e-3, 3),
                           "bytes": moved_bytes, "bytes_per_s": round(moved_bytes / avg, 0),
                           "of_hbm_peak_8e12": round(moved_bytes / avg / HBM_PEAK, 4)}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["morph_kernel"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-reps", type=int, default=3, help="timed 16-spp steps after each path (0: none)")
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--targets", type=int, default=16)
    ap.add_argument("--live", type=int, default=4)
    ap.add_argument("--bones", type=int, default=32)
    ap.add_argument("--lib", default=_abi.LIB_PATH)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--morph-only", action="store_true", help="only (a) and (b): the run a kernel trace is taken of")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph_bench.json"))
    ap.add_argument("--add-kernel-stats", metavar="CSV", help="add k_morph_meshes' time from a rocprofv3 kernel-stats CSV to --out and exit")
    a = ap.parse_args()
    if a.add_kernel_stats:
        return add_kernel_stats(a.out, a.add_kernel_stats)
    lib = load(a.lib)
    scene, camera, sampler = scenes.bunny_frame(a.tris)
    flat = scene.Compile()
    rest = [x.copy() for x in (flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3)]
    n, nm, nt, nb = len(flat.tri_material), len(flat.mesh_first), a.targets, a.bones
    group = np.full(n, -1, np.int32)
    for j in range(nm):
        group[int(flat.mesh_first[j]):int(flat.mesh_first[j]) + int(flat.mesh_count[j])] = j
    first, corner, dpos, dnrm = face(rest, nt)
    weights = np.zeros(nt, F32)
    weights[np.arange(a.live) * max(1, nt // max(1, a.live)) % nt] = np.linspace(0.4, 1.0, a.live).astype(F32)
    doc = {"tool": "tools/morph_bench.py", "scene": f"bunny_frame({a.tris})", "triangles": n, "meshes": nm, "targets": nt,
           "live_targets": int((weights != 0).sum()), "deltas": int(first[-1]), "bones": nb,
           "morph_targets": "target k: every corner of a contiguous eighth of the triangles from k n / T, 0.02 sin^2 bump along the rest normal, dnrm = 0.1 dpos",
           "reps": a.reps, "warmup": a.warmup, "step": f"{W}x{H} at {SPP} spp",
           "library": os.path.relpath(a.lib, ROOT) if a.lib.startswith(ROOT) else os.path.basename(a.lib)}
    lp, ip, fp, dp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    ctx = C.c_void_p()
    opts = _abi.pt_device_opts(0, W, H)
    check(lib, lib.pt_create(C.byref(opts), C.byref(ctx)), "pt_create")
    try:
        check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")   # the rest pose
        words_morph = words_both = None
        if not a.host_only:
            t0 = time.perf_counter()
            check(lib, lib.pt_set_rest_pose(ctx, n, *[x.ctypes.data_as(fp) for x in rest]), "pt_set_rest_pose")
            doc["set_rest_pose_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
            d = _abi.pt_morph_desc(n, nt, (C.c_int32 * 2)(0, 0), first.ctypes.data_as(lp), corner.ctypes.data_as(ip),
                                   dpos.ctypes.data_as(fp), dnrm.ctypes.data_as(fp))
            t0 = time.perf_counter()
            check(lib, lib.pt_set_morph(ctx, C.byref(d)), "pt_set_morph")
            doc["set_morph_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
            counts = (C.c_int64 * 3)()
            check(lib, lib.pt_read_morph(ctx, counts, None, None, None, None), "pt_read_morph")
            slices = 3 * ((n + 63) // 64)
            doc["padded_entries"] = int(counts[2])
            doc["padding_over_deltas"] = round(int(counts[2]) / max(1, int(counts[1])), 4)
            doc["morph_layout_bytes"] = layout_bytes(n, slices, int(counts[2]), True)
            mats, bones, sw = rig(rest, nb)
            sd = _abi.pt_skin_desc(n, nb, (C.c_int32 * 2)(0, 0), *[x.ctypes.data_as(ip) for x in bones], *[x.ctypes.data_as(fp) for x in sw])
            check(lib, lib.pt_set_skin(ctx, C.byref(sd)), "pt_set_skin")
            m = np.ascontiguousarray([k.m for k in mats], np.float64).reshape(-1, 16)
            for key, u in (("morph_skin", _abi.pt_mesh_morph(nt, 0, nb, 0, weights.ctypes.data_as(fp), m.ctypes.data_as(dp))),
                           ("morph", _abi.pt_mesh_morph(nt, 0, 0, 0, weights.ctypes.data_as(fp), None))):
                wall, kernel = [], []
                for i in range(a.warmup + a.reps):
                    ms = C.c_double(0.0)
                    t0 = time.perf_counter()
                    check(lib, lib.pt_morph_meshes(ctx, C.byref(u), C.byref(ms)), "pt_morph_meshes")
                    dt = (time.perf_counter() - t0) * 1e3
                    if i >= a.warmup:
                        wall.append(dt)
                        kernel.append(ms.value)
                doc[key] = {"wall_ms": summary(wall), "kernel_ms": summary(kernel), "input_bytes": 4 * nt + (128 * nb if key == "morph_skin" else 0)}
                if key == "morph_skin":
                    words_both = tri_bvh_words(lib, ctx)
            words_morph = tri_bvh_words(lib, ctx)
            if a.step_reps:
                doc["step_after_morph"] = step(lib, ctx, camera, sampler, a.step_reps, 1)
        host, wall, kernel, total = [], [], [], []
        moved = None
        for i in range(0 if a.morph_only else a.warmup + a.reps):
            ms = C.c_double(0.0)
            t0 = time.perf_counter()
            moved = host_morph(rest, group, first, corner, dpos, dnrm, weights)
            t1 = time.perf_counter()
            uu = _abi.pt_mesh_update(n, 0, (C.c_int32 * 2)(0, 0), *[x.ctypes.data_as(fp) for x in moved])
            check(lib, lib.pt_update_meshes(ctx, C.byref(uu), C.byref(ms)), "pt_update_meshes")
            t2 = time.perf_counter()
            if i >= a.warmup:
                host.append((t1 - t0) * 1e3)
                wall.append((t2 - t1) * 1e3)
                total.append((t2 - t0) * 1e3)
                kernel.append(ms.value)
        if not a.morph_only:
            doc["host"] = {"host_pass_ms": summary(host), "update_wall_ms": summary(wall), "wall_ms": summary(total),
                           "kernel_ms": summary(kernel), "input_bytes": 72 * n}
        if words_morph is not None and not a.morph_only:
            words_host = tri_bvh_words(lib, ctx)
            doc["words_equal"] = bool(all(np.array_equal(x, y) for x, y in zip(words_morph, words_host)))
            doc["host_over_morph_wall"] = round(doc["host"]["wall_ms"]["median"] / doc["morph"]["wall_ms"]["median"], 1)
            up, mo = doc["host"]["update_wall_ms"], doc["morph"]["wall_ms"]
            doc["update_call_over_morph_wall"] = round(up["median"] / mo["median"], 2)
            doc["morph_cheaper_than_update_call_beyond_spread"] = bool(mo["max"] < up["min"])
        if a.step_reps and not a.morph_only:
            doc["step_after_host"] = step(lib, ctx, camera, sampler, a.step_reps, 1)
            if "step_after_morph" in doc:
                sa, sb = doc["step_after_morph"]["step_ms"], doc["step_after_host"]["step_ms"]
                spread = max(sa["max"] - sa["min"], sb["max"] - sb["min"])
                doc["steps_agree"] = bool(abs(sa["median"] - sb["median"]) <= spread)
        if words_both is not None and not a.morph_only:
            # once, untimed: the composed call against the host's skin of the host's morph
            both = host_skin(moved, group, bones, sw, mats)
            uu = _abi.pt_mesh_update(n, 0, (C.c_int32 * 2)(0, 0), *[x.ctypes.data_as(fp) for x in both])
            check(lib, lib.pt_update_meshes(ctx, C.byref(uu), None), "pt_update_meshes")
            doc["words_equal_with_skin"] = bool(all(np.array_equal(x, y) for x, y in zip(words_both, tri_bvh_words(lib, ctx))))
    finally:
        lib.pt_destroy(ctx)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    if doc.get("words_equal") is False or doc.get("words_equal_with_skin") is False:
        raise SystemExit("the BVH words after pt_morph_meshes and after the host morph differ")


if __name__ == "__main__":
    main()
