"""A numpy restatement of pt_rebuild_blas and pt_blas_cost (ptsharp_amd/csrc/pt_blas_rebuild.h): the plan of a BLAS of
n triangles, the order from the rounds of stable sorts, the topology words, then tests/blas_refit_ref.py's refit over
the new order; and the per-BLAS surface-area cost.  tests/test_blas_rebuild_host.py checks it word for word against
tests/native/blas_rebuild_check.cpp's dump; the GPU tests compare the device against it.

Layouts as in blas_refit_ref.py: blas [B, 4] int32 (first node, nodes, first triangle, -), nodes [N, 32] uint32, recs /
shade [T, 12] uint32."""
import numpy as np

import blas_refit_ref as B
from shape_refit_ref import EMPTY, F

MAX_LEVELS = 10


def plan(n):
    """(h, leaves, nodes per level from the root) of a BLAS of n triangles."""
    h, cap = 1, 16
    while cap < n:
        h, cap = h + 1, cap * 4
    assert h <= MAX_LEVELS
    leaves = (n + 3) // 4
    counts = [(leaves + (1 << 2 * (h - l)) - 1) >> 2 * (h - l) for l in range(h)]
    return h, leaves, counts


def ordered_keys(v1, v2, v3):
    """rebuild_keys: min3 + max3 per axis in fp32, as bits that compare as the floats do."""
    with np.errstate(all="ignore"):
        lo = np.fmin(np.fmin(v1, v2), v3)
        hi = np.fmax(np.fmax(v1, v2), v3)
        u = (lo + hi).astype(F).view(np.uint32)
    return np.where(u >> 31, u ^ np.uint32(0xFFFFFFFF), u ^ np.uint32(0x80000000)).astype(np.uint32)


def unordered(o):
    o = np.asarray(o, np.uint32)
    return np.where(o >> 31, o ^ np.uint32(0x80000000), o ^ np.uint32(0xFFFFFFFF)).astype(np.uint32).view(F)


def axis_of(keys):
    """rebuild_axis over a segment's ordered keys [m, 3]: the largest fp32 extent, ties to the lowest axis."""
    with np.errstate(all="ignore"):
        ext = (unordered(keys.max(axis=0)) - unordered(keys.min(axis=0))).astype(F)
    ax = 0
    if ext[1] > ext[ax]:
        ax = 1
    if ext[2] > ext[ax]:
        ax = 2
    return ax


def order(keys):
    """The permutation of one BLAS: out[p] = the start position (relative to the BLAS) of the triangle that ends at p."""
    n = len(keys)
    h = plan(n)[0]
    vals = np.arange(n)
    for s in range(2 * h, 0, -1):
        seg = 4 << s
        for f in range(0, n, seg):
            end = min(n, f + seg)
            if end - f <= seg // 2:
                continue
            k = keys[vals[f:end]]
            vals[f:end] = vals[f:end][np.argsort(k[:, axis_of(k)], kind="stable")]
    return vals


def node_refs(n):
    """Words 24-27 of every node of the balanced tree of n triangles: [nodes, 4] uint32."""
    h, leaves, counts = plan(n)
    off = np.concatenate([[0], np.cumsum(counts)])
    refs = np.full((int(off[-1]), 4), EMPTY, np.uint32)
    for l in range(h):
        below = leaves if l == h - 1 else counts[l + 1]
        for j in range(counts[l]):
            for k in range(4):
                c = 4 * j + k
                if c >= below:
                    continue
                if l == h - 1:
                    cnt = min(4, n - 4 * c)
                    refs[off[l] + j, k] = 0x80000000 | (cnt - 1) << 29 | 4 * c
                else:
                    refs[off[l] + j, k] = off[l + 1] + c
    return refs


def rebuild(blas, nodes0, recs0, shade0, src_of_pos, v1, v2, v3, normals=None, node_cap=None):
    """The device's BLAS words after pt_rebuild_blas(PT_REBUILD_BLAS) with these arrays: blas, nodes, recs, shade, the
    meshes' unpadded boxes, and the new src_of_pos.  node_cap: the node count the upload gave each BLAS (default: the
    counts in blas); a BLAS whose balanced tree needs more keeps its topology and order."""
    v1, v2, v3 = (np.ascontiguousarray(a, F).reshape(-1, 3) for a in (v1, v2, v3))
    blas1 = np.array(blas, np.int32).copy()
    nodes, shade = nodes0.copy(), shade0.copy()
    src = np.asarray(src_of_pos, np.int64).copy()
    cap = [int(x) for x in (blas1[:, 1] if node_cap is None else node_cap)]
    for b, nt in enumerate(B.tri_counts(blas1, len(recs0))):
        n0, r0 = int(blas1[b, 0]), int(blas1[b, 2])
        if nt <= 0 or sum(plan(nt)[2]) > cap[b]:
            continue
        s = src[r0:r0 + nt]
        vals = order(ordered_keys(v1[s], v2[s], v3[s]))
        shade[r0:r0 + nt] = shade0[r0:r0 + nt][vals]
        src[r0:r0 + nt] = s[vals]
        refs = node_refs(nt)
        nn = len(refs)
        rows = nodes[n0:n0 + nn]
        rows[:, 24:28] = refs
        rows[:, 28:32] = 0
        for k in range(4):
            empty = refs[:, k] == EMPTY
            for ax in range(3):
                rows[empty, 8 * ax + k] = 0
                rows[empty, 8 * ax + 4 + k] = 0
        blas1[b, 1] = nn
    nodes, recs, shade, boxes = B.refit(blas1, nodes, recs0, shade, src, v1, v2, v3, normals=normals)
    return blas1, nodes, recs, shade, boxes, src


def cost(blas, nodes):
    """pt_blas_cost: [B, 3] float64 of (inner, leaf, root area)."""
    out = np.zeros((len(blas), 3), np.float64)
    for b, (n0, nn, _, _) in enumerate(np.asarray(blas, np.int64)):
        inner = leaf = area = 0.0
        for i in range(nn):
            w = nodes[n0 + i]
            used = [k for k in range(4) if int(w[24 + k]) != EMPTY]
            lo = np.array([[w[8 * ax + k:8 * ax + k + 1].view(F)[0] for ax in range(3)] for k in used], np.float64).reshape(-1, 3)
            hi = np.array([[w[8 * ax + 4 + k:8 * ax + 5 + k].view(F)[0] for ax in range(3)] for k in used], np.float64).reshape(-1, 3)
            d = hi - lo
            a = 2.0 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0])
            for k, ak in zip(used, a):
                if int(w[24 + k]) & 0x80000000:
                    leaf += ak
                else:
                    inner += ak
            if i == 0 and used:
                u = hi.max(axis=0) - lo.min(axis=0)
                area = 2.0 * (u[0] * u[1] + u[1] * u[2] + u[2] * u[0])
        out[b, 2] = area
        if area > 0:
            out[b, 0], out[b, 1] = (area + inner) / area, leaf / area
    return out
