"""A numpy restatement of pt_rebuild_meshes and pt_tri_bvh_cost, written from the description in DESIGN.md §4g and
include/ptsharp_hip.h, not from the C++ (tests/test_rebuild_host.py checks it word for word against the native check).

With P triangles in the world triangle BVH:
  chunks  chunk ci holds positions 3 ci .. min(3 ci + 3, P) - 1; word 0 = 3 ci | (count - 1) << 29.
  nodes   h = the least integer >= 1 with 3 * 8^h >= P.  The deepest level has ceil(L / 8) nodes over 8 consecutive
          chunks each (n_in = 0, word 5 = 0x80000000 + the first chunk, word 6 = 2 bits per slot: count - 1); every
          level above groups 8 consecutive nodes of the level below (n_in = n, word 4 = the first child, word 5 =
          0x80000000, word 6 = 0).  Nodes are numbered level by level, the root 0.
  order   rounds r = 1 .. 3 h over segments of C_(r-1) = 3 * 8^h / 2^(r-1) positions: a segment that holds more than
          C_r triangles is sorted, stable and ascending, by key = min3 + max3 (fp32) on the axis with the largest fp32
          extent of the keys (ties: the lowest axis), keys compared as u ^ (u >> 31 ? 0xFFFFFFFF : 0x80000000).
Boxes, records and chunk lines then come from refit_ref.refit over the new order.
"""
from __future__ import annotations

import numpy as np

import refit_ref

F32 = np.float32


def plan(P: int):
    """(h, chunks, [nodes per level, the root's first])"""
    if P <= 0:
        return 0, 0, []
    h = 1
    while 3 * 8 ** h < P:
        h += 1
    L = -(-P // 3)
    counts, n = [], L
    for _ in range(h):
        n = -(-n // 8)
        counts.append(n)
    return h, L, counts[::-1]


def ordered_keys(v1, v2, v3) -> np.ndarray:
    """[n, 3] uint32: the three sort keys of every triangle."""
    a, b, c = (np.asarray(x, F32).reshape(-1, 3) for x in (v1, v2, v3))
    lo = np.minimum(np.minimum(a, b), c).astype(F32)
    hi = np.maximum(np.maximum(a, b), c).astype(F32)
    u = (lo + hi).astype(F32).view(np.uint32)
    return u ^ np.where(u >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def _value(o):
    """the fp32 value of an ordered key"""
    o = np.uint32(o)
    u = o ^ (np.uint32(0x80000000) if o >> np.uint32(31) else np.uint32(0xFFFFFFFF))
    return np.array([u], np.uint32).view(F32)[0]


def order(src_of_pos, v1, v2, v3) -> np.ndarray:
    """perm[new position] = the position the triangle had."""
    src = np.asarray(src_of_pos, np.int64)
    P = len(src)
    h, _, _ = plan(P)
    keys = ordered_keys(v1, v2, v3)[src]     # by starting position
    cur = np.arange(P, dtype=np.int64)
    for r in range(1, 3 * h + 1):
        seg = (3 * 8 ** h) >> (r - 1)
        half = seg // 2
        if P <= half:
            continue
        for first in range(0, P, seg):
            end = min(first + seg, P)
            if end - first <= half:
                continue
            k = keys[cur[first:end]]
            ext = [F32(_value(k[:, ax].max()) - _value(k[:, ax].min())) for ax in range(3)]
            ax = 0
            if ext[1] > ext[ax]:
                ax = 1
            if ext[2] > ext[ax]:
                ax = 2
            cur[first:end] = cur[first:end][np.argsort(k[:, ax], kind="stable")]
    return cur


def topology(P: int):
    """(nodes [N, 32] with words 3-7 set, chunks [L, 32] with word 0 set), uint32."""
    h, L, counts = plan(P)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    nodes = np.zeros((int(off[-1]), 32), np.uint32)
    chunks = np.zeros((L, 32), np.uint32)
    ci = np.arange(L, dtype=np.int64)
    cnt = np.minimum(3, P - 3 * ci)
    chunks[:, 0] = (3 * ci) | ((cnt - 1) << 29)
    for l in range(h):
        for j in range(counts[l]):
            w = nodes[off[l] + j]
            if l == h - 1:
                nc = min(8, L - 8 * j)
                w[3] = nc << 28
                w[5] = 0x80000000 + 8 * j
                w[6] = sum(int(cnt[8 * j + k] - 1) << (2 * k) for k in range(nc))
            else:
                nc = min(8, counts[l + 1] - 8 * j)
                w[3] = (nc << 28) | (nc << 24)
                w[4] = off[l + 1] + 8 * j
                w[5] = 0x80000000
    return nodes, chunks


def rebuild(recs, src_of_pos, v1, v2, v3, n1=None, n2=None, n3=None):
    """What pt_read_tri_bvh returns after pt_rebuild_meshes: (nodes, chunks, records, root box) and the new src_of_pos.
    recs: the records before the call ([P, 32] uint32), whose rows 3-7 move with their triangles."""
    src = np.asarray(src_of_pos, np.int64)
    perm = order(src, v1, v2, v3)
    moved = recs[perm].copy()
    new_src = src[perm].astype(np.int32)
    nodes, chunks = topology(len(src))
    nodes, chunks, out, box = refit_ref.refit(nodes, chunks, moved, new_src, v1, v2, v3, n1, n2, n3)
    return (nodes, chunks, out, box), new_src


def cost(nodes):
    """pt_tri_bvh_cost: every slot box as origin + q 2^(e - 127) in fp64; (inner, leaf, root area)."""
    if not len(nodes):
        return 0.0, 0.0, 0.0

    def area(lo, hi):
        d = hi - lo
        return 2.0 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0])

    inner = leaf = root = 0.0
    for i, w in enumerate(nodes):
        nc, nin = int(w[3]) >> 28, (int(w[3]) >> 24) & 15
        halves = w[8:32].reshape(6, 4)
        q = np.stack([halves & 0xFFFF, halves >> 16], axis=2).reshape(6, 8).astype(np.uint16).view(np.float16).astype(np.float64)
        o = w[0:3].view(F32).astype(np.float64)
        step = np.array([2.0 ** (((int(w[3]) >> (8 * ax)) & 0xFF) - 127) for ax in range(3)])
        lo = o[:, None] + q[0::2, :nc] * step[:, None]   # [3, nc]
        hi = o[:, None] + q[1::2, :nc] * step[:, None]
        for k in range(nc):
            a = area(lo[:, k], hi[:, k])
            if k < nin:
                inner += a
            else:
                leaf += a
        if i == 0:
            root = area(lo.min(axis=1), hi.max(axis=1))
    if root <= 0.0:
        return 0.0, 0.0, root
    return (root + inner) / root, leaf / root, root
