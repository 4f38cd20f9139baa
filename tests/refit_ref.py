"""A numpy restatement of pt_update_triangles' refit, written from the description in
ptsharp_amd/csrc/pt_refit.h, pt_bvh.h and DESIGN.md §4c, not from the C++.

`refit(nodes, chunks, recs, src_of_pos, v1, v2, v3, n1, n2, n3)` takes the triangle BVH as
Renderer.ReadTriBvh() returns it before an update ([N, 32], [C, 32], [T, 32] uint32), the source triangle of
every record and the new arrays, and returns the words and the root box expected after the update.

Layout (pt_bvh.h): a node's words 0-2 are the origin (fp32), word 3 holds three exponent bytes (bias 127), the
inner-child count in bits 24-27 and the child count in bits 28-31, word 4 the first inner child's node index,
word 5 + slot is 0x80000000 + the chunk index of a leaf slot, words 8-31 the child bounds as binary16 integers,
rows lo.x hi.x lo.y hi.y lo.z hi.z of eight.  A chunk's word 0 is its first record and, in bits 29-30, its
triangle count - 1; words 1 + 9 t .. 9 + 9 t are {v1, e1, e2} of its triangle t.  A record's words 0-8 are
{v1, e1, e2}, 12-20 the normals, 21 the material, 24-29 the texture coordinates.
"""
from __future__ import annotations

import numpy as np

QMAX = 2047
F32 = np.float32


def src_of_pos_from(recs, flat) -> np.ndarray:
    """The source triangle of every record, by matching the records of a fresh upload (words 0-8 and 12-20) to
    the FlatScene's triangles.  Triangles that are byte-identical cannot be told apart: the scenes of the tests
    have none."""
    v1, v2, v3 = flat.tri_v1, flat.tri_v2, flat.tri_v3
    key = np.concatenate([v1, v2 - v1, v3 - v1, flat.tri_n1, flat.tri_n2, flat.tri_n3], axis=1).astype(F32).view(np.uint32)
    where = {}
    for s, k in enumerate(key):
        b = k.tobytes()
        assert b not in where, "two identical source triangles"
        where[b] = s
    got = np.concatenate([recs[:, 0:9], recs[:, 12:21]], axis=1)
    return np.array([where[np.ascontiguousarray(r).tobytes()] for r in got], np.int32)


def padded_boxes(v1, v2, v3):
    """The padded box of each triangle: pad = max(|lo|, |hi|) * 2.0e-6f + 1e-30f, every operation in fp32."""
    lo = np.minimum(np.minimum(v1, v2), v3).astype(F32)
    hi = np.maximum(np.maximum(v1, v2), v3).astype(F32)
    m = np.maximum(np.abs(lo), np.abs(hi))
    e = (m * F32(2.0e-6)).astype(F32) + F32(1e-30)
    return (lo - e).astype(F32), (hi + e).astype(F32)


def _half_bits(q) -> int:
    return int(np.array([q], np.float16).view(np.uint16)[0])   # 0..2047 are exact in binary16


def _quantize(los, his):
    """One node's words 0-2, the exponent bytes and words 8-31 from its children's exact boxes ([nc, 3] fp32)."""
    nc = len(los)
    origin, ebits, rows = np.zeros(3, F32), 0, np.zeros((6, 8), np.uint32)
    box = np.zeros(6, F32)
    for ax in range(3):
        o, top = los[:, ax].min(), his[:, ax].max()
        o64 = np.float64(o)
        ext = np.float64(top) - o64
        e = -126
        while e < 127 and QMAX * 2.0 ** e < ext:
            e += 1
        while e < 127 and np.ceil((his[:, ax].astype(np.float64) - o64) / 2.0 ** e).max() > QMAX:   # outward rounding
            e += 1
        step = 2.0 ** e
        ql = np.maximum(0.0, np.floor((los[:, ax].astype(np.float64) - o64) / step))
        qh = np.minimum(float(QMAX), np.maximum(0.0, np.ceil((his[:, ax].astype(np.float64) - o64) / step)))
        for k in range(8):
            rows[2 * ax, k] = _half_bits(ql[k]) if k < nc else 0x7C00      # +inf: an empty slot
            rows[2 * ax + 1, k] = _half_bits(qh[k]) if k < nc else 0xFC00  # -inf
        origin[ax] = o
        ebits |= (e + 127) << (8 * ax)
        box[ax], box[3 + ax] = o, top
    words = (rows[:, 0::2] | (rows[:, 1::2] << 16)).reshape(24)
    return origin.view(np.uint32), ebits, words, box


def _levels(nodes):
    depth = np.zeros(len(nodes), np.int64)
    for i, w in enumerate(nodes):   # children come after their parent
        nin = (int(w[3]) >> 24) & 15
        depth[int(w[4]):int(w[4]) + nin] = depth[i] + 1
    return depth


def root_box(nodes) -> np.ndarray:
    """The union of the root's slot boxes: origin + q * 2^(e - 127) in exact arithmetic, rounded outward to fp32."""
    w = nodes[0]
    nc = int(w[3]) >> 28
    box = np.array([np.inf] * 3 + [-np.inf] * 3, F32)
    halves = w[8:32].reshape(6, 4)
    q = np.stack([halves & 0xFFFF, halves >> 16], axis=2).reshape(6, 8).astype(np.uint16).view(np.float16).astype(np.float64)
    for ax in range(3):
        o = np.float64(w[ax:ax + 1].view(F32)[0])
        step = 2.0 ** (((int(w[3]) >> (8 * ax)) & 0xFF) - 127)
        for k in range(nc):
            lo, hi = o + q[2 * ax, k] * step, o + q[2 * ax + 1, k] * step
            fl, fh = F32(lo), F32(hi)
            if np.float64(fl) > lo:
                fl = np.nextafter(fl, F32(-np.inf))
            if np.float64(fh) < hi:
                fh = np.nextafter(fh, F32(np.inf))
            box[ax], box[3 + ax] = min(box[ax], fl), max(box[3 + ax], fh)
    return box


def refit(nodes, chunks, recs, src_of_pos, v1, v2, v3, n1=None, n2=None, n3=None):
    nodes, chunks, recs = nodes.copy(), chunks.copy(), recs.copy()
    src = np.asarray(src_of_pos, np.int64)
    a, b, c = (np.asarray(x, F32).reshape(-1, 3)[src] for x in (v1, v2, v3))
    geom = np.concatenate([a, (b - a).astype(F32), (c - a).astype(F32)], axis=1).astype(F32).view(np.uint32)   # [T, 9]
    recs[:, 0:9] = geom
    recs[:, 9:12] = 0
    if n1 is not None:
        recs[:, 12:21] = np.concatenate([np.asarray(x, F32).reshape(-1, 3)[src] for x in (n1, n2, n3)], axis=1).view(np.uint32)
        recs[:, 22:24] = 0
    lo, hi = padded_boxes(a, b, c)
    first = (chunks[:, 0] & 0x1FFFFFFF).astype(np.int64)
    count = ((chunks[:, 0] >> 29) & 3).astype(np.int64) + 1
    chunks[:, 1:] = 0
    clo = np.full((len(chunks), 3), np.inf, F32)
    chi = np.full((len(chunks), 3), -np.inf, F32)
    for t in range(3):
        on = count > t
        pos = first[on] + t
        chunks[on, 1 + 9 * t:10 + 9 * t] = geom[pos]
        clo[on] = np.minimum(clo[on], lo[pos])
        chi[on] = np.maximum(chi[on], hi[pos])
    depth = _levels(nodes)
    nlo = np.zeros((len(nodes), 3), F32)
    nhi = np.zeros((len(nodes), 3), F32)
    for i in sorted(range(len(nodes)), key=lambda i: -depth[i]):   # the deepest level first
        w = nodes[i]
        nc, nin = int(w[3]) >> 28, (int(w[3]) >> 24) & 15
        los, his = [], []
        for k in range(nc):
            if k < nin:
                los.append(nlo[int(w[4]) + k]); his.append(nhi[int(w[4]) + k])
            else:
                ci = (int(w[5]) + k) & 0x7FFFFFFF
                los.append(clo[ci]); his.append(chi[ci])
        origin, ebits, words, box = _quantize(np.array(los, F32), np.array(his, F32))
        w[0:3] = origin
        w[3] = (int(w[3]) & 0xFF000000) | ebits
        w[8:32] = words
        nlo[i], nhi[i] = box[:3], box[3:]
    return nodes, chunks, recs, (root_box(nodes) if len(nodes) else np.zeros(6, F32))
