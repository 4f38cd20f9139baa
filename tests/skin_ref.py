"""pt_skin_meshes' arithmetic, restated in numpy from its description in include/ptsharp_hip.h and DESIGN.md §4l,
independently of ptsharp_amd/csrc/pt_skin.h:

  a triangle of no mesh (group -1) takes its rest values bit for bit, whatever its weights;
  an influence of a mesh triangle's corner is live when its weight != 0 (false only for +-0; a NaN weight is live);
  a corner with no live influence takes its rest position and, when the normals are given, its rest normal;
  otherwise, over the live influences in ascending order, the term is float64(weight) * P, P the three fp64 sums
  ((m0 x + m1 y) + m2 z) + m3 of Matrix.MulPosition; the accumulator is the first live term, every further live term is
  added to it (it never starts from 0); one conversion to fp32.  The given normals are blended the same way from
  MulDirection's sums (no translation), converted once, then normalised in fp32.

`skin(rest, group, bones, weights, matrices, normals=True)` returns the six arrays pt_skin_meshes stages (v1, v2, v3,
n1, n2, n3, [n, 3] float32): rest the six rest arrays, group [n] (tri_group), bones and weights [n, 3, 4], matrices
[B, 16] or [B, 4, 4] float64.  With normals=False the normals are the rest's (the caller derives them afterwards).
Checked on the CPU against tests/native/skin_check.cpp's dump (tests/test_skin_host.py); the GPU tests compare the
device against it.  `tri_group(flat)` and `seeded_skin(...)` serve those tests.
"""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64


def _sums(m, v, translate):
    """[n, 3] float64: row r is ((m[r,0] x + m[r,1] y) + m[r,2] z) (+ m[r,3]) with m [n, 16] and v [n, 3] float32."""
    x, y, z = (v[:, k].astype(F64) for k in range(3))
    out = np.empty((len(v), 3), F64)
    for r in range(3):
        s = m[:, 4 * r] * x
        s = s + m[:, 4 * r + 1] * y
        s = s + m[:, 4 * r + 2] * z
        if translate:
            s = s + m[:, 4 * r + 3]
        out[:, r] = s
    return out


def _normalize(a):
    a = np.ascontiguousarray(a, F32)
    l = np.sqrt(((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]).astype(F32)).astype(F32)
    return (a / l[:, None]).astype(F32)


def _blend(mats, v, bones, weights, translate):
    """The accumulator [n, 3] float64 and the mask of corners with a live influence."""
    n = len(v)
    acc = np.zeros((n, 3), F64)
    started = np.zeros(n, bool)
    for k in range(bones.shape[1]):
        w = weights[:, k]
        live = w != 0                                   # NaN != 0
        safe = np.where(live, bones[:, k], 0)           # a dead influence's matrix is never read
        term = w.astype(F64)[:, None] * _sums(mats[safe], v, translate)
        first = live & ~started
        more = live & started
        acc[first] = term[first]
        acc[more] = acc[more] + term[more]
        started |= live
    return acc, started


def skin(rest, group, bones, weights, matrices, normals=True):
    rest = [np.ascontiguousarray(a, F32).reshape(-1, 3) for a in rest]
    out = [a.copy() for a in rest]
    n = len(rest[0])
    group = np.asarray(group).reshape(-1)
    bones = np.asarray(bones, np.int64).reshape(n, 3, 4)
    weights = np.ascontiguousarray(weights, F32).reshape(n, 3, 4)
    mats = np.ascontiguousarray([getattr(m, "m", m) for m in matrices], F64).reshape(-1, 16)
    mesh = group >= 0
    with np.errstate(all="ignore"):
        for c in range(3):
            acc, live = _blend(mats, rest[c], bones[:, c], weights[:, c], True)
            sel = mesh & live
            out[c][sel] = acc[sel].astype(F32)
            if normals:
                acc, _ = _blend(mats, rest[3 + c], bones[:, c], weights[:, c], False)
                out[3 + c][sel] = _normalize(acc[sel].astype(F32))
    return out


def tri_group(flat):
    """RefitTables::tri_group: the last mesh range that contains a triangle, -1 for a loose one."""
    g = np.full(len(flat.tri_material), -1, np.int32)
    for j, (f, n) in enumerate(zip(flat.mesh_first, flat.mesh_count)):
        g[int(f):int(f) + int(n)] = j
    return g


def seeded_skin(n, num_bones, seed):
    """bones [n, 3, 4] int32 and weights [n, 3, 4] float32: per corner 1 to 4 live influences at seeded slots, weights
    summing to about 1; every eleventh corner all zero (one of them -0), every seventh a single weight of exactly 1."""
    rng = np.random.default_rng(seed)
    bones = rng.integers(0, num_bones, (n, 3, 4)).astype(np.int32)
    w = rng.uniform(0.05, 1.0, (n, 3, 4))
    dead = rng.uniform(size=(n, 3, 4)) < 0.4
    dead[..., 0] &= dead[..., 1:].all(axis=-1) ^ True     # never all four dead here
    w[dead] = 0.0
    w /= w.sum(axis=-1, keepdims=True)
    w = w.astype(F32)
    flat_w, flat_b = w.reshape(-1, 4), bones.reshape(-1, 4)
    flat_w[::11] = 0.0
    flat_w[::22, 2] = -0.0
    one = np.arange(3, len(flat_w), 7)
    flat_w[one] = 0.0
    flat_w[one, one % 4] = 1.0
    return flat_b.reshape(n, 3, 4), flat_w.reshape(n, 3, 4)
