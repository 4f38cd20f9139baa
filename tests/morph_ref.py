"""pt_morph_meshes' arithmetic, restated in numpy from its description in include/ptsharp_hip.h and DESIGN.md §4m,
independently of ptsharp_amd/csrc/pt_morph.h:

  a triangle of no mesh (group -1) takes its rest values bit for bit, whatever deltas name it;
  a delta of target t is live when weights[t] != 0 (false only for +-0; a NaN weight is live); a dead delta is skipped,
  not multiplied by zero;
  a corner of a mesh triangle with no live delta takes its rest position and rest normal bit for bit;
  otherwise, per component, a = float64(p), then over the corner's live deltas in ascending target order
  a = a + float64(w[t]) * float64(d); one conversion to fp32.  With normals given and a morph that carries dnrm the
  normal is accumulated the same way from the rest normal and dnrm, converted once, then normalised in fp32; else it
  is the rest normal.

`morph(rest, group, targets, weights, normals=True)` returns the six arrays pt_morph_meshes stages (v1, v2, v3, n1, n2,
n3, [n, 3] float32): rest the six rest arrays, group [n] (tri_group), targets a list of (corners, dpos) or (corners,
dpos, dnrm) per target (corners 3 * triangle + c, strictly ascending), weights one per target.  The normal deltas are
used when normals is true and every target carries them.  With normals=False the normals are the rest's (the caller
derives them afterwards).  Checked on the CPU against tests/native/morph_check.cpp's dump (tests/test_morph_host.py);
the GPU tests compare the device against it.  `packed(targets)` gives pt_morph_desc's arrays, `seeded_morph(n,
num_targets, seed)` a target list for those tests.
"""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64


def _normalize(a):
    a = np.ascontiguousarray(a, F32)
    l = np.sqrt(((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]).astype(F32)).astype(F32)
    return (a / l[:, None]).astype(F32)


def has_normal_deltas(targets):
    return len(targets) > 0 and all(len(t) > 2 and t[2] is not None for t in targets)


def morph(rest, group, targets, weights, normals=True):
    rest = [np.ascontiguousarray(a, F32).reshape(-1, 3) for a in rest]
    out = [a.copy() for a in rest]
    n = len(rest[0])
    group = np.asarray(group).reshape(-1)
    weights = np.ascontiguousarray(weights, F32).reshape(-1)
    assert len(weights) == len(targets)
    with_n = bool(normals) and has_normal_deltas(targets)
    # corner q = 3 t + c is row t of array c: one [3n, 3] fp64 accumulator per kind, rows numbered by q
    acc_p = np.stack(rest[:3], axis=1).reshape(3 * n, 3).astype(F64)
    acc_n = np.stack(rest[3:], axis=1).reshape(3 * n, 3).astype(F64)
    live = np.zeros(3 * n, bool)
    with np.errstate(all="ignore"):
        for t, target in enumerate(targets):            # ascending target order
            w = weights[t]
            if not (w != 0):                            # +-0 only; NaN != 0
                continue
            q = np.asarray(target[0], np.int64).reshape(-1)
            assert len(q) == 0 or (np.diff(q) > 0).all()    # strictly ascending: no corner twice in one step
            acc_p[q] = acc_p[q] + F64(w) * np.ascontiguousarray(target[1], F32).reshape(-1, 3).astype(F64)
            if with_n:
                acc_n[q] = acc_n[q] + F64(w) * np.ascontiguousarray(target[2], F32).reshape(-1, 3).astype(F64)
            live[q] = True
        live &= np.repeat(group >= 0, 3)
        pos = acc_p.astype(F32).reshape(n, 3, 3)
        nrm = _normalize(acc_n.astype(F32)).reshape(n, 3, 3) if with_n else None
    live = live.reshape(n, 3)
    for c in range(3):
        sel = live[:, c]
        out[c][sel] = pos[sel, c]
        if with_n:
            out[3 + c][sel] = nrm[sel, c]
    return out


def packed(targets):
    """pt_morph_desc's arrays: target_first [T + 1] int64, corner [D] int32, dpos [D, 3] float32 and dnrm [D, 3] float32
    or None when not every target carries normal deltas."""
    first = np.zeros(len(targets) + 1, np.int64)
    first[1:] = np.cumsum([len(np.asarray(t[0]).reshape(-1)) for t in targets])
    cat = lambda k, dtype, shape: np.ascontiguousarray(np.concatenate([np.asarray(t[k], dtype).reshape(shape) for t in targets]))
    return dict(target_first=first, corner=cat(0, np.int32, (-1,)), dpos=cat(1, F32, (-1, 3)),
                dnrm=cat(2, F32, (-1, 3)) if has_normal_deltas(targets) else None)


def tri_group(flat):
    """RefitTables::tri_group: the last mesh range that contains a triangle, -1 for a loose one."""
    g = np.full(len(flat.tri_material), -1, np.int32)
    for j, (f, n) in enumerate(zip(flat.mesh_first, flat.mesh_count)):
        g[int(f):int(f) + int(n)] = j
    return g


def seeded_morph(n, num_targets, seed, normal_deltas=True):
    """A list of num_targets targets over n triangles, seeded.  The patterns the packed format has to get right:
    target 0 touches every corner; target 1 (when there are more than two) is empty; the last target touches corner 0
    and the last corner; up to 40 targets in between all name the first corner of triangle min(70, n - 1) (a single
    long corner: its slice is as long as that corner, the other 63 lanes mostly padding) and a seeded window of corners
    each; of the targets past 42 every 97th names up to three seeded corners, the others are empty.  With n > 256 no
    target names a corner of the triangles 128..191: three slices with no delta."""
    rng = np.random.default_rng(seed)
    delta = lambda k: (rng.uniform(-0.3, 0.3, (k, 3)).astype(F32), rng.uniform(-0.5, 0.5, (k, 3)).astype(F32))
    long_corner = 3 * min(70, n - 1)
    hole = (lambda q: q[(q < 3 * 128) | (q >= 3 * 192)]) if n > 256 else (lambda q: q)
    targets = []
    for t in range(num_targets):
        if t == 0:
            q = np.arange(3 * n)
        elif t == 1 and num_targets > 2:
            q = np.zeros(0, np.int64)
        elif t == num_targets - 1:
            q = np.unique([0, 3 * n - 1])
        elif t < 42:
            lo = int(rng.integers(0, max(1, 3 * n - 8)))
            q = np.unique(np.concatenate([[long_corner], np.arange(lo, min(3 * n, lo + int(rng.integers(1, 64))))]))
        else:
            q = np.unique(rng.integers(0, 3 * n, int(rng.integers(0, 4)))) if t % 97 == 0 else np.zeros(0, np.int64)
        q = hole(np.asarray(q, np.int64))
        dp, dn = delta(len(q))
        targets.append((q.astype(np.int32), dp, dn) if normal_deltas else (q.astype(np.int32), dp))
    return targets


def seeded_weights(num_targets, seed):
    """One weight per target: about a third dead (+0, some -0), the others in [-1, 1.5]; targets 0 and the last live."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.0, 1.5, num_targets).astype(F32)
    dead = rng.uniform(size=num_targets) < 0.35
    w[dead] = 0.0
    w[dead & (np.arange(num_targets) % 2 == 1)] = -0.0
    w[0] = F32(0.75)
    w[-1] = F32(-0.5) if num_targets > 1 else w[-1]
    return w
