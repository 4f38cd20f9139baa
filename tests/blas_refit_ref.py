"""A numpy restatement of pt_update_meshes' part for instanced meshes (ptsharp_amd/csrc/pt_blas_refit.h) in fp32, each
operation rounded on its own: the BLAS triangle rows, each mesh's unpadded box and the bottom-up refit of every BLAS.
tests/test_blas_refit_host.py checks it against tests/native/blas_check.cpp's dump; the GPU tests compare the device
against it word for word, and feed its boxes to tests/shape_refit_ref.py as the transformed shapes' inner boxes.

Layouts: blas [B, 4] int32 (first node, nodes, first triangle, -: pt_read_blas'), nodes [N, 32] uint32 (pt_bvh.h; child
references and leaf firsts relative to the BLAS), recs / shade [T, 12] uint32 ({v1, e1, e2, 0 0 0} / {n1, n2, n3,
material, 0 0})."""
import numpy as np

from shape_refit_ref import EMPTY, F, pad_box


def tri_counts(blas, total):
    """Triangles per BLAS: each BLAS's run ends where the next begins."""
    first = [int(b[2]) for b in blas] + [int(total)]
    return [first[i + 1] - first[i] for i in range(len(blas))]


def source_of_positions(blas, recs0, mesh_first, mesh_count, meshes, v1, v2, v3):
    """src_of_pos recovered from the upload's words: the source triangle of every BLAS position, matched by its
    geometry rows {v1, v2 - v1, v3 - v1} (duplicates take the first unused one: their rows are the same)."""
    src = np.full(len(recs0), -1, np.int64)
    for b, j in enumerate(meshes):
        f, n, r0 = int(mesh_first[j]), int(mesh_count[j]), int(blas[b][2])
        keys = np.concatenate([v1[f:f + n], (v2[f:f + n] - v1[f:f + n]).astype(F), (v3[f:f + n] - v1[f:f + n]).astype(F)],
                              axis=1).astype(F).view(np.uint32)
        at = {}
        for t in range(n):
            at.setdefault(keys[t].tobytes(), []).append(f + t)
        for t in range(n):
            src[r0 + t] = at[recs0[r0 + t, :9].tobytes()].pop(0)
    return src


def refit(blas, nodes0, recs0, shade0, src_of_pos, v1, v2, v3, normals=None):
    """The device's BLAS words after an update with these arrays ([n, 3] float32 in scene order; normals: (n1, n2, n3)
    or None, the normals stay): nodes, recs, shade, and the meshes' unpadded boxes [B, 6]."""
    v1, v2, v3 = (np.ascontiguousarray(a, F).reshape(-1, 3) for a in (v1, v2, v3))
    nodes, recs, shade = nodes0.copy(), recs0.copy(), shade0.copy()
    s = np.asarray(src_of_pos, np.int64)
    a, b, c = v1[s], v2[s], v3[s]
    with np.errstate(all="ignore"):
        recs[:, 0:3] = a.view(np.uint32)
        recs[:, 3:6] = (b - a).astype(F).view(np.uint32)
        recs[:, 6:9] = (c - a).astype(F).view(np.uint32)
        recs[:, 9:12] = 0
        if normals is not None:
            n1, n2, n3 = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in normals)
            shade[:, 0:3], shade[:, 3:6], shade[:, 6:9] = n1[s].view(np.uint32), n2[s].view(np.uint32), n3[s].view(np.uint32)
            shade[:, 10:12] = 0
        lo = np.minimum(np.minimum(a, b), c)
        hi = np.maximum(np.maximum(a, b), c)
        tlo, thi = pad_box(lo, hi)
    tri_box = np.concatenate([tlo, thi], axis=1)
    boxes = np.zeros((len(blas), 6), F)
    counts = tri_counts(blas, len(recs))
    for bi, (n0, nn, r0, _) in enumerate(np.asarray(blas, np.int64)):
        nt = counts[bi]
        if nt > 0:
            boxes[bi] = np.concatenate([lo[r0:r0 + nt].min(axis=0), hi[r0:r0 + nt].max(axis=0)])
        node_box = np.zeros((nn, 6), F)
        for n in range(nn - 1, -1, -1):   # children before parents: a child's index is greater than its parent's
            w = nodes[n0 + n]
            lo_all, hi_all = np.full(3, np.inf, F), np.full(3, -np.inf, F)
            for k in range(4):
                ref = int(w[24 + k])
                if ref == EMPTY:
                    continue
                if ref & 0x80000000:
                    first, cnt = ref & 0x1FFFFFFF, ((ref >> 29) & 3) + 1
                    tb = tri_box[r0 + first:r0 + first + cnt]
                    l, h = tb[:, :3].min(axis=0), tb[:, 3:].max(axis=0)
                else:
                    l, h = node_box[ref, :3], node_box[ref, 3:]
                for ax in range(3):
                    w[8 * ax + k] = l[ax:ax + 1].view(np.uint32)[0]
                    w[8 * ax + 4 + k] = h[ax:ax + 1].view(np.uint32)[0]
                lo_all, hi_all = np.minimum(lo_all, l), np.maximum(hi_all, h)
            node_box[n] = np.concatenate([lo_all, hi_all])
    return nodes, recs, shade, boxes


def inner_boxes(xf_inner_box0, xf_blas, boxes):
    """The transformed shapes' inner boxes after the update: a mesh's new box where the shape is over one."""
    out = np.array(xf_inner_box0, F).reshape(-1, 6).copy()
    for t, b in enumerate(xf_blas):
        if b >= 0:
            out[t] = boxes[b]
    return out
