"""pt_intersect / pt_occluded at degenerate rays against the oracle's loop over every shape.

The rays are tests/degenerate_rays.py's: direction components of exactly 0 and -0.0 (1/d = +-inf, NaN slabs),
1e-20, -1e-38 and a denormal, rays in the planes that node and leaf boxes share, through vertices, along cube
edges, tangent to spheres, inside the plane of a mesh of zero thickness.  tests/test_degenerate_rays_ref.py checks
on the CPU that they are what they claim and that the reference is well defined at them (no near ties).

The expected value is or_intersect(brute=1), the loop over every shape, and or_any_nearer, which is that loop
already: at these rays the reference's k-d tree walk does not equal its own loop ("Ray queries at
degenerate rays"), and a BVH can only promise the loop.  Per scene:
  1. the t of Renderer.Intersect equals the oracle's, bit for bit, for every ray;
  2. the kind is equal wherever something is hit (two triangles may tie bit for bit: no index is compared);
  3. Renderer.Occluded equals or_any_nearer at t_max = t, nextafter(t), t / 2, 2 t (5 and 1e9 for a miss);
  4. a second renderer's upload of the rest and flat scenes answers as the first did, bit for bit;
  5. the rays that failed when these tests were first run, by name (REGRESSIONS).
"""
import functools
from collections import Counter

import numpy as np
import pytest

import degenerate_rays as D
import oracle_lib as O
from test_gpu_refit import renderer

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def expected(name):
    """The case and the oracle's answers, computed once: (scene tuple, o, d, family, t, kind, {bound: (t_max, occluded)})."""
    st, ref_scene, (o, d, fam) = D.case(name)
    os_ = O.OracleScene(ref_scene)
    t, kind, _ = D.oracle_hits(os_, o, d, brute=True)
    occ = {what: (tm, D.oracle_any_nearer(os_, o, d, tm)) for what, tm in D.occlusion_bounds(t).items()}
    for a in (o, d, t, kind):
        a.setflags(write=False)
    return st, o, d, fam, t, kind, occ


def report(what, bad, fam, o, d, got, want):
    """The failure message: the count, the families it falls in, the first few rays with both answers."""
    lines = [f"{what}: {len(bad)} of {len(o)} rays differ, by family {dict(Counter(fam[bad].tolist()))}"]
    for i in bad[:4]:
        lines.append(f"    ray {i} [{fam[i]}] o {o[i].tolist()} d {d[i].tolist()}: device {got[i]!r}, oracle {want[i]!r}")
    return "\n".join(lines)


def answers(r, name):
    """What the device says of the case's rays, and the differences from the oracle as messages."""
    st, o, d, fam, t, kind, occ = expected(name)
    gt, gk = r.Intersect(o, d)
    failures = []
    bad = np.flatnonzero(gt.view(np.int64) != t.view(np.int64))
    if bad.size:
        failures.append(report(f"{name}: hit distance", bad, fam, o, d, gt, t))
    bad = np.flatnonzero((gk != kind) & (t < 1e9))
    if bad.size:
        failures.append(report(f"{name}: kind", bad, fam, o, d, gk, kind))
    blocked = {}
    for what, (tm, want) in occ.items():
        blocked[what] = r.Occluded(o, d, tm)
        bad = np.flatnonzero(blocked[what] != want)
        if bad.size:
            failures.append(report(f"{name}: occluded, t_max {what}", bad, fam, o, d, blocked[what], want))
    return (gt, gk, blocked), failures


@pytest.mark.parametrize("name", D.SCENES)
def test_the_device_answers_as_the_loop_over_every_shape(gpu, name):
    st = expected(name)[0]
    r = renderer(st)
    try:
        _, failures = answers(r, name)
    finally:
        r.close()
    hits = int((expected(name)[4] < 1e9).sum())
    print(f"{name}: {len(expected(name)[1])} rays, {hits} hit in the oracle, {len(failures)} checks failed")
    assert not failures, "\n" + "\n".join(failures)


@pytest.mark.parametrize("name", ["rest", "flat"])
def test_a_second_upload_answers_bit_for_bit(gpu, name):
    """The BVH build is deterministic at ties: another renderer, after a ResetBuffer, answers the same rays alike."""
    st = expected(name)[0]
    first, second = renderer(st), renderer(st)      # each context compiles and uploads the scene itself
    try:
        (t1, k1, b1), _ = answers(first, name)
        second.ResetBuffer()
        (t2, k2, b2), failures = answers(second, name)
        fam = expected(name)[3]
        for what, x, y in [("t", t1.view(np.int64), t2.view(np.int64)), ("kind", k1, k2)] + [(w, b1[w], b2[w]) for w in b1]:
            bad = np.flatnonzero(x != y)
            assert not bad.size, (f"{name}: the two uploads differ in {what} on {bad.size} rays, "
                                  f"by family {dict(Counter(fam[bad].tolist()))}, first {bad[:5]}: {x[bad[:5]]} vs {y[bad[:5]]}")
        assert not failures, "\n" + "\n".join(failures)
    finally:
        first.close()
        second.close()


# The two rays these tests first failed at, kept whatever the generators' seeds become.
REGRESSIONS = {
    # d.x = -1e-38 with o.x on a vertex plane: (origin - o) / d overflowed to +inf in node8_step while step / d
    # stayed finite, so every child of the node missed, those holding the ray's plane too (node8_offset).
    "tiny_component_overflows_the_node_offset": (
        "rest", [0.7999999523162842, 2.4213106632232666, -1.910062551498413],
        [-9.999999350456404e-39, -0.7363442182540894, 0.6766071319580078]),
    # a hit 6,043,687.8 away that grazes an edge at coordinates of 1e6: the triangle's fp32 t falls short of the
    # entry distance of its own padded box (6,043,803), and pt_occluded culled the box against nextafter(t).
    # Only the occlusion is asserted: which of two grazing hits a closest-hit walk keeps is the tree's.
    "grazing_hit_nearer_than_its_own_box": (
        "huge", [-4948847.0, 1100000.125, 1938270.5], [0.9511966705322266, 0.0, -0.3085852861404419]),
}


@pytest.mark.parametrize("case", list(REGRESSIONS))
def test_named_regressions(gpu, case):
    name, origin, direction = REGRESSIONS[case]
    st, ref_scene, _ = D.case(name)
    o, d = np.array([origin], np.float32), np.array([direction], np.float32)
    os_ = O.OracleScene(ref_scene)
    t, kind, _ = D.oracle_hits(os_, o, d, brute=True)
    assert t[0] < 1e9 and kind[0] == 3, "the oracle's loop hits a triangle here"
    r = renderer(st)
    try:
        if not D.nearer_than_own_box(os_, o, d)[0]:
            gt, gk = r.Intersect(o, d)
            assert gt.view(np.int64)[0] == t.view(np.int64)[0] and gk[0] == kind[0], f"{case}: device t {gt[0]!r} kind {gk[0]}, oracle t {t[0]!r} kind {kind[0]}"
        for what, tm in D.occlusion_bounds(t).items():
            want = D.oracle_any_nearer(os_, o, d, tm)
            got = r.Occluded(o, d, tm)
            assert got[0] == want[0], f"{case}: occluded at t_max {what} = {tm[0]!r}: device {got[0]}, oracle {want[0]}"
    finally:
        r.close()
