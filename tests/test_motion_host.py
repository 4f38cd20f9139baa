"""ptsharp_amd/csrc/pt_motion.h on the host (no GPU): tests/native/motion_check.cpp runs the header's reprojection and
temporal merge over the rows written here (seeded rows of every kind of shape, a miss, points behind the previous camera,
non-finite values, a degenerate cube axis, r'/r; every merge status, Nh' = 1, Nh = 1, the cap, max_history = 0 and the
int32 clamp), plain and once more under AddressSanitizer + UndefinedBehaviorSanitizer, and what it writes is compared
with tests/motion_ref.py, the independent restatement the GPU tests use: bit for bit where only +, − and × occur (a
plane's P' = o + t·d, a miss, the matrix products of a TransformedShape, N, the status, the nearest pixel away from a
rounding boundary), and at the project's fp64 bar (rtol 1e-11, atol 1e-13, as test_denoise_host.py) where a division
or the sqrt enters."""
import os
import subprocess

import numpy as np
import pytest

import motion_ref as R

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
EXE = os.path.join(NATIVE, "_build", "motion_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "motion_check_asan")
RTOL, ATOL = 1e-11, 1e-13
W, H = 64, 48


def look_at(rng, eye, centre):
    """A camera as Camera.LookAt makes it: orthonormal u, v, w in fp32, m from a field of view."""
    w = centre - eye
    w /= np.linalg.norm(w)
    u = np.cross(np.array([0.0, 0.0, 1.0]) + 0.1 * rng.standard_normal(3), w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    f = lambda a: [float(x) for x in a.astype(np.float32)]
    return dict(p=f(eye), u=f(u), v=f(v), w=f(w), m=float(1.0 / np.tan(np.radians(rng.uniform(30, 70)) / 2)))


def point_rows():
    """[(what, kind, W, H, camera, payload)]"""
    rng = np.random.default_rng(20241)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    rows = []
    for i in range(240):
        eye = rng.uniform(-1, 1, 3) + np.array([0.0, -6.0, 1.0])
        cam = look_at(rng, eye, rng.uniform(-0.5, 0.5, 3))
        w, h = ((W, H), (37, 29), (1920, 1080))[i % 3]
        kind = i % 7
        o = f32(eye + 0.01 * rng.standard_normal(3))
        d = rng.standard_normal(3) * 0.3 + np.array(cam["w"])
        d = f32(d / np.linalg.norm(d))
        P = f32(rng.uniform(-1.5, 1.5, 3))
        if kind in (0, 1):
            v1, e1, e2 = f32(rng.uniform(-1, 1, 3)), f32(rng.uniform(-1, 1, 3)), f32(rng.uniform(-1, 1, 3))
            pv1, pe1, pe2 = f32(v1 + 0.2 * rng.standard_normal(3)), f32(e1 + 0.1 * rng.standard_normal(3)), f32(e2 + 0.1 * rng.standard_normal(3))
            pay = [*o, *d, *v1, *e1, *e2, *pv1, *pe1, *pe2]
            if kind == 1:
                pay += list(np.hstack([np.eye(3) + 0.2 * rng.standard_normal((3, 3)), rng.uniform(-1, 1, (3, 1))]).reshape(-1))
        elif kind == 2:
            pay = [*P, *f32(rng.uniform(-1, 1, 3)), rng.uniform(0.2, 2), *f32(rng.uniform(-1, 1, 3)), rng.uniform(0.2, 2)]
        elif kind == 3:
            lo, lo1 = f32(rng.uniform(-2, 0, 3)), f32(rng.uniform(-2, 0, 3))
            pay = [*P, *lo, *f32(lo + rng.uniform(0.5, 2, 3)), *lo1, *f32(lo1 + rng.uniform(0.5, 2, 3))]
        elif kind == 4:
            m = lambda: list(np.hstack([np.eye(3) + 0.3 * rng.standard_normal((3, 3)), rng.uniform(-1, 1, (3, 1))]).reshape(-1))
            pay = [*P, *m(), *m()]
        elif kind == 5:
            pay = [*o, *d, rng.uniform(1, 10)]
        else:
            pay = [*d]
        rows.append((f"seeded{i}", kind, w, h, cam, pay))
    rng = np.random.default_rng(7)
    cam = look_at(rng, np.array([0.0, -5.0, 0.0]), np.zeros(3))
    behind = [c - 3.0 * wk for c, wk in zip(cam["p"], cam["w"])]
    rows += [
        ("behind the camera", 5, W, H, cam, [*behind, 0.0, 0.0, 0.0, 1.0]),
        ("on the camera plane (c = 0)", 5, W, H, cam, [*cam["p"], *cam["u"], 2.0]),
        ("at the camera", 5, W, H, cam, [*cam["p"], 0.0, 0.0, 0.0, 0.0]),
        ("miss behind", 6, W, H, cam, [-x for x in cam["w"]]),
        ("miss ahead", 6, W, H, cam, list(cam["w"])),
        ("NaN point", 5, W, H, cam, [np.nan, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]),
        ("infinite point", 5, W, H, cam, [0.0, np.inf, 0.0, 0.0, 0.0, 0.0, 1.0]),
        ("huge point", 5, W, H, cam, [0.0, 1e200, 0.0, 0.0, 1e200, 0.0, 1e150]),
        ("far outside the image", 5, W, H, cam, [1e6, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]),
        ("degenerate triangle (det = 0)", 0, W, H, cam, [0, -5, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]),
        ("cube with a flat axis", 3, W, H, cam, [0.3, 0.5, 0.2, 0, 0.5, 0, 1, 0.5, 1, 0.1, 0.2, 0.3, 1.1, 0.9, 1.3]),
        ("cube flat on every axis", 3, W, H, cam, [0.3, 0.5, 0.2, 0.3, 0.5, 0.2, 0.3, 0.5, 0.2, 0.1, 0.2, 0.3, 1.1, 0.9, 1.3]),
        ("sphere grown 3x", 2, W, H, cam, [0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.5, 0.0, 0.25, 3.0]),
        ("sphere of radius 0", 2, W, H, cam, [0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.0, 0.25, 3.0]),
        ("pixel centre exactly", 5, W, H, cam, [*cam["p"], *cam["w"], 4.0]),
    ]
    return rows


# (what, mc, vc, nc, have_history, motion_status, mh, vh, nh, shape_p, prim_p, shape_q, prim_q, prev_depth, hist_depth, sigma, max_history)
def merge_rows():
    rng = np.random.default_rng(99)
    rows = []
    c = lambda: list(rng.uniform(0, 2, 3))
    for i in range(200):
        nc, nh = int(rng.integers(1, 9)), int(rng.integers(1, 200))
        rows.append((f"seeded{i}", c(), c(), nc, 1, 0, c(), c(), nh, 3, 17, 3, 17, 5.0, 5.0 * (1 + rng.uniform(-0.05, 0.05)), 0.1,
                     int(rng.integers(1, 64))))
    a, b, z = [0.5, 1.0, 1.5], [0.25, 0.5, 0.125], [0.0, 0.0, 0.0]
    hm, hv = [0.75, 0.5, 2.0], [3.0, 1.0, 0.5]
    ok = (3, 17, 3, 17, 5.0, 5.2, 0.1)
    rows += [
        ("status 7: N = 0", z, z, 0, 1, 0, hm, hv, 8, *ok, 32),
        ("status 7: NaN mean", [np.nan, 0, 0], b, 2, 1, 0, hm, hv, 8, *ok, 32),
        ("status 7: infinite variance", a, [0, np.inf, 0], 2, 1, 0, hm, hv, 8, *ok, 32),
        ("status 7 before status 1", z, z, 0, 0, 2, z, z, 0, *ok, 32),
        ("status 1", a, b, 2, 0, 0, z, z, 0, *ok, 32),
        ("status 1 before status 2", a, b, 2, 0, 2, z, z, 0, *ok, 32),
        ("status 2: outside", a, b, 2, 1, 1, hm, hv, 8, *ok, 32),
        ("status 2: no snapshot", a, b, 2, 1, 2, hm, hv, 8, *ok, 32),
        ("status 3: history N = 0", a, b, 2, 1, 0, z, z, 0, *ok, 32),
        ("status 3: history NaN", a, b, 2, 1, 0, [0, np.nan, 0], hv, 8, *ok, 32),
        ("status 4: shape", a, b, 2, 1, 0, hm, hv, 8, 3, 17, 4, 17, 5.0, 5.0, 0.1, 32),
        ("status 4: prim", a, b, 2, 1, 0, hm, hv, 8, 3, 17, 3, 18, 5.0, 5.0, 0.1, 32),
        ("status 4: miss against hit", a, b, 2, 1, 0, hm, hv, 8, -1, -1, 3, 17, 1e9, 5.0, 0.1, 32),
        ("status 5", a, b, 2, 1, 0, hm, hv, 8, 3, 17, 3, 17, 5.0, 5.6, 0.1, 32),
        ("status 5: shrunk sigma", a, b, 2, 1, 0, hm, hv, 8, 3, 17, 3, 17, 5.0, 5.2, 0.01, 32),
        ("depth test off", a, b, 2, 1, 0, hm, hv, 8, 3, 17, 3, 17, 5.0, 500.0, 0.0, 32),
        ("depth at the bound", a, b, 2, 1, 0, hm, hv, 8, 3, 17, 3, 17, 4.0, 4.5, 0.125, 32),
        ("two misses merge", a, b, 2, 1, 0, hm, hv, 8, -1, -1, -1, -1, 1e9, 1e9, 0.1, 32),
        ("merged, under the cap", a, b, 2, 1, 0, hm, hv, 8, *ok, 32),
        ("merged, at the cap", a, b, 2, 1, 0, hm, hv, 32, *ok, 32),
        ("merged, capped", a, b, 2, 1, 0, hm, hv, 500, *ok, 32),
        ("Nh' = 1", a, b, 2, 1, 0, hm, hv, 40, *ok, 1),
        ("Nh = 1", a, b, 2, 1, 0, hm, z, 1, *ok, 32),
        ("Nh = 1 with a stray V", a, b, 2, 1, 0, hm, hv, 1, *ok, 32),
        ("max_history = 0", a, b, 2, 1, 0, hm, hv, 40, *ok, 0),
        ("int32 clamp", a, b, 2147483647 - 5, 1, 0, hm, hv, 1 << 20, *ok, 1 << 20),
        ("int32 clamp to nothing", a, b, 2147483647, 1, 0, hm, hv, 9, *ok, 32),
        ("equal means", a, b, 4, 1, 0, a, hv, 6, *ok, 32),
    ]
    return rows


POINTS, MERGES = point_rows(), merge_rows()


def write_input(path):
    pts = np.zeros((len(POINTS), 64))
    for r, (_, kind, w, h, cam, pay) in zip(pts, POINTS):
        r[:16] = [kind, w, h, *cam["p"], *cam["u"], *cam["v"], *cam["w"], cam["m"]]
        r[16:16 + len(pay)] = pay
    mrg = np.zeros((len(MERGES), 24))
    for r, (_, mc, vc, nc, hh, ms, mh, vh, nh, sp, pp, sq, pq, pd, hd, sg, mx) in zip(mrg, MERGES):
        r[:] = [*mc, *vc, nc, hh, ms, *mh, *vh, nh, sp, pp, sq, pq, pd, hd, sg, mx]
    with open(path, "wb") as f:
        f.write(np.array([len(pts), len(mrg)], np.int64).tobytes())
        f.write(pts.tobytes())
        f.write(mrg.tobytes())


def run(exe, tmp, env=None):
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    write_input(src)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"motion_check: {len(POINTS)} points, {len(MERGES)} merges"
    return np.fromfile(dst, np.float64).reshape(-1, 8), r


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "motion.mk", "motion_check"], check=True)
    out, _ = run(EXE, str(tmp_path_factory.mktemp("motion")))
    return out


def bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        return bool(((a == b) | (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= ATOL + RTOL * np.abs(b))).all())


def reference_point(kind, w, h, cam, a):
    a = [float(x) for x in a] + [0.0] * 48
    if kind in (0, 1):
        u, v = R.bary(a[0:3], a[3:6], a[6:9], a[9:12], a[12:15])
        P1 = R.tri_point(a[15:18], a[18:21], a[21:24], u, v)
        if kind == 1:
            P1 = R.mat_point(a[24:36], P1)
    elif kind == 2:
        P1 = R.sphere_point(a[0:3], a[3:6], a[6], a[7:10], a[10])
    elif kind == 3:
        P1 = R.cube_point(a[0:3], a[3:6], a[6:9], a[9:12], a[12:15])
    elif kind == 4:
        P1 = R.xform_point(a[0:3], a[3:15], a[15:27])
    elif kind == 5:
        P1 = R.point(a[0:3], a[3:6], a[6])
    else:
        P1 = a[0:3]
        xy, pixel, status = R.project(cam, w, h, P1)
        return P1, xy, R.INF, pixel, status
    xy, depth, pixel, status = R.project_point(cam, w, h, P1)
    return P1, xy, depth, pixel, status


def test_points_match_the_reference(native):
    seen_status, edge = set(), 0
    for got, (what, kind, w, h, cam, pay) in zip(native, POINTS):
        P1, xy, depth, pixel, status = reference_point(kind, w, h, cam, pay)
        exact = kind in (4, 5, 6)   # only +, −, × up to P'
        assert (same if exact else close)(got[0:3], P1), (what, got[0:3], P1)
        assert close(got[3:5], xy), (what, got[3:5], xy)
        assert close(got[5], depth), (what, got[5], depth)
        if status == R.OK and R.near_pixel_edge(xy):
            edge += 1
        else:
            assert got[7] == status, (what, got[7], status)
            assert got[6] == pixel, (what, got[6], pixel)
        seen_status.add(status)
        if status == R.OK:
            assert 0 <= got[6] < w * h
        else:
            assert got[6] == -1
    assert seen_status == {R.OK, R.OUTSIDE}
    assert edge <= len(POINTS) // 100
    by_name = {p[0]: g for p, g in zip(POINTS, native)}
    for what in ("behind the camera", "on the camera plane (c = 0)", "at the camera", "miss behind", "NaN point", "infinite point",
                 "huge point", "degenerate triangle (det = 0)"):
        g = by_name[what]
        assert g[7] == R.OUTSIDE and g[6] == -1 and g[3] == -1.0 and g[4] == -1.0, (what, g)
    for what in ("NaN point", "infinite point", "huge point"):
        assert by_name[what][5] == R.INF
    g = by_name["far outside the image"]
    assert g[7] == R.OUTSIDE and g[6] == -1 and np.isfinite(g[3]) and g[3] != -1.0
    assert by_name["miss ahead"][7] == R.OK and by_name["miss ahead"][5] == R.INF
    g = by_name["cube with a flat axis"]
    assert g[1] == 0.2   # s = 0 on the flat axis: lo'
    assert same(by_name["cube flat on every axis"][0:3], [0.1, 0.2, 0.3])
    assert same(by_name["sphere grown 3x"][0:3], [0.5, -3.0, 0.25])
    assert not np.isfinite(by_name["sphere of radius 0"][0:3]).all()
    g = by_name["pixel centre exactly"]
    assert g[7] == R.OK and close(g[3:5], [(W - 1) / 2, (H - 1) / 2]) and close(g[5], 4.0)


def test_merges_match_the_reference(native):
    seen = set()
    for got, (what, mc, vc, nc, hh, ms, mh, vh, nh, sp, pp, sq, pq, pd, hd, sg, mx) in zip(native[len(POINTS):], MERGES):
        st = R.merge_status(R.valid(mc, vc, nc), bool(hh), ms, R.valid(mh, vh, nh), sp, pp, sq, pq, pd, hd, sg)
        m, v, n = (list(mc), list(vc), nc) if st != R.MERGED else R.merge(mc, vc, nc, mh, vh, nh, mx)
        assert got[7] == st, (what, got[7], st)
        assert got[6] == n, (what, got[6], n)
        if st != R.MERGED or min(nh, mx, 2147483647 - nc) <= 0:
            assert same(got[0:3], mc) and same(got[3:6], vc), what   # the Buffer's pixel as it stands
        else:
            assert close(got[0:3], m) and close(got[3:6], v), (what, got[:6], m, v)
        seen.add(st)
        prefix = what.split(":")[0]
        if prefix.startswith("status "):
            assert st == int(prefix.split()[1]), what
    assert seen == {0, 1, 2, 3, 4, 5, 7}
    by_name = {r[0]: g for r, g in zip(MERGES, native[len(POINTS):])}
    assert by_name["merged, under the cap"][6] == 10 and by_name["merged, at the cap"][6] == 34 and by_name["merged, capped"][6] == 34
    assert by_name["Nh' = 1"][6] == 3 and by_name["Nh = 1"][6] == 3
    assert by_name["max_history = 0"][6] == 2 and by_name["max_history = 0"][7] == 0
    assert by_name["int32 clamp"][6] == 2147483647 and by_name["int32 clamp to nothing"][6] == 2147483647
    assert by_name["depth test off"][7] == 0 and by_name["depth at the bound"][7] == 0 and by_name["two misses merge"][7] == 0
    # Nh' = 1 drops the history's spread: V = Vc + δ²·Nc/(Nc + 1)
    g = by_name["Nh' = 1"]
    assert close(g[3:6], [0.25 + (0.75 - 0.5) ** 2 * 2 / 3, 0.5 + (0.5 - 1.0) ** 2 * 2 / 3, 0.125 + (2.0 - 1.5) ** 2 * 2 / 3])
    # uncapped, the merge is the exact pooling of the two sample sets
    g = by_name["merged, under the cap"]
    assert close(g[0:3], [(2 * x + 8 * y) / 10 for x, y in zip([0.5, 1.0, 1.5], [0.75, 0.5, 2.0])])
    assert same(by_name["equal means"][0:3], [0.5, 1.0, 1.5])


def test_sanitized(tmp_path):
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "motion.mk", "asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out, r = run(EXE_ASAN, str(tmp_path), env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert len(out) == len(POINTS) + len(MERGES)
