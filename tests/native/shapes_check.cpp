// shapes_check.cpp — the arithmetic of pt_update_shapes (ptsharp_amd/csrc/pt_shape_refit.h) on the host: a CPU twin
// of the shape refit (the shared functions driven xforms, records, heavy, levels over the compile's tables, as
// pt_shape_refit.hip's kernels are) on scenes built in C++ (scene_fixture.h), checked against the host builder:
//   identity      a refit with the parameters a scene was compiled from reproduces every word of the BVH4 nodes,
//                 records, ext records, transforms, heavy records and lights (scenes beads, few, routed, instances,
//                 a single sphere: the lone-leaf root, and a scene without analytic shape);
//   poses         every slot box contains the record boxes of its subtree (by recursion); records, ext records,
//                 transforms, heavy boxes and lights equal a fresh compile's of the moved scene, matched per source
//                 shape; every record box equals the fresh compile's BVH box of that shape;
//   sequence      pose A then pose B gives the words of pose B alone; a group not given stays;
//   tables        the level table lists every node once, parents on lower levels than their children;
//   non-finite    NaN and infinite parameters run through the refit (under ASan: no access leaves its array).
// `--dump DIR` writes a pose of the routed and of the instances scene (every group moved), inputs and outputs, as raw
// arrays into DIR/routed and DIR/instances (tests/shape_refit_ref.py is checked against them).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../ptsharp_amd/csrc/pt_bvh.h"
#include "../../ptsharp_amd/csrc/pt_scene_compile.h"
#include "../../ptsharp_amd/csrc/pt_shape_refit.h"
#include "../../ptsharp_amd/csrc/pt_update_layout.h"
#include "layout_parts.h"
#include "scene_fixture.h"

static int failures = 0;
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            if (failures < 40) std::fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
            failures++;                                                           \
        }                                                                         \
    } while (0)

// ---- fixture scenes
enum { MAT_GREY = 0, MAT_EMIT = 1, MAT_BLUE = 2 };
static void materials(FixScene& s) {
    s.material(0.9, 0.9, 0.9, 0);
    s.material(1, 1, 1, 10);
    s.material(0.2, 0.3, 0.8, 0);
}
static void grid_mesh(FixScene& s, int n, float size, float y) {   // 2 n^2 triangles
    const int first = (int)s.tm.size();
    for (int j = 0; j < n; j++)
        for (int i = 0; i < n; i++) {
            auto vtx = [&](int a, int b, float* p) {
                p[0] = size * ((float)a / (float)n - 0.5f);
                p[2] = size * ((float)b / (float)n - 0.5f);
                p[1] = y + 0.1f * std::sin(3.f * p[0]) * std::cos(2.f * p[2]);
            };
            float a[3], b[3], c[3], e[3];
            vtx(i, j, a); vtx(i + 1, j, b); vtx(i, j + 1, c); vtx(i + 1, j + 1, e);
            s.triangle(a, b, c, MAT_BLUE);
            s.triangle(b, e, c, MAT_BLUE);
        }
    s.mfirst.push_back(first);
    s.mcount.push_back(2 * n * n);
}
// A, beads: 5 strands of 60 spheres, a floor cube, one sphere light: 302 records
static void beads_scene(FixScene& s) {
    materials(s);
    s.shape(PT_SHAPE_CUBE, s.cube(-8.f, -1.f, -8.f, 8.f, 0.f, 8.f, MAT_GREY));
    for (int k = 0; k < 5; k++)
        for (int i = 0; i < 60; i++) {
            const float a = 0.21f * (float)i + 1.3f * (float)k;
            s.shape(PT_SHAPE_SPHERE, s.sphere(3.f * std::cos(a) + 0.4f * (float)k, 0.3f + 0.05f * (float)i, 3.f * std::sin(a), 0.1, i % 7 ? MAT_GREY : MAT_BLUE));
        }
    s.shape(PT_SHAPE_SPHERE, s.sphere(0.f, 6.f, 0.f, 0.75, MAT_EMIT));
    s.finish(0);
}
// B, few: a floor cube, two sphere lights and a 200-triangle mesh
static void few_scene(FixScene& s) {
    materials(s);
    grid_mesh(s, 10, 4.f, 0.5f);
    s.shape(PT_SHAPE_CUBE, s.cube(-8.f, -1.f, -8.f, 8.f, 0.f, 8.f, MAT_GREY));
    s.shape(PT_SHAPE_SPHERE, s.sphere(-2.f, 5.f, 1.f, 0.5, MAT_EMIT));
    s.shape(PT_SHAPE_SPHERE, s.sphere(3.f, 4.f, -1.f, 0.25, MAT_EMIT));
    s.shape(PT_SHAPE_MESH, 0);
    s.finish(0);
}
// C, routed: a 3200-triangle grid, a floor cube, a sphere light, an SDF torus, a transformed Volume, a transformed
// sphere and an instanced 8-triangle mesh
static void routed_scene(FixScene& s) {
    materials(s);
    grid_mesh(s, 40, 6.f, 1.f);
    grid_mesh(s, 2, 1.f, 0.f);
    s.shape(PT_SHAPE_MESH, 0);
    s.shape(PT_SHAPE_CUBE, s.cube(-8.f, -1.f, -8.f, 8.f, 0.f, 8.f, MAT_GREY));
    s.shape(PT_SHAPE_SPHERE, s.sphere(0.f, 6.f, 0.f, 0.75, MAT_EMIT));
    const int torus = s.node(PT_SDF_TORUS, {1, 0.25, 2, 2}, {});
    s.sdfs = {pt_sdf_shape{s.node(PT_SDF_UNION, {}, {torus}), MAT_GREY}};   // (a lone leaf leaves sdf_children empty)
    s.shape(PT_SHAPE_SDF, 0);
    s.win0 = {pt_volume_window{0.2, 0.5, MAT_GREY, 0}};
    const int vol = s.volume(3, 3, 3, s.vox0, s.win0, -1.f, 1.f);
    s.shape(PT_SHAPE_TRANSFORMED, s.transformed(PT_SHAPE_VOLUME, vol, 4, 0.5, 1));
    s.shape(PT_SHAPE_TRANSFORMED, s.transformed(PT_SHAPE_SPHERE, s.sphere(0.f, 0.f, 0.f, 0.5, MAT_BLUE), -3, 2, 2));
    s.shape(PT_SHAPE_TRANSFORMED, s.transformed(PT_SHAPE_MESH, 1, -2, 3, -3));
    s.finish(0);
}
// D, instances: 60 transformed cubes and spheres, 50 spheres and a floor cube; four transforms share one inner sphere,
// which is a top-level shape too; one transformed cube is emissive
static void instances_scene(FixScene& s) {
    materials(s);
    s.shape(PT_SHAPE_CUBE, s.cube(-10.f, -1.f, -10.f, 10.f, 0.f, 10.f, MAT_GREY));
    const int shared = s.sphere(0.25f, 0.5f, -0.125f, 0.3, MAT_BLUE);
    s.shape(PT_SHAPE_SPHERE, shared);
    for (int i = 0; i < 50; i++)
        s.shape(PT_SHAPE_SPHERE, s.sphere(0.37f * (float)(i % 10) - 4.f, 0.4f + 0.3f * (float)(i / 10), 0.5f * (float)(i % 7) - 3.f, 0.15 + 0.01 * i, MAT_GREY));
    for (int i = 0; i < 60; i++) {
        const double x = 0.9 * (i % 8) - 3.0, y = 1.0 + 0.5 * (i / 8), z = 0.7 * (i % 5) + 1.0;
        int t;
        if (i < 4) t = s.transformed(PT_SHAPE_SPHERE, shared, x, y + 3, z);
        else if (i % 2) t = s.transformed(PT_SHAPE_SPHERE, s.sphere(0.f, 0.f, 0.f, 0.2, MAT_BLUE), x, y, z);
        else t = s.transformed(PT_SHAPE_CUBE, s.cube(-0.2f, -0.1f, -0.15f, 0.2f, 0.1f, 0.15f, i == 10 ? MAT_EMIT : MAT_GREY), x, y, z);
        s.shape(PT_SHAPE_TRANSFORMED, t);
    }
    s.finish(0);
}
static void one_scene(FixScene& s) {
    materials(s);
    s.shape(PT_SHAPE_SPHERE, s.sphere(1.f, 2.f, 3.f, 0.5, MAT_EMIT));
    s.finish(0);
}
static void none_scene(FixScene& s) {
    materials(s);
    grid_mesh(s, 2, 1.f, 0.f);
    s.shape(PT_SHAPE_MESH, 0);
    s.finish(0);
}

// ---- the CPU twin: the device state of a context and pt_update_shapes on it
struct Twin {
    std::vector<uint32_t> nodes, recs, ext, heavy;
    std::vector<pt::DevXform> xforms;
    std::vector<pt::DevLight> lights;
    pt::ShapeRefitTables T;
    std::vector<float> xbox, rec_box, node_box;
};
static void twin_of(const pt::HostScene& H, Twin& W) {
    const uint32_t* lines = (const uint32_t*)H.lines.data();
    W.nodes.assign(lines, lines + (size_t)H.S.tri_node_line0 * 32);
    W.recs.assign((const uint32_t*)H.ana_recs.data(), (const uint32_t*)H.ana_recs.data() + H.ana_recs.size() * 4);
    W.ext.assign((const uint32_t*)H.ext_recs.data(), (const uint32_t*)H.ext_recs.data() + H.ext_recs.size() * 4);
    W.heavy.assign((const uint32_t*)H.heavy.data(), (const uint32_t*)H.heavy.data() + H.heavy.size() * 4);
    W.xforms = H.xforms;
    W.lights = H.lights;
    W.T = H.shape_refit;
    W.xbox.assign((size_t)W.T.num_transformed * 6, 0.f);
    W.rec_box = W.T.rec_box;
    W.node_box.assign((size_t)W.T.num_nodes * 6, 0.f);
}
struct Pose {   // an empty array: the group is not given
    std::vector<float> sc, cmin, cmax;
    std::vector<double> sr, m, inv;
};
static void twin_update(Twin& W, const Pose& P) {
    pt::ShapeRefitTables& T = W.T;
    if (!P.sc.empty()) T.sphere_center = P.sc;
    if (!P.sr.empty()) T.sphere_radius = P.sr;
    if (!P.cmin.empty()) { T.cube_min = P.cmin; T.cube_max = P.cmax; }
    if (!P.m.empty()) { T.xf_matrix = P.m; T.xf_inverse = P.inv; }
    if (T.num_recs == 0) return;
    const pt::ShapeParams S{T.num_spheres, T.num_cubes, T.num_transformed, T.sphere_center.data(), T.sphere_radius.data(),
                            T.cube_min.data(), T.cube_max.data(), T.xf_matrix.data(), T.xf_inverse.data()};
    for (int64_t t = 0; t < T.num_transformed; t++)
        pt::shape_refit_xform(t, S, W.xforms.data(), W.ext.data(), T.xf_kind.data(), T.xf_index.data(), T.xf_inner_box.data(),
                              W.xbox.data(), nullptr);
    for (int64_t i = 0; i < T.num_recs; i++) pt::shape_refit_record(i, S, W.recs.data(), W.rec_box.data(), W.xbox.data());
    for (int64_t h = 0; h < T.num_heavy; h++) pt::shape_refit_heavy(h, T.num_recs, W.heavy.data(), W.rec_box.data());
    for (int64_t l = (int64_t)T.level_off.size() - 2; l >= 0; l--)
        for (uint32_t q = T.level_off[(size_t)l]; q < T.level_off[(size_t)l + 1]; q++)
            pt::shape_refit_node((int64_t)T.level_nodes[q], T.num_nodes, T.num_recs, W.nodes.data(), W.node_box.data(), W.rec_box.data());
    pt::shape_refit_lights(T, W.lights);
}
static Pose pose_of(const FixScene& s) {
    Pose P;
    P.sc = s.sc; P.sr = s.sr; P.cmin = s.cmin; P.cmax = s.cmax;
    for (const pt_transformed_shape& x : s.xf) {
        P.m.insert(P.m.end(), x.matrix, x.matrix + 16);
        P.inv.insert(P.inv.end(), x.inverse, x.inverse + 16);
    }
    return P;
}
static void pose_into(FixScene& s, const Pose& P) {   // the moved scene, for a fresh compile
    s.sc = P.sc; s.sr = P.sr; s.cmin = P.cmin; s.cmax = P.cmax;
    for (size_t i = 0; i < s.xf.size(); i++) {
        std::memcpy(s.xf[i].matrix, &P.m[16 * i], sizeof s.xf[i].matrix);
        std::memcpy(s.xf[i].inverse, &P.inv[16 * i], sizeof s.xf[i].inverse);
    }
    s.finish(0);
}

// ---- poses
static void mat_mul(const double* a, const double* b, double* o) {
    double r[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double v = 0;
            for (int k = 0; k < 4; k++) v += a[4 * i + k] * b[4 * k + j];
            r[4 * i + j] = v;
        }
    std::memcpy(o, r, sizeof r);
}
static void spin_matrices(double* m, double* inv) {   // a rotation about (1,1,1) by 0.7 rad, then a translation
    const double c = std::cos(0.7), s = std::sin(0.7), u = 1.0 / std::sqrt(3.0), t = 1 - c;
    const double R[9] = {c + u * u * t, u * u * t - u * s, u * u * t + u * s, u * u * t + u * s, c + u * u * t, u * u * t - u * s,
                         u * u * t - u * s, u * u * t + u * s, c + u * u * t};
    const double tr[3] = {0.5, 0.75, -0.25};
    for (int i = 0; i < 16; i++) m[i] = inv[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { m[4 * i + j] = R[3 * i + j]; inv[4 * i + j] = R[3 * j + i]; }
    for (int i = 0; i < 3; i++) {
        m[4 * i + 3] = tr[i];
        inv[4 * i + 3] = -(R[i] * tr[0] + R[3 + i] * tr[1] + R[6 + i] * tr[2]);
    }
}
static Pose make_pose(const FixScene& s, const std::string& name) {
    Pose P = pose_of(s);
    const size_t ns = P.sr.size(), nx = P.m.size() / 16;
    const float tr[3] = {1000.f, -2000.f, 3000.f};
    if (name == "translate") {
        for (size_t i = 0; i < P.sc.size(); i++) P.sc[i] += tr[i % 3];
        for (size_t i = 0; i < P.cmin.size(); i++) { P.cmin[i] += tr[i % 3]; P.cmax[i] += tr[i % 3]; }
        for (size_t i = 0; i < nx; i++)
            for (int k = 0; k < 3; k++) {
                P.m[16 * i + 4 * k + 3] += tr[k];
                double v = 0;   // inverse translation: -(R^-1 t')
                for (int j = 0; j < 3; j++) v += P.inv[16 * i + 4 * k + j] * P.m[16 * i + 4 * j + 3];
                P.inv[16 * i + 4 * k + 3] = -v;
            }
    } else if (name == "swap") {
        for (size_t i = 0; i < ns; i++)
            for (int k = 0; k < 3; k++) P.sc[3 * i + k] = s.sc[3 * (ns - 1 - i) + k];
    } else if (name == "point") {
        for (size_t i = 0; i < ns; i++) { P.sc[3 * i] = 0.5f; P.sc[3 * i + 1] = 1.5f; P.sc[3 * i + 2] = -0.5f; }
    } else if (name == "huge" || name == "tiny") {
        const double f = name == "huge" ? 1e6 : 1e-6;
        for (float& v : P.sc) v = (float)(v * f);
        for (double& v : P.sr) v *= f;
        for (float& v : P.cmin) v = (float)(v * f);
        for (float& v : P.cmax) v = (float)(v * f);
        for (size_t i = 0; i < nx; i++)
            for (int k = 0; k < 3; k++) {
                P.m[16 * i + 4 * k + 3] *= f;
                P.inv[16 * i + 4 * k + 3] *= f;
            }
    } else if (name == "lit") {   // the lights to the far side of the floor
        for (size_t i = 0; i < ns; i++)
            if (s.sm[i] == MAT_EMIT) { P.sc[3 * i + 1] = -P.sc[3 * i + 1] - 1.f; P.sr[i] *= 1.5; }
    } else if (name == "spin") {
        double sm[16], si[16];
        spin_matrices(sm, si);
        for (size_t i = 0; i < nx; i++) {
            mat_mul(sm, &P.m[16 * i], &P.m[16 * i]);        // spin after the shape's own transform
            mat_mul(&P.inv[16 * i], si, &P.inv[16 * i]);
        }
        if (nx == 0)
            for (size_t i = 0; i < ns; i++) P.sc[3 * i + 1] += 0.25f * (float)(i % 3);
    } else if (name == "shared") {   // the instances scene's shared inner sphere (index 0) moves and grows
        if (ns) { P.sc[0] += 0.5f; P.sc[1] -= 0.25f; P.sr[0] *= 1.75; }
    }
    return P;
}

// ---- checks
static bool words_equal(const void* a, const void* b, size_t bytes) { return bytes == 0 || std::memcmp(a, b, bytes) == 0; }
static void check_identity(const char* name, void (*build)(FixScene&)) {
    FixScene s;
    build(s);
    pt::HostScene H;
    std::string err;
    const int rc = pt::compile_scene(&s.d, pt::CompileOptions{}, H, err);
    CHECK(rc == PT_OK);
    if (rc != PT_OK) { std::fprintf(stderr, "%s: %s\n", name, err.c_str()); return; }
    Twin W;
    twin_of(H, W);
    const Twin W0 = W;
    twin_update(W, pose_of(s));
    const int before = failures;
    CHECK(W.nodes == W0.nodes);
    CHECK(W.recs == W0.recs);
    CHECK(W.ext == W0.ext);
    CHECK(W.heavy == W0.heavy);
    CHECK(W.rec_box == W0.rec_box);
    CHECK(words_equal(W.xforms.data(), W0.xforms.data(), W.xforms.size() * sizeof(pt::DevXform)));
    CHECK(words_equal(W.lights.data(), W0.lights.data(), W.lights.size() * sizeof(pt::DevLight)));
    // the level table: every node once, a child on a deeper level than its parent
    std::vector<int> level((size_t)W.T.num_nodes, -1);
    for (size_t l = 0; l + 1 < W.T.level_off.size(); l++)
        for (uint32_t q = W.T.level_off[l]; q < W.T.level_off[l + 1]; q++) {
            CHECK(W.T.level_nodes[q] < (uint32_t)W.T.num_nodes && level[W.T.level_nodes[q]] < 0);
            level[W.T.level_nodes[q]] = (int)l;
        }
    for (int64_t n = 0; n < W.T.num_nodes; n++) {
        CHECK(level[(size_t)n] >= 0);
        for (int k = 0; k < 4; k++) {
            const uint32_t ref = W.nodes[(size_t)n * 32 + 24 + (size_t)k];
            if (ref != pt::kEmpty4 && !(ref & 0x80000000u)) CHECK(level[ref] == level[(size_t)n] + 1);
        }
    }
    // the shape workspace (pt_update_layout.h) from a null base: parts 256-B aligned, disjoint, in the documented order,
    // inside `bytes`, each as large as what the refit indexes, counted from the scene and the compiled arrays
    const size_t ns = s.sr.size(), nc = s.cm.size(), nx = s.xf.size(), nn = W.nodes.size() / 32, nr = W.rec_box.size() / 6;
    const size_t f4 = sizeof(float), f8 = sizeof(double), i4 = sizeof(int32_t);
    const pt::ShapesDev D = pt::shapes_layout(H.shape_refit, nullptr);
    CHECK((size_t)H.shape_refit.num_nodes == nn && (size_t)H.shape_refit.num_recs == nr);
    CHECK(layout_violations({{D.sphere_center, ns * 3 * f4}, {D.sphere_radius, ns * f8}, {D.cube_min, nc * 3 * f4}, {D.cube_max, nc * 3 * f4},
                             {D.xf_matrix, nx * 16 * f8}, {D.xf_inverse, nx * 16 * f8}, {D.xbox, nx * 6 * f4}, {D.rec_box, nr * 6 * f4},
                             {D.node_box, nn * 6 * f4}, {D.level_nodes, nn * i4}, {D.xf_kind, nx * i4}, {D.xf_index, nx * i4},
                             {D.xf_inner_box, nx * 6 * f4}},
                            D.bytes) == 0);
    std::printf("identity %s nodes %lld recs %lld heavy %lld levels %zu lights %zu: %s\n", name, (long long)W.T.num_nodes,
                (long long)W.T.num_recs, (long long)W.T.num_heavy, W.T.level_off.size() - 1, W.lights.size(),
                failures == before ? "ok" : "FAILED");
}

// every slot box of node n contains the record boxes of its subtree; returns nothing, counts failures
static void contain(const Twin& W, uint32_t n, const float* plo, const float* phi, int depth) {
    CHECK(depth < 64);
    if (depth >= 64) return;
    const uint32_t* w = &W.nodes[(size_t)n * 32];
    for (int k = 0; k < 4; k++) {
        const uint32_t ref = w[24 + k];
        if (ref == pt::kEmpty4) continue;
        float lo[3], hi[3];
        for (int ax = 0; ax < 3; ax++) {
            std::memcpy(&lo[ax], &w[8 * ax + k], 4);
            std::memcpy(&hi[ax], &w[8 * ax + 4 + k], 4);
            if (plo) CHECK(lo[ax] >= plo[ax] && hi[ax] <= phi[ax]);
        }
        if (ref & 0x80000000u) {
            const uint32_t first = ref & 0x1FFFFFFFu, cnt = ((ref >> 29) & 3u) + 1;
            for (uint32_t t = 0; t < cnt; t++)
                for (int ax = 0; ax < 3; ax++)
                    CHECK(W.rec_box[6 * (size_t)(first + t) + ax] >= lo[ax] && W.rec_box[6 * (size_t)(first + t) + 3 + ax] <= hi[ax]);
        } else {
            contain(W, ref, lo, hi, depth + 1);
        }
    }
}
using Key = std::pair<uint32_t, uint32_t>;
static std::map<Key, size_t> rec_positions(const std::vector<uint32_t>& recs) {
    std::map<Key, size_t> m;
    for (size_t i = 0; i < recs.size() / 12; i++) m.emplace(Key{recs[12 * i + 3], recs[12 * i + 7]}, i);
    return m;
}
static void check_against_fresh(const Twin& W, void (*build)(FixScene&), const Pose& P) {
    FixScene f;
    build(f);
    pose_into(f, P);
    pt::HostScene F;
    std::string err;
    const int rc = pt::compile_scene(&f.d, pt::CompileOptions{}, F, err);
    CHECK(rc == PT_OK);
    if (rc != PT_OK) return;
    Twin G;
    twin_of(F, G);
    CHECK(G.recs.size() == W.recs.size() && G.heavy.size() == W.heavy.size());
    if (G.recs.size() != W.recs.size() || G.heavy.size() != W.heavy.size()) return;
    const std::map<Key, size_t> at = rec_positions(G.recs);
    for (size_t i = 0; i < W.recs.size() / 12; i++) {
        const auto it = at.find(Key{W.recs[12 * i + 3], W.recs[12 * i + 7]});
        CHECK(it != at.end());
        if (it == at.end()) continue;
        CHECK(words_equal(&W.recs[12 * i], &G.recs[12 * it->second], 48));
        CHECK(words_equal(&W.rec_box[6 * i], &G.T.rec_box[6 * it->second], 24));   // the fresh compile's ana_boxes box
    }
    for (size_t h = 0; h < W.heavy.size() / 8; h++) {
        const size_t i = W.heavy[8 * h + 3];
        const auto it = at.find(Key{W.recs[12 * i + 3], W.recs[12 * i + 7]});
        if (it == at.end()) continue;
        bool found = false;
        for (size_t g = 0; g < G.heavy.size() / 8 && !found; g++)
            if (G.heavy[8 * g + 3] == it->second) {
                found = true;
                CHECK(words_equal(&W.heavy[8 * h], &G.heavy[8 * g], 12) && words_equal(&W.heavy[8 * h + 4], &G.heavy[8 * g + 4], 16));
            }
        CHECK(found);
    }
    CHECK(W.ext == G.ext);
    CHECK(words_equal(W.xforms.data(), G.xforms.data(), W.xforms.size() * sizeof(pt::DevXform)));
    CHECK(W.lights.size() == G.lights.size());
    for (size_t i = 0; i < W.lights.size() && i < G.lights.size(); i++) {
        pt::DevLight a = W.lights[i], b = G.lights[i];
        a.index = b.index = 0;   // a record position: the fresh BVH orders its records anew
        CHECK(words_equal(&a, &b, sizeof a));
    }
}
static void check_poses(const char* name, void (*build)(FixScene&), std::initializer_list<const char*> poses) {
    FixScene s;
    build(s);
    pt::HostScene H;
    std::string err;
    if (pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) != PT_OK) { CHECK(false); return; }
    for (const char* pn : poses) {
        const int before = failures;
        Twin W;
        twin_of(H, W);
        const Twin W0 = W;
        const Pose P = make_pose(s, pn);
        twin_update(W, P);
        if (W.T.num_nodes) contain(W, 0, nullptr, nullptr, 0);
        check_against_fresh(W, build, P);
        CHECK(W.nodes != W0.nodes);
        for (size_t i = 0; i < W.nodes.size() / 32; i++)   // topology and padding words stay
            CHECK(words_equal(&W.nodes[32 * i + 24], &W0.nodes[32 * i + 24], 32));
        // the sequence: this pose after another one gives the same words
        Twin V;
        twin_of(H, V);
        twin_update(V, make_pose(s, "translate"));
        twin_update(V, P);
        CHECK(V.nodes == W.nodes && V.recs == W.recs && V.heavy == W.heavy && V.ext == W.ext);
        CHECK(words_equal(V.lights.data(), W.lights.data(), W.lights.size() * sizeof(pt::DevLight)));
        std::printf("pose %s %s %s\n", name, pn, failures == before ? "ok" : "FAILED");
    }
}
// only sphere_center given: the radii, cubes and matrices stay what an earlier update made them
static void check_partial() {
    const int before = failures;
    FixScene s;
    instances_scene(s);
    pt::HostScene H;
    std::string err;
    if (pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) != PT_OK) { CHECK(false); return; }
    Twin W, V;
    twin_of(H, W);
    twin_of(H, V);
    const Pose spin = make_pose(s, "spin"), moved = make_pose(s, "shared");
    twin_update(W, spin);
    Pose centres;
    centres.sc = moved.sc;
    twin_update(W, centres);
    Pose both = spin;
    both.sc = moved.sc;
    twin_update(V, both);
    CHECK(V.nodes == W.nodes && V.recs == W.recs && V.ext == W.ext && V.heavy == W.heavy);
    CHECK(W.T.sphere_radius == spin.sr);
    std::printf("partial %s\n", failures == before ? "ok" : "FAILED");
}
// NaN and infinite parameters: the boxes are unspecified, the walk stays inside its arrays (ASan is the witness)
static void check_nonfinite() {
    for (auto build : {beads_scene, routed_scene, instances_scene}) {
        FixScene s;
        build(s);
        pt::HostScene H;
        std::string err;
        if (pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) != PT_OK) { CHECK(false); return; }
        Twin W;
        twin_of(H, W);
        Pose P = pose_of(s);
        const float bad[4] = {NAN, INFINITY, -INFINITY, 3.0e38f};
        for (size_t i = 0; i < P.sc.size(); i++) if (i % 5 == 0) P.sc[i] = bad[i % 4];
        for (size_t i = 0; i < P.sr.size(); i++) if (i % 3 == 0) P.sr[i] = (double)bad[i % 4];
        for (size_t i = 0; i < P.cmin.size(); i++) if (i % 2 == 0) P.cmin[i] = bad[i % 4];
        for (size_t i = 0; i < P.m.size(); i++) if (i % 7 == 0) P.m[i] = (double)bad[i % 4];
        twin_update(W, P);
        for (size_t i = 0; i < W.nodes.size() / 32; i++) CHECK(words_equal(&W.nodes[32 * i + 24], (const uint32_t*)H.lines.data() + 32 * i + 24, 32));
    }
    std::printf("nonfinite ok\n");
}

template <class T>
static void dump(const std::string& dir, const char* name, const std::vector<T>& v) {
    FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
    if (!f) { CHECK(false); return; }
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
    std::fclose(f);
}
static std::vector<double> light_rows(const std::vector<pt::DevLight>& L) {
    std::vector<double> r;
    for (const pt::DevLight& l : L) { r.push_back(l.center[0]); r.push_back(l.center[1]); r.push_back(l.center[2]); r.push_back(l.radius); }
    return r;
}
static void dump_pose(const std::string& root, const char* scene, void (*build)(FixScene&)) {
    const std::string dir = root + "/" + scene;
    FixScene s;
    build(s);
    pt::HostScene H;
    std::string err;
    if (pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) != PT_OK) { CHECK(false); return; }
    Twin W;
    twin_of(H, W);
    dump(dir, "nodes0.u32", W.nodes); dump(dir, "recs0.u32", W.recs); dump(dir, "heavy0.u32", W.heavy);
    dump(dir, "lights0.f64", light_rows(W.lights));
    dump(dir, "rec_box0.f32", W.T.rec_box);
    dump(dir, "xf_kind.i32", W.T.xf_kind); dump(dir, "xf_index.i32", W.T.xf_index); dump(dir, "xf_inner_box.f32", W.T.xf_inner_box);
    dump(dir, "light_kind.i32", W.T.light_kind); dump(dir, "light_index.i32", W.T.light_index);
    Pose P = make_pose(s, "spin");
    const Pose lit = make_pose(s, "lit"), tr = make_pose(s, "tiny");
    P.sc = lit.sc; P.sr = lit.sr; P.cmin = tr.cmin; P.cmax = tr.cmax;
    twin_update(W, P);
    dump(dir, "sphere_center.f32", P.sc); dump(dir, "sphere_radius.f64", P.sr);
    dump(dir, "cube_min.f32", P.cmin); dump(dir, "cube_max.f32", P.cmax);
    dump(dir, "xf_matrix.f64", P.m); dump(dir, "xf_inverse.f64", P.inv);
    dump(dir, "nodes1.u32", W.nodes); dump(dir, "recs1.u32", W.recs); dump(dir, "heavy1.u32", W.heavy);
    dump(dir, "lights1.f64", light_rows(W.lights));
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "--dump") {
        dump_pose(argv[2], "routed", routed_scene);      // the caller makes the two directories
        dump_pose(argv[2], "instances", instances_scene);
        return failures ? 1 : 0;
    }
    check_identity("beads", beads_scene);
    check_identity("few", few_scene);
    check_identity("routed", routed_scene);
    check_identity("instances", instances_scene);
    check_identity("one", one_scene);
    check_identity("none", none_scene);
    check_poses("beads", beads_scene, {"translate", "swap", "point", "huge", "tiny", "lit"});
    check_poses("few", few_scene, {"translate", "lit", "huge", "tiny"});
    check_poses("routed", routed_scene, {"translate", "spin", "lit", "huge", "tiny"});
    check_poses("instances", instances_scene, {"translate", "swap", "point", "spin", "shared", "huge", "tiny"});
    check_poses("one", one_scene, {"translate", "lit", "huge", "tiny"});
    check_partial();
    check_nonfinite();
    {   // a scene without analytic shape: an update changes nothing
        FixScene s;
        none_scene(s);
        pt::HostScene H;
        std::string err;
        CHECK(pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) == PT_OK);
        Twin W;
        twin_of(H, W);
        twin_update(W, pose_of(s));
        CHECK(W.nodes.empty() && W.recs.empty() && W.T.num_recs == 0 && W.T.level_off.size() == 1);
    }
    std::printf("shapes_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
