// blas_check.cpp — the arithmetic of pt_update_meshes for instanced meshes (ptsharp_amd/csrc/pt_blas_refit.h) on the
// host: a CPU twin of the BLAS refit (the shared functions driven tris, bounds, levels, then the shape refit's
// xforms, records, heavy, levels over the compile's tables, as the kernels are) on scenes built in C++, checked
// against the host builder:
//   identity      a refit with the vertices a scene was compiled from reproduces every word of the BLAS nodes, recs
//                 and shade, the analytic nodes, records and heavy records, the transforms and the lights (scenes
//                 routed: an 8-triangle instanced mesh; instances: no instanced mesh; two: a 1-triangle and a
//                 288-triangle mesh, each instanced twice under a rotation and a non-uniform scale, the larger one a
//                 top-level shape too; only: a scene whose only triangles are instanced);
//   poses         every BLAS slot box contains the triangle boxes of its subtree (by recursion); recs and shade per
//                 source triangle equal a fresh compile's of the moved scene; each mesh's inner box equals the fresh
//                 compile's as values (-0 == +0: the flat pose puts both zeros into the vertices); records, their
//                 padded world boxes, heavy boxes and transforms equal it bit for bit, the lights as values;
//   sequence      pose A then pose B gives the words of pose B alone;
//   tables        the level table lists every BLAS node once, parents on lower levels than their children;
//   layout        the BLAS workspace (pt_update_layout.h) of each scene: the bounds kernel's blocks cover every position
//                 once and never span two BLASes; parts 256-B aligned, disjoint, in the documented order, inside
//                 `bytes` and as large as what the kernels index;
//   non-finite    NaN and infinite vertices run through the refit (under ASan: no access leaves its array).
// `--dump DIR` writes the sine pose of the `two` scene with given normals, inputs and outputs, as raw arrays into DIR
// (tests/blas_refit_ref.py is checked against them).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../ptsharp_amd/csrc/pt_blas_refit.h"
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
static void grid_mesh(FixScene& s, int n, float size, float y, int mat = MAT_BLUE) {   // 2 n^2 triangles
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
            s.triangle(a, b, c, mat);
            s.triangle(b, e, c, mat);
        }
    s.mfirst.push_back(first);
    s.mcount.push_back(2 * n * n);
}
// shapes_check.cpp's routed scene: a 3200-triangle grid, a floor cube, a sphere light, an SDF torus, a transformed
// Volume, a transformed sphere and an instanced 8-triangle mesh
static void routed_scene(FixScene& s) {
    materials(s);
    grid_mesh(s, 40, 6.f, 1.f);
    grid_mesh(s, 2, 1.f, 0.f);
    s.shape(PT_SHAPE_MESH, 0);
    s.shape(PT_SHAPE_CUBE, s.cube(-8.f, -1.f, -8.f, 8.f, 0.f, 8.f, MAT_GREY));
    s.shape(PT_SHAPE_SPHERE, s.sphere(0.f, 6.f, 0.f, 0.75, MAT_EMIT));
    const int torus = s.node(PT_SDF_TORUS, {1, 0.25, 2, 2}, {});
    s.sdfs = {pt_sdf_shape{s.node(PT_SDF_UNION, {}, {torus}), MAT_GREY}};
    s.shape(PT_SHAPE_SDF, 0);
    s.win0 = {pt_volume_window{0.2, 0.5, MAT_GREY, 0}};
    const int vol = s.volume(3, 3, 3, s.vox0, s.win0, -1.f, 1.f);
    s.shape(PT_SHAPE_TRANSFORMED, s.transformed(PT_SHAPE_VOLUME, vol, 4, 0.5, 1));
    s.shape(PT_SHAPE_TRANSFORMED, s.transformed(PT_SHAPE_SPHERE, s.sphere(0.f, 0.f, 0.f, 0.5, MAT_BLUE), -3, 2, 2));
    s.shape(PT_SHAPE_TRANSFORMED, s.transformed(PT_SHAPE_MESH, 1, -2, 3, -3));
    s.finish(0);
}
// shapes_check.cpp's instances scene without its spheres: transformed cubes and spheres, a mesh, no instanced mesh
static void instances_scene(FixScene& s) {
    materials(s);
    grid_mesh(s, 5, 3.f, 0.5f);
    s.shape(PT_SHAPE_MESH, 0);
    s.shape(PT_SHAPE_CUBE, s.cube(-10.f, -1.f, -10.f, 10.f, 0.f, 10.f, MAT_GREY));
    for (int i = 0; i < 12; i++) {
        const double x = 0.9 * (i % 8) - 3.0, y = 1.0 + 0.5 * (i / 8), z = 0.7 * (i % 5) + 1.0;
        int t;
        if (i % 2) t = s.transformed(PT_SHAPE_SPHERE, s.sphere(0.f, 0.f, 0.f, 0.2, MAT_BLUE), x, y, z);
        else t = s.transformed(PT_SHAPE_CUBE, s.cube(-0.2f, -0.1f, -0.15f, 0.2f, 0.1f, 0.15f, i == 10 ? MAT_EMIT : MAT_GREY), x, y, z);
        s.shape(PT_SHAPE_TRANSFORMED, t);
    }
    s.finish(0);
}
// a rotation about (1,1,1) by `angle`, after a scale (sx, sy, sz), then a translation: m and its inverse
static void rot_scale(double* m, double* inv, double angle, double sx, double sy, double sz, double tx, double ty, double tz) {
    const double c = std::cos(angle), s = std::sin(angle), u = 1.0 / std::sqrt(3.0), t = 1 - c;
    const double R[9] = {c + u * u * t, u * u * t - u * s, u * u * t + u * s, u * u * t + u * s, c + u * u * t, u * u * t - u * s,
                         u * u * t - u * s, u * u * t + u * s, c + u * u * t};
    const double sc[3] = {sx, sy, sz}, tr[3] = {tx, ty, tz};
    for (int i = 0; i < 16; i++) m[i] = inv[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { m[4 * i + j] = R[3 * i + j] * sc[j]; inv[4 * i + j] = R[3 * j + i] / sc[i]; }
    for (int i = 0; i < 3; i++) {
        m[4 * i + 3] = tr[i];
        inv[4 * i + 3] = -(inv[4 * i] * tr[0] + inv[4 * i + 1] * tr[1] + inv[4 * i + 2] * tr[2]);
    }
}
static int instance(FixScene& s, int mesh, double angle, double sx, double sy, double sz, double tx, double ty, double tz) {
    const int t = s.transformed(PT_SHAPE_MESH, mesh, 0, 0, 0);
    rot_scale(s.xf[(size_t)t].matrix, s.xf[(size_t)t].inverse, angle, sx, sy, sz, tx, ty, tz);
    return t;
}
// two BLASes: an emissive 1-triangle mesh (the lone-leaf root) and a 288-triangle mesh, each instanced twice; the
// larger mesh is a top-level shape too
static void two_scene(FixScene& s) {
    materials(s);
    const float a[3] = {-0.5f, 0.f, -0.25f}, b[3] = {0.5f, 0.125f, 0.f}, c[3] = {0.f, 0.25f, 0.75f};
    s.triangle(a, b, c, MAT_EMIT);
    s.mfirst.push_back(0);
    s.mcount.push_back(1);
    grid_mesh(s, 12, 2.f, 0.75f);
    s.shape(PT_SHAPE_CUBE, s.cube(-8.f, -1.f, -8.f, 8.f, 0.f, 8.f, MAT_GREY));
    s.shape(PT_SHAPE_SPHERE, s.sphere(0.f, 7.f, 0.f, 0.75, MAT_EMIT));
    s.shape(PT_SHAPE_MESH, 1);
    s.shape(PT_SHAPE_TRANSFORMED, instance(s, 0, 0.4, 1.5, 0.75, 2.0, -3, 2.5, 1));
    s.shape(PT_SHAPE_TRANSFORMED, instance(s, 1, 0.7, 1.25, 0.5, 0.8, 3, 2, -1));
    s.shape(PT_SHAPE_TRANSFORMED, instance(s, 0, -1.1, 0.5, 2.0, 1.0, 1, 4, 3));
    s.shape(PT_SHAPE_TRANSFORMED, instance(s, 1, 2.1, 0.6, 1.5, 1.1, -2, 3.5, -3));
    s.finish(0);
}
// a scene whose only triangles are instanced: no world triangle BVH
static void only_scene(FixScene& s) {
    materials(s);
    grid_mesh(s, 3, 1.5f, 0.f);
    s.shape(PT_SHAPE_CUBE, s.cube(-8.f, -1.f, -8.f, 8.f, 0.f, 8.f, MAT_GREY));
    s.shape(PT_SHAPE_SPHERE, s.sphere(0.f, 6.f, 0.f, 0.75, MAT_EMIT));
    s.shape(PT_SHAPE_TRANSFORMED, instance(s, 0, 0.3, 1.0, 2.0, 1.0, 0.5, 2, 0.25));
    s.finish(0);
}

// ---- the CPU twin: the device state of a context and pt_update_meshes' BLAS part on it
struct Twin {
    std::vector<uint32_t> bnodes, brecs, bshade;     // the BLASes
    std::vector<uint32_t> nodes, recs, ext, heavy;   // the analytic BVH
    std::vector<pt::DevXform> xforms;
    std::vector<pt::DevLight> lights;
    pt::BlasRefitTables B;
    pt::ShapeRefitTables T;
    std::vector<float> tri_box, bnode_box, blas_box, xbox, rec_box, node_box;
};
static std::vector<uint32_t> words_of(const std::vector<float4>& v) {
    const uint32_t* p = (const uint32_t*)v.data();
    return std::vector<uint32_t>(p, p + v.size() * 4);
}
static void twin_of(const pt::HostScene& H, Twin& W) {
    W.bnodes = words_of(H.blas_nodes); W.brecs = words_of(H.blas_recs); W.bshade = words_of(H.blas_shade);
    const uint32_t* lines = (const uint32_t*)H.lines.data();
    W.nodes.assign(lines, lines + (size_t)H.S.tri_node_line0 * 32);
    W.recs = words_of(H.ana_recs); W.ext = words_of(H.ext_recs); W.heavy = words_of(H.heavy);
    W.xforms = H.xforms;
    W.lights = H.lights;
    W.B = H.blas_refit;
    W.T = H.shape_refit;
    W.tri_box.assign((size_t)W.B.num_tris * 6, 0.f);
    W.bnode_box.assign((size_t)W.B.num_nodes * 6, 0.f);
    W.blas_box.assign(W.B.num_blas() * 6, 0.f);
    W.xbox.assign((size_t)W.T.num_transformed * 6, 0.f);
    W.rec_box = W.T.rec_box;
    W.node_box.assign((size_t)W.T.num_nodes * 6, 0.f);
}
struct Verts {
    std::vector<float> v1, v2, v3, n1, n2, n3;   // n1 empty: the normals stay
};
constexpr int64_t kSpan = 7;   // positions per partial of the bounds fold (the kernel's blocks fold 2048)
static void twin_update(Twin& W, const Verts& V) {
    const pt::BlasRefitTables& B = W.B;
    pt::ShapeRefitTables& T = W.T;
    const float* n1 = V.n1.empty() ? nullptr : V.n1.data();
    const float* n2 = V.n1.empty() ? nullptr : V.n2.data();
    const float* n3 = V.n1.empty() ? nullptr : V.n3.data();
    const int64_t ntri = (int64_t)V.v1.size() / 3;
    for (int64_t pos = 0; pos < B.num_tris; pos++) {   // k_blas_tris
        const int64_t s = B.src_of_pos[(size_t)pos];
        if (s < 0 || s >= ntri) continue;
        pt::blas_refit_tri(pos, s, W.brecs.data(), W.bshade.data(), V.v1.data(), V.v2.data(), V.v3.data(), n1, n2, n3, W.tri_box.data());
    }
    for (size_t b = 0; b < B.num_blas(); b++) {   // k_blas_bounds, k_blas_bounds_fold: partials of kSpan positions, last first
        const int64_t r0 = B.desc[4 * b + 2], n = B.desc[4 * b + 3];
        std::vector<float> parts;
        for (int64_t at = 0; at < n; at += kSpan) {
            float box[6];
            pt::blas_bounds_empty(box);
            for (int64_t pos = std::min(n, at + kSpan) - 1; pos >= at; pos--) {
                const int64_t s = B.src_of_pos[(size_t)(r0 + pos)];
                if (s >= 0 && s < ntri) pt::blas_bounds_tri(s, V.v1.data(), V.v2.data(), V.v3.data(), box);
            }
            parts.insert(parts.end(), box, box + 6);
        }
        float box[6];
        pt::blas_bounds_empty(box);
        for (size_t p = parts.size() / 6; p-- > 0;) pt::blas_bounds_merge(box, &parts[6 * p]);
        pt::blas_bounds_finish(n, box);
        std::memcpy(&W.blas_box[6 * b], box, sizeof box);
    }
    for (size_t t = 0; t < B.xf_blas.size(); t++)   // k_blas_inner
        if (B.xf_blas[t] >= 0) std::memcpy(&T.xf_inner_box[6 * t], &W.blas_box[6 * (size_t)B.xf_blas[t]], 6 * sizeof(float));
    for (int64_t l = (int64_t)B.level_off.size() - 2; l >= 0; l--)   // k_blas_level
        for (uint32_t q = B.level_off[(size_t)l]; q < B.level_off[(size_t)l + 1]; q++) {
            const int32_t* d = &B.desc[4 * (size_t)B.level_blas[q]];
            pt::blas_refit_node((int64_t)B.level_nodes[q], pt::BlasDesc{d[0], d[1], d[2], d[3]}, B.num_nodes, B.num_tris,
                                W.bnodes.data(), W.bnode_box.data(), W.tri_box.data());
        }
    if (T.num_recs == 0) return;   // launch_shape_refit from the current parameters
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
static Verts verts_of(const FixScene& s, bool normals) {
    Verts V;
    V.v1 = s.v1; V.v2 = s.v2; V.v3 = s.v3;
    if (normals) { V.n1 = s.n1; V.n2 = s.n2; V.n3 = s.n3; }
    return V;
}
static void verts_into(FixScene& s, const Verts& V) {   // the moved scene, for a fresh compile
    s.v1 = V.v1; s.v2 = V.v2; s.v3 = V.v3;
    if (!V.n1.empty()) { s.n1 = V.n1; s.n2 = V.n2; s.n3 = V.n3; }
    s.finish(0);
}

// ---- poses
static Verts make_pose(const FixScene& s, const std::string& name) {
    Verts V = verts_of(s, false);
    const float tr[3] = {1000.f, -2000.f, 3000.f};
    size_t corner = 0;
    for (std::vector<float>* v : {&V.v1, &V.v2, &V.v3}) {
        for (size_t i = 0; i < v->size(); i += 3) {
            float* p = &(*v)[i];
            if (name == "translate") {
                for (int k = 0; k < 3; k++) p[k] += tr[k];
            } else if (name == "sine") {
                p[1] += 0.3f * std::sin(2.5f * p[0] + 0.5f) * std::cos(1.5f * p[2]);
                p[0] += 0.1f * std::cos(3.f * p[2]);
            } else if (name == "flat") {   // onto the plane y = 0, both zeros among the vertices
                p[1] = ((i / 3 + corner) % 2) ? -0.f : 0.f;
            } else if (name == "point") {
                p[0] = 0.5f; p[1] = 1.5f; p[2] = -0.5f;
            } else if (name == "huge" || name == "tiny") {
                const double f = name == "huge" ? 1e6 : 1e-6;
                for (int k = 0; k < 3; k++) p[k] = (float)(p[k] * f);
            }
        }
        corner++;
    }
    if (name == "sine") {   // with normals: given ones
        V.n1 = s.n1; V.n2 = s.n2; V.n3 = s.n3;
        for (size_t i = 0; i < V.n1.size(); i += 3) {
            const float a = 0.01f * (float)i;
            V.n1[i] = std::sin(a); V.n1[i + 1] = std::cos(a); V.n1[i + 2] = 0.f;
            V.n2[i] = 0.f; V.n2[i + 1] = std::cos(a); V.n2[i + 2] = std::sin(a);
            V.n3[i] = 0.6f; V.n3[i + 1] = 0.8f; V.n3[i + 2] = 0.001f * (float)i;
        }
    }
    return V;
}

// ---- checks
static bool words_equal(const void* a, const void* b, size_t bytes) { return bytes == 0 || std::memcmp(a, b, bytes) == 0; }
static bool floats_equal(const float* a, const float* b, size_t n) {   // as values: -0 == +0
    for (size_t i = 0; i < n; i++) if (!(a[i] == b[i])) return false;
    return true;
}
static bool lights_equal(const pt::DevLight& a, const pt::DevLight& b) {   // as values; the record position aside
    return a.center[0] == b.center[0] && a.center[1] == b.center[1] && a.center[2] == b.center[2] && a.radius == b.radius;
}
// the BLAS level table: every node once, a child on a deeper level than its parent; returns the deepest BLAS's levels
static size_t check_levels(const Twin& W) {
    const pt::BlasRefitTables& B = W.B;
    std::vector<int> level((size_t)B.num_nodes, -1);
    CHECK(B.level_blas.size() == B.level_nodes.size() && B.level_off.back() == B.level_nodes.size());
    for (size_t l = 0; l + 1 < B.level_off.size(); l++)
        for (uint32_t q = B.level_off[l]; q < B.level_off[l + 1]; q++) {
            const size_t b = (size_t)B.level_blas[q];
            CHECK(b < B.num_blas() && B.level_nodes[q] < (uint32_t)B.desc[4 * b + 1]);
            const size_t g = (size_t)B.desc[4 * b] + B.level_nodes[q];
            CHECK(level[g] < 0);
            level[g] = (int)l;
        }
    for (size_t b = 0; b < B.num_blas(); b++)
        for (int32_t n = 0; n < B.desc[4 * b + 1]; n++) {
            const size_t g = (size_t)B.desc[4 * b] + (size_t)n;
            CHECK(level[g] >= 0);
            for (int k = 0; k < 4; k++) {
                const uint32_t ref = W.bnodes[g * 32 + 24 + (size_t)k];
                if (ref != pt::kEmpty4 && !(ref & 0x80000000u)) CHECK(level[(size_t)B.desc[4 * b] + ref] == level[g] + 1);
            }
        }
    return B.level_off.size() - 1;
}
// The BLAS workspace (pt_update_layout.h) from a null base, for k_blas_bounds blocks of `span` positions (the kernels'
// is 2048, pt_blas_refit.hip kBlasSpan; a small one gives the fixtures' meshes several blocks): every position of every
// BLAS in exactly one block of its own BLAS, and every part as large as what the kernels index
// nb, nn, nt, nx: the BLASes, their nodes and triangle positions as the compiled arrays count them, and the scene's
// transformed shapes
static void check_layout(const pt::BlasRefitTables& T, size_t nb, size_t nn, size_t nt, size_t nx, int64_t span) {
    pt::BlasBlocks B;
    pt::blas_blocks(T, span, B);
    CHECK(T.num_blas() == nb && (size_t)T.num_nodes == nn && (size_t)T.num_tris == nt);
    size_t blocks = 0;
    CHECK(B.off.size() == nb + 1 && B.blas.size() == B.first.size());
    for (size_t b = 0; b < nb; b++) {
        const int64_t r0 = T.desc[4 * b + 2], n = T.desc[4 * b + 3];
        CHECK((size_t)B.off[b] == blocks);
        for (int64_t at = 0; at < n; at += span, blocks++) {
            if (blocks >= B.blas.size()) break;
            CHECK(B.blas[blocks] == (int32_t)b && B.first[blocks] == r0 + at);
        }
    }
    CHECK(blocks == B.blas.size() && (size_t)B.off[nb] == blocks);
    const pt::BlasDev D = pt::blas_layout(T, blocks, nullptr);
    const size_t i4 = sizeof(int32_t), box = 6 * sizeof(float);
    CHECK(D.num_blocks == blocks);
    CHECK(layout_violations({{D.desc, nb * 4 * i4}, {D.src_of_pos, nt * i4}, {D.level_nodes, nn * i4},
                             {D.level_blas, nn * i4}, {D.block_blas, blocks * i4}, {D.block_first, blocks * i4},
                             {D.blas_block_off, (nb + 1) * i4}, {D.xf_blas, nx * i4}, {D.tri_box, nt * box},
                             {D.node_box, nn * box}, {D.block_part, blocks * box}, {D.blas_box, nb * box}},
                            D.bytes) == 0);
}
static void check_identity(const char* name, void (*build)(FixScene&)) {
    FixScene s;
    build(s);
    pt::HostScene H;
    std::string err;
    const int rc = pt::compile_scene(&s.d, pt::CompileOptions{}, H, err);
    CHECK(rc == PT_OK);
    if (rc != PT_OK) { std::fprintf(stderr, "%s: %s\n", name, err.c_str()); return; }
    const int before = failures;
    for (const int64_t span : {2048, 100, 1})   // float4 rows: 8 per BLAS node, kBlasRecWords / 4 per triangle position
        check_layout(H.blas_refit, H.blas.size(), H.blas_nodes.size() / 8, H.blas_recs.size() / (pt::kBlasRecWords / 4), s.xf.size(), span);
    for (const bool normals : {false, true}) {
        Twin W;
        twin_of(H, W);
        const Twin W0 = W;
        twin_update(W, verts_of(s, normals));
        CHECK(W.bnodes == W0.bnodes);
        CHECK(W.brecs == W0.brecs);
        CHECK(W.bshade == W0.bshade);
        CHECK(W.nodes == W0.nodes);
        CHECK(W.recs == W0.recs);
        CHECK(W.ext == W0.ext);
        CHECK(W.heavy == W0.heavy);
        CHECK(W.rec_box == W0.rec_box);
        CHECK(floats_equal(W.T.xf_inner_box.data(), W0.T.xf_inner_box.data(), W.T.xf_inner_box.size()));
        CHECK(words_equal(W.xforms.data(), W0.xforms.data(), W.xforms.size() * sizeof(pt::DevXform)));
        CHECK(W.lights.size() == W0.lights.size());
        for (size_t i = 0; i < W.lights.size(); i++) CHECK(lights_equal(W.lights[i], W0.lights[i]) && W.lights[i].index == W0.lights[i].index);
    }
    Twin W;
    twin_of(H, W);
    const size_t levels = check_levels(W);
    std::printf("identity %s blases %zu nodes %lld tris %lld levels %zu chunks %lld lights %zu: %s\n", name, W.B.num_blas(),
                (long long)W.B.num_nodes, (long long)W.B.num_tris, levels, (long long)H.refit.num_chunks, W.lights.size(),
                failures == before ? "ok" : "FAILED");
}

// every slot box of node n of a BLAS contains the triangle boxes of its subtree
static void contain(const Twin& W, const int32_t* d, uint32_t n, const float* plo, const float* phi, int depth) {
    CHECK(depth < 64 && n < (uint32_t)d[1]);
    if (depth >= 64 || n >= (uint32_t)d[1]) return;
    const uint32_t* w = &W.bnodes[((size_t)d[0] + n) * 32];
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
            CHECK(first + cnt <= (uint32_t)d[3]);
            for (uint32_t t = 0; t < cnt && first + t < (uint32_t)d[3]; t++) {
                const float* tb = &W.tri_box[6 * ((size_t)d[2] + first + t)];
                for (int ax = 0; ax < 3; ax++) CHECK(tb[ax] >= lo[ax] && tb[3 + ax] <= hi[ax]);
            }
        } else {
            contain(W, d, ref, lo, hi, depth + 1);
        }
    }
}
using Key = std::pair<uint32_t, uint32_t>;
static void check_against_fresh(const Twin& W, void (*build)(FixScene&), const Verts& V) {
    FixScene f;
    build(f);
    verts_into(f, V);
    pt::HostScene F;
    std::string err;
    const int rc = pt::compile_scene(&f.d, pt::CompileOptions{}, F, err);
    CHECK(rc == PT_OK);
    if (rc != PT_OK) return;
    Twin G;
    twin_of(F, G);
    // BLAS recs and shade per source triangle (the fresh build orders its triangles anew)
    CHECK(G.B.src_of_pos.size() == W.B.src_of_pos.size() && G.B.num_blas() == W.B.num_blas());
    if (G.B.src_of_pos.size() != W.B.src_of_pos.size()) return;
    std::map<int32_t, size_t> at;
    for (size_t i = 0; i < G.B.src_of_pos.size(); i++) at.emplace(G.B.src_of_pos[i], i);
    for (size_t i = 0; i < W.B.src_of_pos.size(); i++) {
        const auto it = at.find(W.B.src_of_pos[i]);
        CHECK(it != at.end());
        if (it == at.end()) continue;
        CHECK(words_equal(&W.brecs[12 * i], &G.brecs[12 * it->second], 48));
        CHECK(words_equal(&W.bshade[12 * i], &G.bshade[12 * it->second], 48));
    }
    // the meshes' inner boxes as values, then everything the shape refit derives from them, bit for bit
    CHECK(W.T.xf_inner_box.size() == G.T.xf_inner_box.size());
    CHECK(floats_equal(W.T.xf_inner_box.data(), G.T.xf_inner_box.data(), std::min(W.T.xf_inner_box.size(), G.T.xf_inner_box.size())));
    CHECK(G.recs.size() == W.recs.size() && G.heavy.size() == W.heavy.size());
    if (G.recs.size() != W.recs.size() || G.heavy.size() != W.heavy.size()) return;
    std::map<Key, size_t> rat;
    for (size_t i = 0; i < G.recs.size() / 12; i++) rat.emplace(Key{G.recs[12 * i + 3], G.recs[12 * i + 7]}, i);
    for (size_t i = 0; i < W.recs.size() / 12; i++) {
        const auto it = rat.find(Key{W.recs[12 * i + 3], W.recs[12 * i + 7]});
        CHECK(it != rat.end());
        if (it == rat.end()) continue;
        CHECK(words_equal(&W.recs[12 * i], &G.recs[12 * it->second], 48));
        CHECK(words_equal(&W.rec_box[6 * i], &G.T.rec_box[6 * it->second], 24));   // a transformed shape's: its padded world box
    }
    for (size_t h = 0; h < W.heavy.size() / 8; h++) {
        const size_t i = W.heavy[8 * h + 3];
        const auto it = rat.find(Key{W.recs[12 * i + 3], W.recs[12 * i + 7]});
        if (it == rat.end()) continue;
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
    for (size_t i = 0; i < W.lights.size() && i < G.lights.size(); i++) CHECK(lights_equal(W.lights[i], G.lights[i]));
}
static void check_poses(const char* name, void (*build)(FixScene&)) {
    FixScene s;
    build(s);
    pt::HostScene H;
    std::string err;
    if (pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) != PT_OK) { CHECK(false); return; }
    for (const char* pn : {"translate", "sine", "flat", "point", "huge", "tiny"}) {
        const int before = failures;
        Twin W;
        twin_of(H, W);
        const Twin W0 = W;
        const Verts V = make_pose(s, pn);
        twin_update(W, V);
        for (size_t b = 0; b < W.B.num_blas(); b++)
            if (W.B.desc[4 * b + 1] > 0) contain(W, &W.B.desc[4 * b], 0, nullptr, nullptr, 0);
        check_against_fresh(W, build, V);
        if (W.B.num_blas()) CHECK(W.bnodes != W0.bnodes && W.brecs != W0.brecs);
        for (size_t i = 0; i < W.bnodes.size() / 32; i++)   // topology and padding words stay
            CHECK(words_equal(&W.bnodes[32 * i + 24], &W0.bnodes[32 * i + 24], 32));
        for (size_t i = 0; i < W.bshade.size() / 12; i++) CHECK(W.bshade[12 * i + 9] == W0.bshade[12 * i + 9]);   // the material
        if (V.n1.empty()) CHECK(W.bshade == W0.bshade);
        // the sequence: this pose after another one gives the same words
        Twin U;
        twin_of(H, U);
        twin_update(U, make_pose(s, "translate"));
        Verts again = V;
        if (again.n1.empty()) { again.n1 = s.n1; again.n2 = s.n2; again.n3 = s.n3; }
        twin_update(U, again);
        CHECK(U.bnodes == W.bnodes && U.brecs == W.brecs && U.bshade == W.bshade);
        CHECK(U.nodes == W.nodes && U.recs == W.recs && U.heavy == W.heavy && U.ext == W.ext);
        std::printf("pose %s %s %s\n", name, pn, failures == before ? "ok" : "FAILED");
    }
}
// NaN and infinite vertices: boxes and normals are unspecified, the walk stays inside its arrays (ASan is the witness)
static void check_nonfinite() {
    for (auto build : {routed_scene, two_scene, only_scene}) {
        FixScene s;
        build(s);
        pt::HostScene H;
        std::string err;
        if (pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) != PT_OK) { CHECK(false); return; }
        Twin W;
        twin_of(H, W);
        const Twin W0 = W;
        Verts V = verts_of(s, true);
        const float bad[4] = {NAN, INFINITY, -INFINITY, 3.0e38f};
        for (size_t i = 0; i < V.v1.size(); i++) if (i % 5 == 0) V.v1[i] = bad[i % 4];
        for (size_t i = 0; i < V.v2.size(); i++) if (i % 7 == 0) V.v2[i] = bad[i % 4];
        for (size_t i = 0; i < V.n3.size(); i++) if (i % 3 == 0) V.n3[i] = bad[i % 4];
        twin_update(W, V);
        for (size_t i = 0; i < W.bnodes.size() / 32; i++) CHECK(words_equal(&W.bnodes[32 * i + 24], &W0.bnodes[32 * i + 24], 32));
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
static void dump_pose(const std::string& dir) {
    FixScene s;
    two_scene(s);
    pt::HostScene H;
    std::string err;
    if (pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) != PT_OK) { CHECK(false); return; }
    Twin W;
    twin_of(H, W);
    dump(dir, "desc.i32", W.B.desc); dump(dir, "src_of_pos.i32", W.B.src_of_pos); dump(dir, "xf_blas.i32", W.B.xf_blas);
    dump(dir, "nodes0.u32", W.bnodes); dump(dir, "recs0.u32", W.brecs); dump(dir, "shade0.u32", W.bshade);
    dump(dir, "xf_inner_box0.f32", W.T.xf_inner_box);
    const Verts V = make_pose(s, "sine");
    twin_update(W, V);
    dump(dir, "v1.f32", V.v1); dump(dir, "v2.f32", V.v2); dump(dir, "v3.f32", V.v3);
    dump(dir, "n1.f32", V.n1); dump(dir, "n2.f32", V.n2); dump(dir, "n3.f32", V.n3);
    dump(dir, "nodes1.u32", W.bnodes); dump(dir, "recs1.u32", W.brecs); dump(dir, "shade1.u32", W.bshade);
    dump(dir, "boxes1.f32", W.blas_box); dump(dir, "xf_inner_box1.f32", W.T.xf_inner_box);
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "--dump") {
        dump_pose(argv[2]);
        return failures ? 1 : 0;
    }
    check_identity("routed", routed_scene);
    check_identity("instances", instances_scene);
    check_identity("two", two_scene);
    check_identity("only", only_scene);
    check_poses("routed", routed_scene);
    check_poses("instances", instances_scene);
    check_poses("two", two_scene);
    check_poses("only", only_scene);
    check_nonfinite();
    std::printf("blas_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
