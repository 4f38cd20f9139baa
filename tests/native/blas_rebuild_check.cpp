// blas_rebuild_check.cpp — the arithmetic of pt_rebuild_blas and pt_blas_cost (ptsharp_amd/csrc/pt_blas_rebuild.h) on
// the host: a CPU twin of the BLAS rebuild (the shared functions driven with std::stable_sort as the kernels drive
// them with the device sorts, then blas_check.cpp's refit steps over the new order) on scenes of two BLASes built in
// C++, checked against the host builder:
//   sizes         BLASes of n in {1, 4, 5, 16, 17, 64, 65, 288, 1025, 4097, 6400} triangles, two per scene (node_off and
//                 rec_off != 0), at the rest, sine, twist and per-triangle-offset poses;
//   tree          every triangle once; every slot box contains its subtree's triangle boxes (by recursion); the stack
//                 need <= 3 h; a child's index exceeds its parent's; empty slots as collapse_bvh4 writes them;
//   fresh         recs, shade (material word included) and uv per source triangle equal a fresh compile's of the moved
//                 scene; the meshes' inner boxes as values; records, world boxes, heavy boxes, transforms and lights as
//                 blas_check.cpp checks them;
//   fixed point   a second rebuild changes no word;
//   fallback      the table of n in 1 .. 400 whose balanced tree needs more nodes than the compile gave the BLAS (printed:
//                 DESIGN.md §4j quotes it; it is empty), and, with the capacity of one BLAS lowered by hand, that BLAS
//                 keeps words 24-31 of every node and its order while the other is rebuilt;
//   tables        the level table lists every node of every BLAS once, parents above children;
//   tail          blas_tail_table's workgroups cover every rebuilt position once, for every tail size;
//   cost          pt_blas_cost's arithmetic on the 6,400-triangle sphere at twist and offset: fresh F, refitted R,
//                 rebuilt M; M < R, and M <= (the measured M / F + 10 %) F;
//   non-finite    NaN and infinite vertices run through (under ASan: no access leaves its array), still a permutation.
// `--dump DIR` writes the twist pose of the (288, 65) scene with given normals, inputs and outputs, as raw arrays
// (tests/blas_rebuild_ref.py is checked against them).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../ptsharp_amd/csrc/pt_blas_rebuild.h"
#include "../../ptsharp_amd/csrc/pt_blas_refit.h"
#include "../../ptsharp_amd/csrc/pt_bvh.h"
#include "../../ptsharp_amd/csrc/pt_scene_compile.h"
#include "../../ptsharp_amd/csrc/pt_shape_refit.h"
#include "../../ptsharp_amd/csrc/pt_update_layout.h"
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
enum { MAT_GREY = 0, MAT_EMIT = 1, MAT_BLUE = 2, MAT_RED = 3 };
// the first n triangles of a wavy grid of side ceil(sqrt(n / 2)), materials alternating so that a misplaced material
// word shows
static void grid_mesh(FixScene& s, int n, float size, float y) {
    const int first = (int)s.tm.size();
    int side = 1;
    while (2 * side * side < n) side++;
    int made = 0;
    for (int j = 0; j < side && made < n; j++)
        for (int i = 0; i < side && made < n; i++) {
            auto vtx = [&](int a, int b, float* p) {
                p[0] = size * ((float)a / (float)side - 0.5f);
                p[2] = size * ((float)b / (float)side - 0.5f);
                p[1] = y + 0.1f * std::sin(3.f * p[0]) * std::cos(2.f * p[2]);
            };
            float a[3], b[3], c[3], e[3];
            vtx(i, j, a); vtx(i + 1, j, b); vtx(i, j + 1, c); vtx(i + 1, j + 1, e);
            s.triangle(a, b, c, made % 3 ? MAT_BLUE : MAT_RED);
            if (++made < n) { s.triangle(b, e, c, made % 3 ? MAT_BLUE : MAT_RED); made++; }
        }
    s.mfirst.push_back(first);
    s.mcount.push_back(n);
}
// a latitude-longitude sphere of 2 * slices * stacks triangles (80 x 40: 6,400)
static void sphere_mesh(FixScene& s, int slices, int stacks, float radius) {
    const int first = (int)s.tm.size();
    auto vtx = [&](int i, int j, float* p) {
        const float th = 3.14159265f * (float)j / (float)stacks, ph = 6.2831853f * (float)i / (float)slices;
        p[0] = radius * std::sin(th) * std::cos(ph);
        p[1] = radius * std::cos(th);
        p[2] = radius * std::sin(th) * std::sin(ph);
    };
    for (int j = 0; j < stacks; j++)
        for (int i = 0; i < slices; i++) {
            float a[3], b[3], c[3], e[3];
            vtx(i, j, a); vtx(i + 1, j, b); vtx(i, j + 1, c); vtx(i + 1, j + 1, e);
            s.triangle(a, b, c, (i + j) % 3 ? MAT_BLUE : MAT_RED);
            s.triangle(b, e, c, (i + j) % 3 ? MAT_BLUE : MAT_RED);
        }
    s.mfirst.push_back(first);
    s.mcount.push_back(2 * slices * stacks);
}
static void add_mesh(FixScene& s, int n) {
    if (n == 6400) sphere_mesh(s, 80, 40, 1.f);
    else grid_mesh(s, n, 2.f, 0.75f);
}
// two BLASes of na and nb triangles, each instanced under a translation, a floor and a light
static int g_na = 288, g_nb = 65;
static void pair_scene(FixScene& s) {
    s.material(0.9, 0.9, 0.9, 0);
    s.material(1, 1, 1, 10);
    s.material(0.2, 0.3, 0.8, 0);
    s.material(0.8, 0.3, 0.2, 0);
    add_mesh(s, g_na);
    add_mesh(s, g_nb);
    s.shape(PT_SHAPE_CUBE, s.cube(-8.f, -1.f, -8.f, 8.f, 0.f, 8.f, MAT_GREY));
    s.shape(PT_SHAPE_SPHERE, s.sphere(0.f, 7.f, 0.f, 0.75, MAT_EMIT));
    s.shape(PT_SHAPE_TRANSFORMED, s.transformed(PT_SHAPE_MESH, 0, -3, 2.5, 1));
    s.shape(PT_SHAPE_TRANSFORMED, s.transformed(PT_SHAPE_MESH, 1, 3, 2, -1));
    s.shape(PT_SHAPE_TRANSFORMED, s.transformed(PT_SHAPE_MESH, 0, 1, 4, 3));
    s.finish(0);
}

// ---- the CPU twin: the device state of a context, pt_rebuild_blas' BLAS part and pt_update_meshes' on it
struct Twin {
    std::vector<uint32_t> bnodes, brecs, bshade, buv;   // the BLASes
    std::vector<uint32_t> nodes, recs, ext, heavy;      // the analytic BVH
    std::vector<pt::DevXform> xforms;
    std::vector<pt::DevLight> lights;
    pt::BlasRefitTables B;
    pt::ShapeRefitTables T;
    std::vector<int32_t> node_cap, items;
    std::vector<float> tri_box, bnode_box, blas_box, xbox, rec_box, node_box;
};
static std::vector<uint32_t> words_of(const std::vector<float4>& v) {
    const uint32_t* p = (const uint32_t*)v.data();
    return std::vector<uint32_t>(p, p + v.size() * 4);
}
static void twin_of(const pt::HostScene& H, Twin& W) {
    W.bnodes = words_of(H.blas_nodes); W.brecs = words_of(H.blas_recs); W.bshade = words_of(H.blas_shade); W.buv = words_of(H.blas_uv);
    const uint32_t* lines = (const uint32_t*)H.lines.data();
    W.nodes.assign(lines, lines + (size_t)H.S.tri_node_line0 * 32);
    W.recs = words_of(H.ana_recs); W.ext = words_of(H.ext_recs); W.heavy = words_of(H.heavy);
    W.xforms = H.xforms;
    W.lights = H.lights;
    W.B = H.blas_refit;
    W.T = H.shape_refit;
    for (const pt::DevBlas& b : H.blas) W.node_cap.push_back(b.num_nodes);
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
// blas_check.cpp's twin_update: tris, bounds, inner boxes, levels, then the shape refit
static void twin_update(Twin& W, const Verts& V) {
    const pt::BlasRefitTables& B = W.B;
    pt::ShapeRefitTables& T = W.T;
    const float* n1 = V.n1.empty() ? nullptr : V.n1.data();
    const float* n2 = V.n1.empty() ? nullptr : V.n2.data();
    const float* n3 = V.n1.empty() ? nullptr : V.n3.data();
    const int64_t ntri = (int64_t)V.v1.size() / 3;
    for (int64_t pos = 0; pos < B.num_tris; pos++) {
        const int64_t s = B.src_of_pos[(size_t)pos];
        if (s < 0 || s >= ntri) continue;
        pt::blas_refit_tri(pos, s, W.brecs.data(), W.bshade.data(), V.v1.data(), V.v2.data(), V.v3.data(), n1, n2, n3, W.tri_box.data());
    }
    for (size_t b = 0; b < B.num_blas(); b++) {
        const int64_t r0 = B.desc[4 * b + 2], n = B.desc[4 * b + 3];
        float box[6];
        pt::blas_bounds_empty(box);
        for (int64_t pos = 0; pos < n; pos++) {
            const int64_t s = B.src_of_pos[(size_t)(r0 + pos)];
            if (s >= 0 && s < ntri) pt::blas_bounds_tri(s, V.v1.data(), V.v2.data(), V.v3.data(), box);
        }
        pt::blas_bounds_finish(n, box);
        std::memcpy(&W.blas_box[6 * b], box, sizeof box);
    }
    for (size_t t = 0; t < B.xf_blas.size(); t++)
        if (B.xf_blas[t] >= 0) std::memcpy(&T.xf_inner_box[6 * t], &W.blas_box[6 * (size_t)B.xf_blas[t]], 6 * sizeof(float));
    for (int64_t l = (int64_t)B.level_off.size() - 2; l >= 0; l--)
        for (uint32_t q = B.level_off[(size_t)l]; q < B.level_off[(size_t)l + 1]; q++) {
            const int32_t* d = &B.desc[4 * (size_t)B.level_blas[q]];
            pt::blas_refit_node((int64_t)B.level_nodes[q], pt::BlasDesc{d[0], d[1], d[2], d[3]}, B.num_nodes, B.num_tris,
                                W.bnodes.data(), W.bnode_box.data(), W.tri_box.data());
        }
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
// pt_rebuild_blas' re-sort: the plans, the order by std::stable_sort, the permutation of what the refit does not
// rewrite, the topology, the tables; then the refit
static void twin_rebuild(Twin& W, const Verts& V) {
    pt::BlasRefitTables& B = W.B;
    size_t refused = 0;
    CHECK(pt::blas_rebuild_items(B, W.node_cap, W.items, &refused));
    const size_t P = (size_t)B.num_tris;
    std::vector<uint32_t> keys3(3 * P), vals(P);
    for (size_t p = 0; p < P; p++) {   // the keys
        const size_t s = (size_t)B.src_of_pos[p];
        pt::rebuild_keys(&V.v1[3 * s], &V.v2[3 * s], &V.v3[3 * s], &keys3[3 * p]);
        vals[p] = (uint32_t)p;
    }
    for (size_t b = 0; b < B.num_blas(); b++) {   // the rounds
        const int64_t r0 = W.items[4 * b], n = W.items[4 * b + 1];
        const int h = W.items[4 * b + 2];
        for (int s = 2 * h; s >= 1; s--)
            for (int64_t f = 0; f < n; f += (int64_t)4 << s) {
                if (!pt::blas_rebuild_segment_sorted(f, s, n)) continue;
                const int64_t end = std::min(n, f + ((int64_t)4 << s));
                uint32_t bd[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
                for (int64_t q = f; q < end; q++)
                    for (int a = 0; a < 3; a++) {
                        const uint32_t k = keys3[3 * (size_t)vals[(size_t)(r0 + q)] + (size_t)a];
                        bd[a] = std::min(bd[a], k);
                        bd[3 + a] = std::max(bd[3 + a], k);
                    }
                const int ax = pt::rebuild_axis(bd);
                std::stable_sort(vals.begin() + (ptrdiff_t)(r0 + f), vals.begin() + (ptrdiff_t)(r0 + end),
                                 [&](uint32_t x, uint32_t y) { return keys3[3 * (size_t)x + (size_t)ax] < keys3[3 * (size_t)y + (size_t)ax]; });
            }
    }
    {   // the permutation: shade, uv, src_of_pos
        const std::vector<uint32_t> shade = W.bshade, uv = W.buv;
        const std::vector<int32_t> src = B.src_of_pos;
        for (size_t p = 0; p < P; p++) {
            const size_t t = vals[p];
            std::memcpy(&W.bshade[12 * p], &shade[12 * t], 48);
            std::memcpy(&W.buv[8 * p], &uv[8 * t], 32);
            B.src_of_pos[p] = src[t];
        }
    }
    for (size_t b = 0; b < B.num_blas(); b++) {   // the topology
        if (W.items[4 * b + 2] <= 0) continue;
        pt::BlasPlan R;
        CHECK(pt::blas_rebuild_plan(W.items[4 * b + 1], R));
        for (int64_t i = 0; i < R.num_nodes; i++) pt::blas_rebuild_node_write(R, i, &W.bnodes[((size_t)W.items[4 * b + 3] + (size_t)i) * 32]);
    }
    pt::blas_rebuild_tables(B, W.items);
    twin_update(W, V);
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
    for (std::vector<float>* v : {&V.v1, &V.v2, &V.v3})
        for (size_t i = 0; i < v->size(); i += 3) {
            float* p = &(*v)[i];
            if (name == "sine") {
                p[1] += 0.3f * std::sin(2.5f * p[0] + 0.5f) * std::cos(1.5f * p[2]);
                p[0] += 0.1f * std::cos(3.f * p[2]);
            } else if (name == "twist") {   // turned about y by an angle that grows with the height and the radius
                const float ang = 2.5f * p[1] + 1.5f * std::sqrt(p[0] * p[0] + p[2] * p[2]);
                const float c = std::cos(ang), sn = std::sin(ang), x = p[0], z = p[2];
                p[0] = c * x - sn * z;
                p[2] = sn * x + c * z;
            } else if (name == "offset") {   // every triangle moved as a whole by its own vector
                uint32_t hsh = (uint32_t)(i / 3) * 2654435761u;
                for (int k = 0; k < 3; k++) {
                    hsh = hsh * 1664525u + 1013904223u;
                    p[k] += 1.5f * ((float)(hsh >> 8) * (1.0f / 16777216.0f) - 0.5f);
                }
            }
        }
    if (name == "twist") {   // with given normals
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
static bool lights_equal(const pt::DevLight& a, const pt::DevLight& b) {
    return a.center[0] == b.center[0] && a.center[1] == b.center[1] && a.center[2] == b.center[2] && a.radius == b.radius;
}
// every slot box of node n of a BLAS contains the triangle boxes of its subtree; every triangle is reached once; a
// child's index exceeds its parent's; the pushes along every path stay within `budget`
static void walk(const Twin& W, const int32_t* d, uint32_t n, const float* plo, const float* phi, int pushed, int budget,
                 std::vector<int>& seen) {
    CHECK(n < (uint32_t)d[1]);
    if (n >= (uint32_t)d[1]) return;
    const uint32_t* w = &W.bnodes[((size_t)d[0] + n) * 32];
    int children = 0;
    for (int k = 0; k < 4; k++) children += w[24 + k] != pt::kEmpty4;
    CHECK(children >= 1 && w[24] != pt::kEmpty4);
    const int here = pushed + children - 1;
    CHECK(here <= budget);
    for (int k = 0; k < 4; k++) {
        const uint32_t ref = w[24 + k];
        if (ref == pt::kEmpty4) {
            for (int ax = 0; ax < 3; ax++) CHECK(w[8 * ax + k] == 0u && w[8 * ax + 4 + k] == 0u);
            continue;
        }
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
                seen[(size_t)d[2] + first + t]++;
                const float* tb = &W.tri_box[6 * ((size_t)d[2] + first + t)];
                for (int ax = 0; ax < 3; ax++) CHECK(tb[ax] >= lo[ax] && tb[3 + ax] <= hi[ax]);
            }
        } else {
            CHECK(ref > n);
            if (ref > n) walk(W, d, ref, lo, hi, here, budget, seen);
        }
    }
    for (int k = 28; k < 32; k++) CHECK(w[k] == 0u);
}
static void check_tree(const Twin& W) {
    std::vector<int> seen((size_t)W.B.num_tris, 0);
    for (size_t b = 0; b < W.B.num_blas(); b++) {
        const int h = W.items.empty() ? 0 : W.items[4 * b + 2];
        if (W.B.desc[4 * b + 1] > 0) walk(W, &W.B.desc[4 * b], 0, nullptr, nullptr, 0, h > 0 ? 3 * h : pt::kStack4Budget, seen);
    }
    for (int c : seen) CHECK(c == 1);
    std::vector<int32_t> src = W.B.src_of_pos;   // a permutation of every BLAS's source triangles
    for (size_t b = 0; b < W.B.num_blas(); b++) {
        const auto first = src.begin() + W.B.desc[4 * b + 2], last = first + W.B.desc[4 * b + 3];
        std::sort(first, last);
        CHECK(std::adjacent_find(first, last) == last);
    }
}
static void check_levels(const Twin& W) {
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
}
using Key = std::pair<uint32_t, uint32_t>;
static bool compile_moved(void (*build)(FixScene&), const Verts& V, pt::HostScene& F) {
    FixScene f;
    build(f);
    verts_into(f, V);
    std::string err;
    const int rc = pt::compile_scene(&f.d, pt::CompileOptions{}, F, err);
    CHECK(rc == PT_OK);
    return rc == PT_OK;
}
static void check_against_fresh(const Twin& W, const Twin& G) {
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
        CHECK(words_equal(&W.buv[8 * i], &G.buv[8 * it->second], 32));
    }
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
        CHECK(words_equal(&W.rec_box[6 * i], &G.T.rec_box[6 * it->second], 24));
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
// pt_blas_cost's arithmetic for BLAS b of a twin: {inner, leaf, area}
static void cost_of(const Twin& W, size_t b, double out[3]) {
    const int64_t n0 = W.B.desc[4 * b], nn = W.B.desc[4 * b + 1];
    double si = 0.0, sl = 0.0, area = 0.0;
    for (int64_t i = 0; i < nn; i++) {
        double a, c, own;
        pt::blas_node_cost(&W.bnodes[(size_t)(n0 + i) * 32], &a, &c, &own);
        si += a;
        sl += c;
        if (i == 0) area = own;
    }
    pt::blas_cost_finish(si, sl, area, out);
}
static void check_tail_tables(const Twin& W) {
    for (const int64_t T : {64, 256, 1024}) {
        std::vector<int32_t> tail;
        pt::blas_tail_table(W.items.data(), (int64_t)W.B.num_blas(), T, tail);
        std::vector<int> covered((size_t)W.B.num_tris, 0);
        CHECK((int64_t)tail.size() / 4 <= W.B.num_tris / 64 + (int64_t)W.B.num_blas() + 1);
        for (size_t i = 0; i + 3 < tail.size(); i += 4) {
            CHECK(tail[i + 2] >= 1 && tail[i + 2] <= 8 && tail[i + 1] >= 1 && tail[i + 1] <= (4 << tail[i + 2]) && (4 << tail[i + 2]) <= T);
            for (int32_t q = 0; q < tail[i + 1]; q++) covered[(size_t)(tail[i] + q)]++;
        }
        for (size_t b = 0; b < W.B.num_blas(); b++)
            for (int32_t q = 0; q < W.items[4 * b + 1]; q++) CHECK(covered[(size_t)(W.items[4 * b] + q)] == (W.items[4 * b + 2] > 0 ? 1 : 0));
    }
}

static const char* kPoses[] = {"rest", "sine", "twist", "offset"};
static void check_pair(int na, int nb) {
    g_na = na; g_nb = nb;
    FixScene s;
    pair_scene(s);
    pt::HostScene H;
    std::string err;
    if (pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) != PT_OK) { CHECK(false); std::fprintf(stderr, "%s\n", err.c_str()); return; }
    for (const char* pn : kPoses) {
        const int before = failures;
        Twin W;
        twin_of(H, W);
        const Twin W0 = W;
        CHECK(W.B.num_blas() == 2 && W.B.desc[4] != 0 && W.B.desc[6] != 0);
        const Verts V = make_pose(s, pn);
        twin_rebuild(W, V);
        check_tree(W);
        check_levels(W);
        check_tail_tables(W);
        pt::HostScene F;
        if (compile_moved(pair_scene, V, F)) {
            Twin G;
            twin_of(F, G);
            check_against_fresh(W, G);
        }
        int kept = 0;
        for (size_t b = 0; b < 2; b++) {
            const int32_t* d0 = &W0.B.desc[4 * b];
            pt::BlasPlan R;
            pt::blas_rebuild_plan(d0[3], R);
            if (W.items[4 * b + 2] > 0) {
                CHECK(W.B.desc[4 * b + 1] == R.num_nodes && R.num_nodes <= d0[1]);
                for (int64_t i = R.num_nodes; i < d0[1]; i++)   // lines past the new count are left as they are
                    CHECK(words_equal(&W.bnodes[(size_t)(d0[0] + i) * 32], &W0.bnodes[(size_t)(d0[0] + i) * 32], 128));
            } else {   // the fallback: topology and order as they were
                kept++;
                CHECK(R.num_nodes > d0[1] && W.B.desc[4 * b + 1] == d0[1]);
                for (int32_t i = 0; i < d0[1]; i++)
                    CHECK(words_equal(&W.bnodes[(size_t)(d0[0] + i) * 32 + 24], &W0.bnodes[(size_t)(d0[0] + i) * 32 + 24], 32));
                CHECK(words_equal(&W.B.src_of_pos[(size_t)d0[2]], &W0.B.src_of_pos[(size_t)d0[2]], (size_t)d0[3] * 4));
            }
        }
        // a second rebuild is a fixed point
        Twin U = W;
        twin_rebuild(U, V);
        CHECK(U.bnodes == W.bnodes && U.brecs == W.brecs && U.bshade == W.bshade && U.buv == W.buv && U.B.src_of_pos == W.B.src_of_pos);
        CHECK(U.B.desc == W.B.desc && U.B.level_nodes == W.B.level_nodes && U.B.level_off == W.B.level_off && U.nodes == W.nodes);
        // and a refit of the rebuilt topology with the same arrays too
        Twin R2 = W;
        twin_update(R2, V);
        CHECK(R2.bnodes == W.bnodes && R2.brecs == W.brecs && R2.bshade == W.bshade);
        std::printf("pair %d %d %s nodes %d->%d %d->%d kept %d: %s\n", na, nb, pn, W0.B.desc[1], W.B.desc[1], W0.B.desc[5], W.B.desc[5],
                    kept, failures == before ? "ok" : "FAILED");
    }
}

// a BLAS that cannot hold its balanced tree (its capacity lowered by hand: no compile gives one) is refitted, the other
// rebuilt, and the scene still equals the fresh compile's
static void check_forced_fallback() {
    g_na = 288; g_nb = 65;
    FixScene s;
    pair_scene(s);
    pt::HostScene H;
    std::string err;
    if (pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) != PT_OK) { CHECK(false); return; }
    Twin W;
    twin_of(H, W);
    const Twin W0 = W;
    W.node_cap[0] = 25;   // the plan of 288 triangles has 26 nodes
    const Verts V = make_pose(s, "twist");
    twin_rebuild(W, V);
    CHECK(W.items[2] == 0 && W.items[6] > 0);
    CHECK(W.B.desc[1] == W0.B.desc[1] && W.B.desc[5] < W0.B.desc[5]);
    for (int32_t i = 0; i < W0.B.desc[1]; i++) CHECK(words_equal(&W.bnodes[(size_t)i * 32 + 24], &W0.bnodes[(size_t)i * 32 + 24], 32));
    CHECK(words_equal(W.B.src_of_pos.data(), W0.B.src_of_pos.data(), 288 * 4));
    check_tree(W);
    check_levels(W);
    check_tail_tables(W);
    pt::HostScene F;
    if (compile_moved(pair_scene, V, F)) {
        Twin G;
        twin_of(F, G);
        check_against_fresh(W, G);
    }
    std::printf("forced fallback ok\n");
}

// which n in 1 .. 400 fall back: build_bvh + collapse_bvh4 over the first n triangles of the wavy grid at rest, against
// the plan's node count
static void fallback_table() {
    std::printf("fallback n:");
    int count = 0;
    for (int n = 1; n <= 400; n++) {
        FixScene s;
        s.material(0.9, 0.9, 0.9, 0); s.material(1, 1, 1, 10); s.material(0.2, 0.3, 0.8, 0); s.material(0.8, 0.3, 0.2, 0);
        grid_mesh(s, n, 2.f, 0.75f);
        std::vector<float> lo((size_t)n * 3), hi((size_t)n * 3);
        for (int t = 0; t < n; t++) pt::refit_tri_box(&s.v1[3 * (size_t)t], &s.v2[3 * (size_t)t], &s.v3[3 * (size_t)t], &lo[3 * (size_t)t], &hi[3 * (size_t)t]);
        pt::BvhResult bb;
        pt::build_bvh(lo.data(), hi.data(), (int64_t)n, 0, bb);
        pt::Bvh4Result r;
        pt::collapse_bvh4(bb, pt::kStack4Budget, r);
        pt::BlasPlan R;
        CHECK(pt::blas_rebuild_plan(n, R));
        CHECK(pt::blas_rebuild_stack_bound(R) <= pt::kStack4Budget);
        if (R.num_nodes > (int64_t)r.nodes()) { std::printf(" %d", n); count++; }
    }
    std::printf(" (%d of 400)\n", count);
}

// the cost gates on the 6,400-triangle sphere.  kCostRatio: M / F per pose as this check measured it (it prints the
// figures: twist 0.9613, offset 1.1129); the gate allows 10 % of F more.
static double cost_ratio(const std::string& pose) { return pose == "twist" ? 0.9613 : 1.1129; }
static void check_cost() {
    g_na = 6400; g_nb = 64;
    FixScene s;
    pair_scene(s);
    pt::HostScene H;
    std::string err;
    if (pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) != PT_OK) { CHECK(false); return; }
    for (const char* pn : {"twist", "offset"}) {
        const Verts V = make_pose(s, pn);
        Twin Rf, M, G;
        twin_of(H, Rf);
        twin_update(Rf, V);
        twin_of(H, M);
        twin_rebuild(M, V);
        pt::HostScene F;
        if (!compile_moved(pair_scene, V, F)) return;
        twin_of(F, G);
        double f[3], r[3], m[3];
        cost_of(G, 0, f); cost_of(Rf, 0, r); cost_of(M, 0, m);
        const double cf = f[0] + f[1], cr = r[0] + r[1], cm = m[0] + m[1];
        std::printf("cost sphere %s: fresh %.4f (inner %.4f leaf %.4f) refit %.4f (%.4f %.4f) rebuilt %.4f (%.4f %.4f) M/F %.4f area %.4f\n", pn,
                    cf, f[0], f[1], cr, r[0], r[1], cm, m[0], m[1], cm / cf, m[2]);
        CHECK(M.items[2] > 0);
        CHECK(cm < cr);
        CHECK(cm <= (cost_ratio(pn) + 0.10) * cf);
        CHECK(f[2] > 0 && m[2] == r[2]);
    }
}

// NaN and infinite vertices: the order is unspecified, still a permutation; ASan is the witness for the accesses
static void check_nonfinite() {
    g_na = 1025; g_nb = 17;
    FixScene s;
    pair_scene(s);
    pt::HostScene H;
    std::string err;
    if (pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) != PT_OK) { CHECK(false); return; }
    Twin W;
    twin_of(H, W);
    Verts V = verts_of(s, true);
    const float bad[4] = {NAN, INFINITY, -INFINITY, 3.0e38f};
    for (size_t i = 0; i < V.v1.size(); i++) if (i % 5 == 0) V.v1[i] = bad[i % 4];
    for (size_t i = 0; i < V.v2.size(); i++) if (i % 7 == 0) V.v2[i] = bad[i % 4];
    twin_rebuild(W, V);
    std::vector<int32_t> a = W.B.src_of_pos, b = H.blas_refit.src_of_pos;
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    CHECK(a == b);
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
    g_na = 288; g_nb = 65;
    FixScene s;
    pair_scene(s);
    pt::HostScene H;
    std::string err;
    if (pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) != PT_OK) { CHECK(false); return; }
    Twin W;
    twin_of(H, W);
    dump(dir, "desc.i32", W.B.desc); dump(dir, "src_of_pos.i32", W.B.src_of_pos);
    dump(dir, "nodes0.u32", W.bnodes); dump(dir, "recs0.u32", W.brecs); dump(dir, "shade0.u32", W.bshade);
    const Verts V = make_pose(s, "twist");
    twin_rebuild(W, V);
    dump(dir, "v1.f32", V.v1); dump(dir, "v2.f32", V.v2); dump(dir, "v3.f32", V.v3);
    dump(dir, "n1.f32", V.n1); dump(dir, "n2.f32", V.n2); dump(dir, "n3.f32", V.n3);
    dump(dir, "desc1.i32", W.B.desc); dump(dir, "src_of_pos1.i32", W.B.src_of_pos);
    dump(dir, "nodes1.u32", W.bnodes); dump(dir, "recs1.u32", W.brecs); dump(dir, "shade1.u32", W.bshade);
    dump(dir, "boxes1.f32", W.blas_box);
    std::vector<double> cost(6);
    cost_of(W, 0, &cost[0]); cost_of(W, 1, &cost[3]);
    dump(dir, "cost1.f64", cost);
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "--dump") {
        dump_pose(argv[2]);
        return failures ? 1 : 0;
    }
    const int pairs[][2] = {{1, 288}, {4, 5}, {16, 17}, {64, 65}, {288, 65}, {1025, 17}, {4097, 5}, {6400, 64}};
    for (const auto& p : pairs) check_pair(p[0], p[1]);
    fallback_table();
    check_forced_fallback();
    check_cost();
    check_nonfinite();
    std::printf("blas_rebuild_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
