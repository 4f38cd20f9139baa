// query_tables_check.cpp — the identity tables of pt_intersect_hits (ptsharp_amd/csrc/pt_scene_compile.h QueryTables,
// RefitTables::src_of_pos, BlasRefitTables::src_of_pos) on the host, from first principles, on scenes
// built in C++ (scene_fixture.h):
//   fixed     scene_fixture.h's fixed_scene: every kind of shape, a mesh at top level and inside two transformed
//             shapes, a sphere that is in Scene.Shapes twice;
//   shared    one mesh added twice, a mesh that is both top-level and instanced (twice), a mesh that is only instanced,
//             a loose triangle inside no mesh, a loose triangle inside a top-level mesh's range, a triangle in no
//             shape at all, two planes of which one is added twice.
// Asserted for each:
//   triangles  every source triangle's slot is the one a plain search of Scene.Shapes finds: the first
//              PT_SHAPE_TRIANGLE slot naming it, else the first slot of the last mesh range holding it, else the first
//              slot of a mesh holding it, else -1;
//   analytic   every analytic record's (kind, index) maps to the first slot naming that shape;
//   planes     every plane record likewise;
//   positions  every world BVH position's source triangle has the position's record geometry and a slot whose shape
//              holds that triangle; every BLAS position's source triangle lies in its mesh's range and has its record;
//   rebuild    a permutation of the positions (what pt_rebuild_meshes leaves: rebuild_plan keeps their number) applied
//              to src_of_pos leaves every source triangle's answer unchanged, and the device layout's part sizes too.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ptsharp_amd/csrc/pt_rebuild.h"
#include "../../ptsharp_amd/csrc/pt_scene_compile.h"
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

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// the first slot of Scene.Shapes that names (kind, index), or -1
static int first_slot(const pt_scene_desc& d, int kind, int index) {
    for (int i = 0; i < d.num_shapes; i++)
        if (d.shape_kind[i] == kind && d.shape_index[i] == index) return i;
    return -1;
}
static bool in_mesh(const pt_scene_desc& d, int m, int t) { return t >= d.mesh_first[m] && t < d.mesh_first[m] + d.mesh_count[m]; }

static int expected_tri_slot(const pt_scene_desc& d, int t) {
    const int loose = first_slot(d, PT_SHAPE_TRIANGLE, t);
    if (loose >= 0) return loose;
    int last = -1;
    for (int m = 0; m < d.num_meshes; m++) if (in_mesh(d, m, t)) last = m;
    if (last >= 0 && first_slot(d, PT_SHAPE_MESH, last) >= 0) return first_slot(d, PT_SHAPE_MESH, last);
    int best = -1;
    for (int m = 0; m < d.num_meshes; m++) {
        const int s = first_slot(d, PT_SHAPE_MESH, m);
        if (in_mesh(d, m, t) && s >= 0 && (best < 0 || s < best)) best = s;
    }
    return best;
}

static bool same_vertex(const float4& rec, const float* v) { return bits(rec.x) == bits(v[0]) && bits(rec.y) == bits(v[1]) && bits(rec.z) == bits(v[2]); }

static void check_scene(const char* name, FixScene& s) {
    const pt_scene_desc& d = s.d;
    pt::HostScene H;
    std::string err;
    const int rc = pt::compile_scene(&d, pt::CompileOptions{}, H, err);
    if (rc != PT_OK) { std::fprintf(stderr, "%s: compile_scene %d %s\n", name, rc, err.c_str()); failures++; return; }
    const pt::QueryTables& Q = H.query;
    const int before = failures;
    // triangles
    CHECK((int)Q.tri_slot.size() == d.num_triangles);
    for (int t = 0; t < d.num_triangles && t < (int)Q.tri_slot.size(); t++) CHECK(Q.tri_slot[(size_t)t] == expected_tri_slot(d, t));
    // analytic records
    const int counts[8] = {d.num_spheres, d.num_cubes, 0, 0, 0, d.num_sdf_shapes, d.num_volumes, d.num_transformed};
    int total = 0;
    for (int k = 0; k < 8; k++) { CHECK(Q.ana_off[k] == total); CHECK(Q.ana_cnt[k] == counts[k]); total += counts[k]; }
    CHECK((int)Q.ana_slot.size() == total);
    size_t named = 0;
    for (size_t p = 0; p < H.ana_recs.size() / 3 && failures == before; p++) {
        const int kind = (int)bits(H.ana_recs[3 * p].w), j = (int)bits(H.ana_recs[3 * p + 1].w);
        CHECK(kind >= 0 && kind < 8 && j >= 0 && j < Q.ana_cnt[kind]);
        if (failures != before) break;
        const int slot = Q.ana_slot[(size_t)(Q.ana_off[kind] + j)];
        CHECK(slot >= 0 && slot == first_slot(d, kind, j));
        named++;
    }
    CHECK(named == H.ana_recs.size() / 3);
    for (int k = 0; k < 8; k++)   // a shape in no slot (the inner shape of a transformed shape) has none
        for (int j = 0; j < Q.ana_cnt[k]; j++) CHECK(Q.ana_slot[(size_t)(Q.ana_off[k] + j)] == first_slot(d, k, j));
    // planes
    CHECK((int)Q.plane_slot.size() == d.num_planes);
    for (size_t p = 0; p < H.planes.size() / 2; p++) {
        const int j = (int)bits(H.planes[2 * p + 1].w);
        CHECK(j >= 0 && j < d.num_planes);
        if (j >= 0 && j < (int)Q.plane_slot.size()) CHECK(Q.plane_slot[(size_t)j] >= 0 && Q.plane_slot[(size_t)j] == first_slot(d, PT_SHAPE_PLANE, j));
    }
    // positions of the world BVH
    const std::vector<int32_t>& src = H.refit.src_of_pos;
    CHECK(src.size() == H.tri_sh.size() / 8);
    CHECK(src.size() == pt::gather_tri_src(&d).size());
    for (size_t p = 0; p < src.size(); p++) {
        const int t = src[p];
        CHECK(t >= 0 && t < d.num_triangles);
        if (t < 0 || t >= d.num_triangles) continue;
        CHECK(same_vertex(H.tri_sh[8 * p], d.tri_v1 + 3 * t));
        const int slot = Q.tri_slot[(size_t)t];
        CHECK(slot >= 0 && slot < d.num_shapes);
        if (slot < 0 || slot >= d.num_shapes) continue;
        const int k = d.shape_kind[slot], j = d.shape_index[slot];
        CHECK((k == PT_SHAPE_TRIANGLE && j == t) || (k == PT_SHAPE_MESH && in_mesh(d, j, t)));
    }
    // positions of the BLASes
    const pt::BlasRefitTables& B = H.blas_refit;
    CHECK(B.src_of_pos.size() == H.blas_recs.size() / 3);
    for (size_t x = 0; x < B.xf_blas.size(); x++) {
        const int b = B.xf_blas[x];
        CHECK((b >= 0) == (d.transformed[x].shape_kind == PT_SHAPE_MESH));
        if (b < 0) continue;
        const int m = d.transformed[x].shape_index, r0 = B.desc[4 * (size_t)b + 2], n = B.desc[4 * (size_t)b + 3];
        CHECK(n == d.mesh_count[m]);
        std::vector<int> seen((size_t)n, 0);
        for (int p = r0; p < r0 + n; p++) {
            const int t = B.src_of_pos[(size_t)p];
            CHECK(in_mesh(d, m, t));
            if (!in_mesh(d, m, t)) continue;
            seen[(size_t)(t - d.mesh_first[m])]++;
            CHECK(same_vertex(H.blas_recs[3 * (size_t)p], d.tri_v1 + 3 * t));
        }
        for (int q : seen) CHECK(q == 1);
        CHECK(Q.ana_slot[(size_t)(Q.ana_off[PT_SHAPE_TRANSFORMED] + (int)x)] == first_slot(d, PT_SHAPE_TRANSFORMED, (int)x));
    }
    // a rebuild's permutation of the positions: the per-source answers and the layout stay
    pt::RebuildPlan R;
    CHECK(pt::rebuild_plan((int64_t)src.size(), R) && R.P == (int64_t)src.size() && 3 * R.num_chunks >= R.P);
    std::vector<int32_t> moved(src.size());
    const size_t P = src.size();
    size_t mul = 7;   // coprime with P: p -> (mul p + 3) mod P is a permutation
    while (P > 0 && P % mul == 0) mul += 4;
    for (size_t p = 0; p < P; p++) moved[p] = src[(p * mul + 3) % P];
    if (P > 0) {
        std::vector<int32_t> a(src), b(moved);
        std::sort(a.begin(), a.end());
        std::sort(b.begin(), b.end());
        CHECK(a == b);
        for (size_t p = 0; p < P; p++) {
            const int t = moved[p], slot = Q.tri_slot[(size_t)t];
            CHECK(slot == expected_tri_slot(d, t));
        }
        pt::RefitTables T2 = H.refit;
        T2.src_of_pos = moved;
        const pt::QueryDev L1 = pt::query_layout(H.refit, B, Q, nullptr), L2 = pt::query_layout(T2, B, Q, nullptr);
        CHECK(L1.bytes == L2.bytes && L1.blas_src == L2.blas_src && L1.tri_slot == L2.tri_slot && L1.plane_slot == L2.plane_slot);
        CHECK(((uintptr_t)L1.blas_src & 255) == 0 && ((uintptr_t)L1.tri_slot & 255) == 0 && ((uintptr_t)L1.ana_slot & 255) == 0 &&
              ((uintptr_t)L1.plane_slot & 255) == 0);
        CHECK((uintptr_t)L1.blas_src >= P * 4 && (uintptr_t)L1.tri_slot - (uintptr_t)L1.blas_src >= B.src_of_pos.size() * 4);
        CHECK((uintptr_t)L1.ana_slot - (uintptr_t)L1.tri_slot >= Q.tri_slot.size() * 4);
        CHECK((uintptr_t)L1.plane_slot - (uintptr_t)L1.ana_slot >= Q.ana_slot.size() * 4);
        CHECK(L1.bytes >= (uintptr_t)L1.plane_slot + Q.plane_slot.size() * 4);
    }
    std::printf("case %s %s: %d triangles, %zu positions, %zu BLAS positions, %zu analytic records, %zu planes\n", name,
                failures == before ? "ok" : "FAILED", d.num_triangles, P, B.src_of_pos.size(), H.ana_recs.size() / 3, H.planes.size() / 2);
}

// one mesh added twice, a mesh both top-level and instanced, a mesh only instanced, loose triangles, a triangle in no shape
static void shared_scene(FixScene& s) {
    s.material(0.9, 0.9, 0.9, 0);
    s.material(1, 1, 1, 10);
    auto strip = [&](int n, float y) {
        for (int i = 0; i < n; i++) {
            const float p[3] = {(float)i * 0.5f, y, 2.f}, q[3] = {(float)i * 0.5f + 0.5f, y, 2.f}, r[3] = {(float)i * 0.5f, y + 0.25f, 2.5f};
            s.triangle(p, q, r, MAT_WHITE);
        }
    };
    strip(6, 0.5f);    // mesh 0: triangles 0..5, added twice
    strip(4, 1.5f);    // mesh 1: triangles 6..9, top-level and instanced
    strip(5, 2.5f);    // mesh 2: triangles 10..14, only instanced
    const float a[3] = {6.f, 3.f, 0.f}, b[3] = {7.f, 3.f, 0.f}, c[3] = {6.f, 3.f, 1.f};
    const int loose = s.triangle(a, b, c, MAT_LIGHT);          // 15: inside no mesh
    const int orphan = s.triangle(b, c, a, MAT_WHITE);         // 16: in no shape at all
    (void)orphan;
    s.mfirst = {0, 6, 10}; s.mcount = {6, 4, 5};
    s.pp = {0.f, -2.f, 0.f, 0.f, 9.f, 0.f}; s.pn = {0.f, 1.f, 0.f, 0.f, -1.f, 0.f}; s.pm = {MAT_WHITE, MAT_WHITE};
    const int s0 = s.sphere(0.f, 1.f, 0.f, 1.0, MAT_WHITE);
    const int x0 = s.transformed(PT_SHAPE_MESH, 1, 0, 3, 0), x1 = s.transformed(PT_SHAPE_MESH, 1, 0, 6, 0);
    const int x2 = s.transformed(PT_SHAPE_MESH, 2, 3, 3, 0);
    s.shape(PT_SHAPE_PLANE, 1);
    s.shape(PT_SHAPE_MESH, 0);
    s.shape(PT_SHAPE_TRANSFORMED, x0);
    s.shape(PT_SHAPE_TRIANGLE, loose);
    s.shape(PT_SHAPE_MESH, 1);
    s.shape(PT_SHAPE_TRIANGLE, 7);      // a loose triangle inside mesh 1's range: its own slot wins
    s.shape(PT_SHAPE_MESH, 0);          // the same mesh again: its triangles twice in the BVH, the first slot named
    s.shape(PT_SHAPE_SPHERE, s0);
    s.shape(PT_SHAPE_TRANSFORMED, x1);
    s.shape(PT_SHAPE_TRANSFORMED, x2);
    s.shape(PT_SHAPE_PLANE, 0);
    s.shape(PT_SHAPE_PLANE, 1);
    s.finish(0);
}

int main() {
    {
        FixScene s;
        fixed_scene(s, false);
        check_scene("fixed", s);
    }
    {
        FixScene s;
        shared_scene(s);
        check_scene("shared", s);
        // the answers of that scene, spelled out
        pt::HostScene H;
        std::string err;
        if (pt::compile_scene(&s.d, pt::CompileOptions{}, H, err) == PT_OK) {
            const std::vector<int32_t>& t = H.query.tri_slot;
            CHECK(t.size() == 17);
            if (t.size() == 17) {
                for (int i = 0; i < 6; i++) CHECK(t[(size_t)i] == 1);
                CHECK(t[6] == 4 && t[7] == 5 && t[8] == 4 && t[9] == 4);
                for (int i = 10; i < 15; i++) CHECK(t[(size_t)i] == -1);
                CHECK(t[15] == 3 && t[16] == -1);
            }
            CHECK(H.refit.src_of_pos.size() == 6 + 1 + 4 + 1 + 6);
            CHECK(H.query.plane_slot.size() == 2 && H.query.plane_slot[0] == 10 && H.query.plane_slot[1] == 0);
            const int32_t* xs = H.query.ana_slot.data() + H.query.ana_off[PT_SHAPE_TRANSFORMED];
            CHECK(xs[0] == 2 && xs[1] == 8 && xs[2] == 9);
        } else {
            failures++;
        }
    }
    std::printf("query_tables_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
