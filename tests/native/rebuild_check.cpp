// rebuild_check.cpp — the arithmetic of pt_rebuild_meshes (ptsharp_amd/csrc/pt_rebuild.h) on the host: a CPU twin of the
// rebuild (the order by std::stable_sort over the shared key, axis and segment functions, the topology from
// rebuild_node_words / rebuild_chunk_word0, then pt_refit.h leaves-then-levels, as pt_rebuild.hip and pt_refit.hip
// run them) on scenes built in C++ (scene_fixture.h), checked from first principles and against the host builder.
// The scene of P triangles: the first P - 1 triangles of a displaced sphere (40 x 80 quads, r = 1 + 0.05 sin 7θ cos 5φ
// + 0.02 sin(23φ + 3θ)) as one mesh and one loose emissive triangle.  For P in {1, 2, 3, 4, 24, 25, 192, 193, 1537,
// 6400} and the poses rest, sine, twist (about y by 3 y rad) and offset (each triangle moved by a seeded ±0.5):
//   structure    every position in exactly one chunk of 1..3, src_of_pos a permutation of the upload's, children
//                1..8 with the inner ones first, child indices in range, every node and chunk reached once, word 6's
//                counts those of the chunks, the stack path sum <= 7 h <= kStackMax;
//   containment  by recursion: every slot box holds the padded boxes of the triangles under it, every origin is the
//                least lower bound, the root box is the union of the root's slot boxes;
//   records      the triangle records and the chunk geometry equal a fresh compile's of the deformed scene per source
//                triangle; the emissive loose triangle's light equals the fresh compile's;
//   fixed point  a rebuild applied twice to the same arrays leaves src_of_pos (and every word) as the first left them;
//   cost         on the 6,400-triangle sphere, Σ area(slot box) / area(root box): after the offset pose
//                cost(rebuilt) <= cost(refit) / 3, after the twist cost(rebuilt) <= 0.8 cost(refit);
//   layouts      for every P in 1..6400 (the sanitized build: 1..400, every 61st P after that and the sizes above; a
//                compile each), the refit and pose workspaces (pt_update_layout.h) laid out from the compiled scene's
//                tables: parts 256-B aligned, disjoint, in the documented order and inside `bytes`; level_nodes,
//                node_box and chunk_box hold the uploaded tree and rebuild_plan(P)'s; a layout from the tables a
//                rebuild leaves is never larger.
// `--dump DIR P POSE` writes that case's inputs and outputs as raw arrays (tests/rebuild_ref.py is checked against them).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../ptsharp_amd/csrc/pt_bvh.h"
#include "../../ptsharp_amd/csrc/pt_rebuild.h"
#include "../../ptsharp_amd/csrc/pt_refit.h"
#include "../../ptsharp_amd/csrc/pt_scene_compile.h"
#include "../../ptsharp_amd/csrc/pt_update_layout.h"
#include "layout_parts.h"
#include "scene_fixture.h"

static std::atomic<int> failures{0};   // the layout sweep counts from several threads
constexpr size_t kSweepThreads = 8;
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            if (failures < 40) std::fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
            failures++;                                                           \
        }                                                                         \
    } while (0)

// ---- the scene
enum { MAT_GREY = 0, MAT_EMIT = 1, MAT_TEX = 2 };
constexpr int kTheta = 40, kPhi = 80;
static void sphere_vertex(int i, int j, float* p) {
    const float th = 3.14159265f * (0.02f + 0.96f * (float)i / (float)kTheta), ph = 6.28318531f * (float)j / (float)kPhi;
    const float r = 1.f + 0.05f * std::sin(7.f * th) * std::cos(5.f * ph) + 0.02f * std::sin(23.f * ph + 3.f * th);
    p[0] = r * std::sin(th) * std::cos(ph);
    p[1] = r * std::cos(th);
    p[2] = r * std::sin(th) * std::sin(ph);
}
// P triangles in the BVH: P - 1 of the sphere as one mesh, then the loose emissive triangle
static void sphere_scene(FixScene& s, int P) {
    s.material(0.9, 0.9, 0.9, 0);
    s.material(1, 1, 1, 10);
    s.material(0.5, 0.6, 0.7, 0);
    s.tex0 = {0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 0.9, 0.8};
    s.texs = {pt_texture{2, 2, s.tex0.data()}};
    s.mats[MAT_TEX].texture = 1;
    int made = 0;
    for (int i = 0; i < kTheta && made < P - 1; i++)
        for (int j = 0; j < kPhi && made < P - 1; j++) {
            float a[3], b[3], c[3], e[3];
            sphere_vertex(i, j, a); sphere_vertex(i + 1, j, b); sphere_vertex(i, j + 1, c); sphere_vertex(i + 1, j + 1, e);
            s.triangle(a, b, c, MAT_TEX);
            made++;
            if (made < P - 1) { s.triangle(b, e, c, MAT_TEX); made++; }
        }
    for (size_t t = 0; t < s.tm.size(); t++) {   // normals that differ per vertex, so a wrong gather shows
        s.n1[3 * t] = 0.01f * (float)(t % 17); s.n2[3 * t + 2] = 0.02f * (float)(t % 13); s.n3[3 * t] = -0.03f * (float)(t % 7);
    }
    if (made > 0) { s.mfirst = {0}; s.mcount = {made}; s.shape(PT_SHAPE_MESH, 0); }
    const float l[3][3] = {{0.f, 2.f, 0.f}, {0.5f, 2.f, 0.f}, {0.f, 2.f, 0.5f}};
    s.shape(PT_SHAPE_TRIANGLE, s.triangle(l[0], l[1], l[2], MAT_EMIT));
    s.shape(PT_SHAPE_SPHERE, s.sphere(0.f, 5.f, 0.f, 0.5, MAT_EMIT));
    s.finish(0);
}

// ---- poses
enum { POSE_REST, POSE_SINE, POSE_TWIST, POSE_OFFSET, POSE_COUNT };
static const char* kPoseName[POSE_COUNT] = {"rest", "sine", "twist", "offset"};
struct Pose {
    std::vector<float> v1, v2, v3;
};
static void pose_point(int pose, const float* p, float* q) {
    const float x = p[0], y = p[1], z = p[2];
    switch (pose) {
        case POSE_SINE: q[0] = x; q[1] = y; q[2] = z + 0.3f * std::sin(5.f * x) * std::cos(3.f * y); break;
        case POSE_TWIST: {
            const float a = 3.f * y, c = std::cos(a), s = std::sin(a);
            q[0] = c * x + s * z; q[1] = y; q[2] = c * z - s * x;
            break;
        }
        default: q[0] = x; q[1] = y; q[2] = z; break;
    }
}
static void make_pose(const FixScene& s, int pose, Pose& P) {
    P.v1 = s.v1; P.v2 = s.v2; P.v3 = s.v3;
    FixRng rng{12345u};
    for (size_t t = 0; t < s.tm.size(); t++) {
        pose_point(pose, &s.v1[3 * t], &P.v1[3 * t]);
        pose_point(pose, &s.v2[3 * t], &P.v2[3 * t]);
        pose_point(pose, &s.v3[3 * t], &P.v3[3 * t]);
        if (pose == POSE_OFFSET)
            for (int k = 0; k < 3; k++) {
                const float d = rng.next() - 0.5f;
                P.v1[3 * t + k] += d; P.v2[3 * t + k] += d; P.v3[3 * t + k] += d;
            }
    }
}

// ---- the CPU twin: the device state of a context, pt_update_triangles and pt_rebuild_meshes on it
struct Twin {
    std::vector<uint32_t> nodes, chunks, recs;
    float box[6];
    pt::RefitTables T;
    std::vector<pt::DevLight> lights;
    std::vector<float> node_box, chunk_box;
};
static void twin_of(const pt::HostScene& H, Twin& W) {
    const uint32_t* lines = (const uint32_t*)H.lines.data();
    const size_t n0 = (size_t)H.S.tri_node_line0 * 32, c0 = (size_t)H.S.tri_chunk_line0 * 32, end = (size_t)H.S.lines_n * 32;
    W.nodes.assign(lines + n0, lines + c0);
    W.chunks.assign(lines + c0, lines + end);
    W.recs.assign((const uint32_t*)H.tri_sh.data(), (const uint32_t*)H.tri_sh.data() + H.tri_sh.size() * 4);
    std::memcpy(W.box, H.S.tri_box, sizeof W.box);
    W.T = H.refit;
    W.lights = H.lights;
    W.node_box.assign((size_t)W.T.num_nodes * 6, 0.f);
    W.chunk_box.assign((size_t)W.T.num_chunks * 6, 0.f);
}
static void twin_update(Twin& W, const Pose& P, const float* n1 = nullptr, const float* n2 = nullptr, const float* n3 = nullptr) {
    for (int64_t ci = 0; ci < W.T.num_chunks; ci++)
        pt::refit_chunk(ci, W.chunks.data(), W.recs.data(), W.T.src_of_pos.data(), P.v1.data(), P.v2.data(), P.v3.data(), n1, n2, n3,
                        W.chunk_box.data());
    for (int64_t l = (int64_t)W.T.level_off.size() - 2; l >= 0; l--)
        for (uint32_t i = W.T.level_off[(size_t)l]; i < W.T.level_off[(size_t)l + 1]; i++)
            pt::refit_node((int64_t)W.T.level_nodes[i], W.nodes.data(), W.node_box.data(), W.chunk_box.data());
    if (W.T.num_nodes) pt::tri_root_box(W.nodes.data(), W.box);
    for (size_t i = 0; i < W.lights.size(); i++) {
        const int64_t j = W.T.light_tri[i];
        if (j >= 0) pt::tri_light_sphere(&P.v1[3 * (size_t)j], &P.v2[3 * (size_t)j], &P.v3[3 * (size_t)j], W.lights[i]);
    }
}
// the order of pt_rebuild.h: new position -> the position it had
static std::vector<uint32_t> rebuild_order(const pt::RebuildPlan& R, const std::vector<int32_t>& src, const Pose& P) {
    const int64_t n = R.P;
    std::vector<uint32_t> keys3((size_t)n * 3), cur((size_t)n);
    for (int64_t p = 0; p < n; p++) {
        const size_t s = (size_t)src[(size_t)p];
        pt::rebuild_keys(&P.v1[3 * s], &P.v2[3 * s], &P.v3[3 * s], &keys3[3 * (size_t)p]);
        cur[(size_t)p] = (uint32_t)p;
    }
    for (int r = 1; r <= pt::rebuild_rounds(R); r++) {
        if (!pt::rebuild_round_sorts(R, r)) continue;
        const int shift = pt::rebuild_shift(R, r);
        const int64_t seg = pt::rebuild_segment(R, r);
        for (int64_t first = 0; first < n; first += seg) {
            const uint32_t j = pt::rebuild_segment_of(first, shift);
            CHECK((int64_t)j * seg == first);
            if (!pt::rebuild_segment_sorted(j, shift, n)) continue;
            const int64_t end = std::min(first + seg, n);
            uint32_t b[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
            for (int64_t p = first; p < end; p++)
                for (int a = 0; a < 3; a++) {
                    b[a] = std::min(b[a], keys3[3 * (size_t)cur[(size_t)p] + a]);
                    b[3 + a] = std::max(b[3 + a], keys3[3 * (size_t)cur[(size_t)p] + a]);
                }
            const int ax = pt::rebuild_axis(b);
            std::stable_sort(cur.begin() + first, cur.begin() + end,
                             [&](uint32_t x, uint32_t y) { return keys3[3 * (size_t)x + ax] < keys3[3 * (size_t)y + ax]; });
        }
    }
    return cur;
}
static bool twin_rebuild(Twin& W, const Pose& P, const float* n1 = nullptr, const float* n2 = nullptr, const float* n3 = nullptr) {
    pt::RebuildPlan R;
    if (!pt::rebuild_plan((int64_t)W.T.src_of_pos.size(), R)) return false;
    const std::vector<uint32_t> order = rebuild_order(R, W.T.src_of_pos, P);
    std::vector<uint32_t> recs((size_t)R.P * 32);
    std::vector<int32_t> src((size_t)R.P);
    for (int64_t p = 0; p < R.P; p++) {   // rows 3-7 move with their triangle; rows 0-2 are the refit's
        std::memcpy(&recs[(size_t)p * 32], &W.recs[(size_t)p * 32], 48);
        std::memcpy(&recs[(size_t)p * 32 + 12], &W.recs[(size_t)order[(size_t)p] * 32 + 12], 80);
        src[(size_t)p] = W.T.src_of_pos[(size_t)order[(size_t)p]];
    }
    W.recs = recs;
    W.T.src_of_pos = src;
    // lines past the new counts stay on the device; the twin drops them
    W.nodes.resize((size_t)R.num_nodes * 32, 0u);
    W.chunks.resize((size_t)R.num_chunks * 32, 0u);
    for (int64_t ci = 0; ci < R.num_chunks; ci++) W.chunks[(size_t)ci * 32] = pt::rebuild_chunk_word0(ci, R.P);
    W.T.level_nodes.assign((size_t)R.num_nodes, 0u);
    for (int64_t ni = 0; ni < R.num_nodes; ni++) {
        uint32_t w[5];
        pt::rebuild_node_words(R, ni, w);
        for (int k = 0; k < 5; k++) W.nodes[(size_t)ni * 32 + 3 + (size_t)k] = w[k];
        W.T.level_nodes[(size_t)ni] = (uint32_t)ni;
    }
    W.T.level_off.assign(R.level_off, R.level_off + R.h + 1);
    W.T.num_nodes = R.num_nodes;
    W.T.num_chunks = R.num_chunks;
    W.node_box.assign((size_t)R.num_nodes * 6, 0.f);
    W.chunk_box.assign((size_t)R.num_chunks * 6, 0.f);
    twin_update(W, P, n1, n2, n3);
    return true;
}
static bool same_state(const Twin& a, const Twin& b) {
    return a.nodes == b.nodes && a.chunks == b.chunks && a.recs == b.recs && !std::memcmp(a.box, b.box, sizeof a.box) &&
           a.T.src_of_pos == b.T.src_of_pos;
}
static void twin_cost(const Twin& W, double out[3]) {
    double si = 0.0, sl = 0.0, area = 0.0;
    for (int64_t ni = 0; ni < W.T.num_nodes; ni++) {
        double a, b, own;
        pt::rebuild_node_cost(&W.nodes[(size_t)ni * 32], &a, &b, &own);
        si += a; sl += b;
        if (ni == 0) area = own;
    }
    out[0] = area > 0.0 ? (area + si) / area : 0.0;
    out[1] = area > 0.0 ? sl / area : 0.0;
    out[2] = area;
}

static int compile(FixScene& s, pt::HostScene& H) {
    std::string err;
    const int rc = pt::compile_scene(&s.d, pt::CompileOptions{}, H, err);
    if (rc != PT_OK) std::fprintf(stderr, "compile_scene: %d %s\n", rc, err.c_str());
    return rc;
}

// ---- checks from first principles
struct Box {
    float lo[3], hi[3];
    Box() { for (int k = 0; k < 3; k++) { lo[k] = INFINITY; hi[k] = -INFINITY; } }
    void grow(const Box& o) { for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], o.lo[k]); hi[k] = std::max(hi[k], o.hi[k]); } }
};
static Box padded(const Pose& P, int64_t s) {
    Box b;
    for (int k = 0; k < 3; k++) {
        const float x = P.v1[3 * (size_t)s + k], y = P.v2[3 * (size_t)s + k], z = P.v3[3 * (size_t)s + k];
        const float lo = std::min(std::min(x, y), z), hi = std::max(std::max(x, y), z);
        const float m = std::max(std::fabs(lo), std::fabs(hi));
        volatile float prod = m * 2.0e-6f;   // each operation rounded on its own
        const float e = prod + 1e-30f;
        b.lo[k] = lo - e;
        b.hi[k] = hi + e;
    }
    return b;
}
static Box union_under(const Twin& W, const Pose& P, int64_t ni);
static Box slot_union(const Twin& W, const Pose& P, const uint32_t* w, int k) {
    const int nin = (int)((w[3] >> 24) & 15u);
    if (k < nin) return union_under(W, P, (int64_t)w[4] + k);
    const uint32_t ci = (w[5] + (uint32_t)k) & 0x7FFFFFFFu;
    const uint32_t w0 = W.chunks[(size_t)ci * 32];
    Box b;
    for (uint32_t t = 0; t <= ((w0 >> 29) & 3u); t++) b.grow(padded(P, W.T.src_of_pos[(w0 & 0x1FFFFFFFu) + t]));
    return b;
}
static Box union_under(const Twin& W, const Pose& P, int64_t ni) {
    const uint32_t* w = &W.nodes[(size_t)ni * 32];
    const int nc = (int)(w[3] >> 28);
    Box all;
    float origin[3] = {INFINITY, INFINITY, INFINITY};
    for (int k = 0; k < 8; k++) {
        float lo[3], hi[3];
        pt::bvh8_child_box(w, k, lo, hi);
        if (k >= nc) { CHECK(lo[0] == INFINITY && hi[0] == -INFINITY); continue; }
        const Box u = slot_union(W, P, w, k);
        for (int ax = 0; ax < 3; ax++) {
            CHECK(lo[ax] <= u.lo[ax] && hi[ax] >= u.hi[ax]);
            origin[ax] = std::min(origin[ax], u.lo[ax]);
        }
        all.grow(u);
    }
    for (int ax = 0; ax < 3; ax++) CHECK(pt::refit_bits(origin[ax]) == w[ax]);
    return all;
}
// bvh8_check's structural rules on the twin; the permutation against the upload's src_of_pos
static void check_structure(const Twin& W, const std::vector<int32_t>& src0) {
    const size_t nn = (size_t)W.T.num_nodes, nc_ = (size_t)W.T.num_chunks, np = W.T.src_of_pos.size();
    pt::RebuildPlan R;
    CHECK(pt::rebuild_plan((int64_t)np, R));
    CHECK((size_t)R.num_nodes == nn && (size_t)R.num_chunks == nc_ && W.nodes.size() == nn * 32 && W.chunks.size() == nc_ * 32);
    CHECK(pt::rebuild_stack_bound(R) <= pt::kStackMax);
    std::vector<int32_t> a = src0, b = W.T.src_of_pos;
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    CHECK(a == b);
    std::vector<int> pos_seen(np, 0), reached(nn, 0), chunk_seen(nc_, 0);
    for (size_t ci = 0; ci < nc_; ci++) {
        const uint32_t w0 = W.chunks[ci * 32], first = w0 & 0x1FFFFFFFu, cnt = ((w0 >> 29) & 3u) + 1u;
        CHECK(cnt <= 3u && (size_t)first + cnt <= np);
        for (uint32_t t = 0; t < cnt && (size_t)first + t < np; t++) pos_seen[first + t]++;
    }
    for (int v : pos_seen) CHECK(v == 1);
    std::vector<std::pair<uint32_t, int>> todo{{0u, 0}};
    int need = 0;
    while (!todo.empty() && nn > 0) {
        const auto [nd, pushed] = todo.back();
        todo.pop_back();
        CHECK(nd < nn);
        if (nd >= nn) continue;
        reached[nd]++;
        const uint32_t* w = &W.nodes[(size_t)nd * 32];
        const int nc = (int)(w[3] >> 28), nin = (int)((w[3] >> 24) & 15u);
        CHECK(nc >= 1 && nc <= 8 && nin <= nc);
        CHECK(w[7] == 0u);
        const int p = pushed + nc - 1;
        need = std::max(need, p);
        for (int k = 0; k < nc && k < 8; k++) {
            if (k < nin) {   // the inner children come first
                const uint32_t c = w[4] + (uint32_t)k;
                CHECK(c < nn && c > nd);
                if (c < nn) todo.push_back({c, p});
            } else {
                CHECK(((w[5] + (uint32_t)k) & 0x80000000u) != 0);   // a leaf ref
                const uint32_t ch = (w[5] + (uint32_t)k) & 0x7FFFFFFFu;
                CHECK(ch < nc_);
                if (ch >= nc_) continue;
                chunk_seen[ch]++;
                CHECK(((w[6] >> (2 * k)) & 3u) == ((W.chunks[(size_t)ch * 32] >> 29) & 3u));
            }
        }
    }
    for (int v : reached) CHECK(v == 1);
    for (int v : chunk_seen) CHECK(v == 1);
    CHECK(need <= 7 * R.h && 7 * R.h <= pt::kStackMax);
    // the level table: every node once, parents on lower levels than their children
    CHECK(W.T.level_off.size() == (size_t)R.h + 1 && W.T.level_nodes.size() == nn);
    std::vector<int> level(nn, -1);
    for (size_t l = 0; l + 1 < W.T.level_off.size(); l++)
        for (uint32_t i = W.T.level_off[l]; i < W.T.level_off[l + 1] && i < nn; i++) level[W.T.level_nodes[i]] = (int)l;
    for (size_t ni = 0; ni < nn; ni++) {
        CHECK(level[ni] >= 0);
        const uint32_t* w = &W.nodes[ni * 32];
        for (uint32_t k = 0; k < ((w[3] >> 24) & 15u); k++)
            if (w[4] + k < nn) CHECK(level[w[4] + k] == level[ni] + 1);
    }
}

static void check_case(int P, int pose) {
    FixScene s;
    sphere_scene(s, P);
    pt::HostScene H0;
    if (compile(s, H0) != PT_OK) { failures++; return; }
    const int before = failures;
    Pose Q;
    make_pose(s, pose, Q);
    Twin W;
    twin_of(H0, W);
    CHECK((int)W.T.src_of_pos.size() == P);
    const std::vector<int32_t> src0 = W.T.src_of_pos;
    const long long up_nodes = (long long)W.T.num_nodes, up_chunks = (long long)W.T.num_chunks;
    CHECK(twin_rebuild(W, Q));
    if (pose == POSE_REST)   // what pt_rebuild_meshes checks against the upload's allocation
        std::printf("P %-5d upload %lld nodes %lld chunks, rebuilt %lld nodes %lld chunks\n", P, up_nodes, up_chunks,
                    (long long)W.T.num_nodes, (long long)W.T.num_chunks);
    check_structure(W, src0);
    // containment, origins, the root box
    const Box all = union_under(W, Q, 0);
    float rb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < (int)(W.nodes[3] >> 28); k++) {
        float lo[3], hi[3];
        pt::bvh8_child_box(W.nodes.data(), k, lo, hi);
        for (int ax = 0; ax < 3; ax++) { rb[ax] = std::min(rb[ax], lo[ax]); rb[3 + ax] = std::max(rb[3 + ax], hi[ax]); }
    }
    CHECK(!std::memcmp(rb, W.box, sizeof rb));
    for (int ax = 0; ax < 3; ax++) CHECK(W.box[ax] <= all.lo[ax] && W.box[3 + ax] >= all.hi[ax]);
    // a fresh compile of the deformed scene: records and chunk geometry per source triangle, the light
    FixScene f;
    sphere_scene(f, P);
    f.v1 = Q.v1; f.v2 = Q.v2; f.v3 = Q.v3;   // same sizes: the pointers in f.d stay valid
    pt::HostScene H1;
    if (compile(f, H1) != PT_OK) { failures++; return; }
    Twin F;
    twin_of(H1, F);
    CHECK(F.T.src_of_pos.size() == W.T.src_of_pos.size());
    std::vector<int64_t> fresh_pos(s.tm.size(), -1), fresh_chunk(F.T.src_of_pos.size(), -1);
    std::vector<int> fresh_slot(F.T.src_of_pos.size(), 0);
    for (size_t i = 0; i < F.T.src_of_pos.size(); i++) fresh_pos[(size_t)F.T.src_of_pos[i]] = (int64_t)i;
    for (int64_t ci = 0; ci < F.T.num_chunks; ci++) {
        const uint32_t w0 = F.chunks[(size_t)ci * 32];
        for (uint32_t t = 0; t <= ((w0 >> 29) & 3u); t++) { fresh_chunk[(w0 & 0x1FFFFFFFu) + t] = ci; fresh_slot[(w0 & 0x1FFFFFFFu) + t] = (int)t; }
    }
    for (size_t i = 0; i < W.T.src_of_pos.size(); i++) {
        const int64_t fp = fresh_pos[(size_t)W.T.src_of_pos[i]];
        CHECK(fp >= 0);
        if (fp < 0) continue;
        CHECK(!std::memcmp(&W.recs[i * 32], &F.recs[(size_t)fp * 32], 128));
    }
    for (int64_t ci = 0; ci < W.T.num_chunks; ci++) {
        const uint32_t w0 = W.chunks[(size_t)ci * 32];
        for (uint32_t t = 0; t <= ((w0 >> 29) & 3u); t++) {
            const int64_t fp = fresh_pos[(size_t)W.T.src_of_pos[(w0 & 0x1FFFFFFFu) + t]];
            if (fp < 0) continue;
            CHECK(!std::memcmp(&W.chunks[(size_t)ci * 32 + 1 + 9 * t], &F.chunks[(size_t)fresh_chunk[(size_t)fp] * 32 + 1 + 9 * (size_t)fresh_slot[(size_t)fp]], 36));
        }
    }
    CHECK(W.lights.size() == F.lights.size() && W.lights.size() == 2);
    for (size_t i = 0; i < W.lights.size() && i < F.lights.size(); i++) CHECK(!std::memcmp(&W.lights[i], &F.lights[i], sizeof(pt::DevLight)));
    // a second rebuild with the same arrays: a fixed point
    Twin W2 = W;
    CHECK(twin_rebuild(W2, Q));
    CHECK(same_state(W, W2));
    // a refit of the rebuilt topology back at the rest pose still holds its triangles
    if (pose != POSE_REST) {
        Pose R0{s.v1, s.v2, s.v3};
        twin_update(W2, R0);
        union_under(W2, R0, 0);
    }
    std::printf("P %-5d pose %-7s %s\n", P, kPoseName[pose], failures == before ? "ok" : "FAILED");
}

static void check_cost() {
    FixScene s;
    sphere_scene(s, 6400);
    pt::HostScene H;
    if (compile(s, H) != PT_OK) { failures++; return; }
    const double bound[POSE_COUNT] = {0.0, 0.0, 0.8, 1.0 / 3.0};
    for (int pose : {POSE_TWIST, POSE_OFFSET}) {
        Pose Q;
        make_pose(s, pose, Q);
        Twin A, B;
        twin_of(H, A);
        twin_of(H, B);
        twin_update(A, Q);
        CHECK(twin_rebuild(B, Q));
        double ca[3], cb[3];
        twin_cost(A, ca);
        twin_cost(B, cb);
        const double refit = ca[0] + ca[1], rebuilt = cb[0] + cb[1];
        std::printf("cost %-7s refit %.3f rebuilt %.3f ratio %.3f (bound %.3f)\n", kPoseName[pose], refit, rebuilt, rebuilt / refit, bound[pose]);
        CHECK(rebuilt <= bound[pose] * refit);
    }
}

// ---- the refit and pose workspaces of a P-triangle scene as pt_api.hip lays them out once per scene, from the
// uploaded tables: the refit's scratch parts hold the uploaded tree and the balanced one a rebuild puts in its place
static void check_layouts(int P) {
    FixScene s;
    sphere_scene(s, P);
    pt::HostScene H;
    if (compile(s, H) != PT_OK) { failures++; return; }
    const pt::RefitTables& T = H.refit;
    pt::RebuildPlan R;
    CHECK(pt::rebuild_plan(P, R));
    const size_t nt = s.tm.size(), up_nodes = (size_t)T.num_nodes, up_chunks = (size_t)T.num_chunks;
    CHECK((size_t)T.num_triangles == nt && T.src_of_pos.size() == (size_t)P && T.level_nodes.size() == up_nodes);
    const size_t nodes = std::max(up_nodes, (size_t)R.num_nodes), chunks = std::max(up_chunks, (size_t)R.num_chunks);
    const pt::RefitDev D = pt::refit_layout(T, nullptr);
    std::vector<LayoutPart> parts;
    for (const float* a : D.in) parts.push_back({a, nt * 3 * sizeof(float)});
    parts.push_back({D.src_of_pos, (size_t)P * sizeof(int32_t)});
    parts.push_back({D.level_nodes, nodes * sizeof(uint32_t)});
    parts.push_back({D.node_box, nodes * 6 * sizeof(float)});
    parts.push_back({D.chunk_box, chunks * 6 * sizeof(float)});
    CHECK(layout_violations(parts, D.bytes) == 0);
    // the tables overwritten as pt_rebuild_meshes leaves them: a layout from these is never larger, part by part
    pt::RefitTables T1 = T;
    T1.num_nodes = R.num_nodes;
    T1.num_chunks = R.num_chunks;
    T1.level_nodes.resize((size_t)R.num_nodes);
    T1.level_off.assign(R.level_off, R.level_off + R.h + 1);
    const pt::RefitDev D1 = pt::refit_layout(T1, nullptr);
    CHECK(D1.bytes <= D.bytes && D1.level_nodes == D.level_nodes && D1.node_box <= D.node_box && D1.chunk_box <= D.chunk_box);

    const size_t ng = (size_t)T.num_groups;
    const pt::PoseDev Q = pt::pose_layout(T, nullptr);
    parts.clear();
    for (const float* a : Q.rest) parts.push_back({a, nt * 3 * sizeof(float)});
    parts.push_back({Q.group, nt * sizeof(int32_t)});
    parts.push_back({Q.matrices, ng * 16 * sizeof(double)});
    parts.push_back({Q.mask, ng * sizeof(int32_t)});
    CHECK(layout_violations(parts, Q.bytes) == 0);
    pt::tri_bvh_release(H.tri_build);   // the sweep keeps no build cached
}

template <class T>
static void dump(const std::string& dir, const char* name, const T* p, size_t n) {
    const std::string path = dir + "/" + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); failures++; }
    if (f) std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc == 5 && !std::strcmp(argv[1], "--dump")) {   // one case, normals given: inputs and outputs as raw arrays
        const std::string dir = argv[2];
        const int P = std::atoi(argv[3]);
        int pose = -1;
        for (int k = 0; k < POSE_COUNT; k++) if (!std::strcmp(argv[4], kPoseName[k])) pose = k;
        if (P < 1 || P > 6400 || pose < 0) { std::fprintf(stderr, "usage: rebuild_check --dump DIR P rest|sine|twist|offset\n"); return 2; }
        FixScene s;
        sphere_scene(s, P);
        pt::HostScene H;
        if (compile(s, H) != PT_OK) return 1;
        Twin W;
        twin_of(H, W);
        Pose Q;
        make_pose(s, pose, Q);
        std::vector<float> n1 = s.n1, n2 = s.n2, n3 = s.n3;
        for (size_t i = 0; i < n1.size(); i++) { n1[i] += 0.5f; n2[i] -= 0.25f; n3[i] *= 2.f; }
        dump(dir, "recs0.u32", W.recs.data(), W.recs.size());
        dump(dir, "src0.i32", W.T.src_of_pos.data(), W.T.src_of_pos.size());
        dump(dir, "v1.f32", Q.v1.data(), Q.v1.size()); dump(dir, "v2.f32", Q.v2.data(), Q.v2.size()); dump(dir, "v3.f32", Q.v3.data(), Q.v3.size());
        dump(dir, "n1.f32", n1.data(), n1.size()); dump(dir, "n2.f32", n2.data(), n2.size()); dump(dir, "n3.f32", n3.data(), n3.size());
        if (!twin_rebuild(W, Q, n1.data(), n2.data(), n3.data())) return 1;
        double cost[3];
        twin_cost(W, cost);
        dump(dir, "nodes1.u32", W.nodes.data(), W.nodes.size());
        dump(dir, "chunks1.u32", W.chunks.data(), W.chunks.size());
        dump(dir, "recs1.u32", W.recs.data(), W.recs.size());
        dump(dir, "src1.i32", W.T.src_of_pos.data(), W.T.src_of_pos.size());
        dump(dir, "box1.f32", W.box, 6);
        dump(dir, "cost1.f64", cost, 3);
        return failures ? 1 : 0;
    }
    {   // the plan's limits
        pt::RebuildPlan R;
        CHECK(pt::rebuild_plan(0, R) && R.num_nodes == 0 && R.num_chunks == 0);
        CHECK(pt::rebuild_plan(24, R) && R.h == 1 && R.num_nodes == 1);
        CHECK(pt::rebuild_plan(25, R) && R.h == 2 && R.num_nodes == 3);
        CHECK(pt::rebuild_plan((int64_t)3 << 27, R) && R.h == 9);
        CHECK(!pt::rebuild_plan(((int64_t)3 << 27) + 1, R));
        CHECK(!pt::rebuild_plan(-1, R));
    }
    for (int P : {1, 2, 3, 4, 24, 25, 192, 193, 1537, 6400})
        for (int pose = 0; pose < POSE_COUNT; pose++) check_case(P, pose);
    check_cost();
    {   // every P up to the largest case, a compile each, on a few threads (the compile is made for that: contexts
        // upload at once).  Under the sanitizers all 6,400 take minutes: that build keeps every P up to 400, every
        // 61st after that and the cases above.
#if defined(__SANITIZE_ADDRESS__)
        const bool all = false;
#else
        const bool all = true;
#endif
        const int before = failures;
        std::vector<int> sweep;
        for (int P = 1; P <= 6400; P++)
            if (all || P <= 400 || P % 61 == 0 || P == 1537 || P == 6400) sweep.push_back(P);
        std::vector<std::thread> pool;
        for (size_t t = 0; t < kSweepThreads; t++)
            pool.emplace_back([&sweep, t] { for (size_t i = t; i < sweep.size(); i += kSweepThreads) check_layouts(sweep[i]); });
        for (std::thread& th : pool) th.join();
        std::printf("layouts %zu of P 1..6400 %s\n", sweep.size(), failures == before ? "ok" : "FAILED");
    }
    std::printf("rebuild_check: %d failures\n", failures.load());
    return failures ? 1 : 0;
}
