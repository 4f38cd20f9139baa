// refit_check.cpp — the arithmetic of pt_update_triangles (ptsharp_amd/csrc/pt_refit.h) on the host: a CPU twin of
// the refit (the shared functions driven leaves-then-levels over the compile's tables, as pt_refit.hip's kernels
// are) on scenes built in C++ (scene_fixture.h), checked against the host builder:
//   identity      a refit with the vertices a scene was compiled from reproduces the node lines, chunk lines and
//                 tri_sh byte for byte (a 40x40 grid mesh with three loose triangles, a single triangle: the
//                 lone-leaf root, two triangles, nine triangles: a root with empty slots);
//   deformations  of the grid: every slot's box contains the padded boxes of the triangles under it, every origin
//                 is the least lower bound of the node's children, the root box is the union of the root's slot
//                 boxes, and the triangle records and chunk geometry equal a fresh compile's of the deformed scene
//                 per source triangle; the emissive loose triangle's light sphere equals the fresh compile's;
//   sequence      pose A then pose B gives the bytes of pose B alone;
//   tables        the level table lists every node once, parents on lower levels than their children.
// `--dump DIR` writes the sine pose's inputs and outputs as raw arrays (tests/refit_ref.py is checked against them).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ptsharp_amd/csrc/pt_bvh.h"
#include "../../ptsharp_amd/csrc/pt_refit.h"
#include "../../ptsharp_amd/csrc/pt_scene_compile.h"
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
enum { MAT_GREY = 0, MAT_EMIT = 1, MAT_TEX = 2 };
static void materials(FixScene& s) {
    s.material(0.9, 0.9, 0.9, 0);
    s.material(1, 1, 1, 10);
    s.material(0.5, 0.6, 0.7, 0);
    s.tex0 = {0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 0.9, 0.8};
    s.texs = {pt_texture{2, 2, s.tex0.data()}};
    s.mats[MAT_TEX].texture = 1;
}
constexpr int kGrid = 40;
static void grid_vertex(int i, int j, float* p) {
    p[0] = (float)i * 0.1f - 2.f;
    p[1] = (float)j * 0.1f - 2.f;
    p[2] = 0.25f * std::cos(1.5f * p[0]) * std::sin(2.f * p[1]);
}
// the grid mesh (2 * 40 * 40 triangles, distinct vertex normals) and three loose triangles, the second emissive
static void grid_scene(FixScene& s) {
    materials(s);
    for (int j = 0; j < kGrid; j++)
        for (int i = 0; i < kGrid; i++) {
            float a[3], b[3], c[3], e[3];
            grid_vertex(i, j, a); grid_vertex(i + 1, j, b); grid_vertex(i, j + 1, c); grid_vertex(i + 1, j + 1, e);
            s.triangle(a, b, c, MAT_TEX);
            s.triangle(b, e, c, MAT_TEX);
        }
    for (size_t t = 0; t < s.tm.size(); t++) {   // normals that differ per vertex, so a wrong gather shows
        s.n1[3 * t] = 0.01f * (float)(t % 17); s.n2[3 * t + 2] = 0.02f * (float)(t % 13); s.n3[3 * t] = -0.03f * (float)(t % 7);
    }
    s.mfirst = {0}; s.mcount = {2 * kGrid * kGrid};
    const float l0[3][3] = {{-3.f, 0.f, 1.f}, {-2.5f, 0.f, 1.f}, {-3.f, 0.5f, 1.2f}};
    const float l1[3][3] = {{0.f, 0.f, 2.f}, {0.5f, 0.f, 2.f}, {0.f, 0.5f, 2.f}};
    const float l2[3][3] = {{3.f, 3.f, -1.f}, {3.5f, 3.f, -1.f}, {3.f, 3.5f, -1.5f}};
    const int t0 = s.triangle(l0[0], l0[1], l0[2], MAT_GREY), t1 = s.triangle(l1[0], l1[1], l1[2], MAT_EMIT);
    const int t2 = s.triangle(l2[0], l2[1], l2[2], MAT_GREY);
    s.shape(PT_SHAPE_TRIANGLE, t0);
    s.shape(PT_SHAPE_MESH, 0);
    s.shape(PT_SHAPE_TRIANGLE, t1);
    s.shape(PT_SHAPE_TRIANGLE, t2);
    s.shape(PT_SHAPE_SPHERE, s.sphere(0.f, 0.f, 5.f, 0.5, MAT_EMIT));
    s.finish(0);
}
// n loose triangles in a row
static void row_scene(FixScene& s, int n) {
    materials(s);
    for (int i = 0; i < n; i++) {
        const float a[3] = {(float)i, 0.f, 0.f}, b[3] = {(float)i + 0.75f, 0.f, 0.25f}, c[3] = {(float)i, 1.f, 0.5f};
        s.shape(PT_SHAPE_TRIANGLE, s.triangle(a, b, c, i == 0 ? MAT_EMIT : MAT_GREY));
    }
    s.finish(0);
}

// ---- the CPU twin: the device state of a context and pt_update_triangles on it
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
struct Pose {
    std::vector<float> v1, v2, v3;
};
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
static bool same_state(const Twin& a, const Twin& b) {
    return a.nodes == b.nodes && a.chunks == b.chunks && a.recs == b.recs && !std::memcmp(a.box, b.box, sizeof a.box);
}

static int compile(FixScene& s, pt::HostScene& H) {
    std::string err;
    const int rc = pt::compile_scene(&s.d, pt::CompileOptions{}, H, err);
    if (rc != PT_OK) std::fprintf(stderr, "compile_scene: %d %s\n", rc, err.c_str());
    return rc;
}

// ---- poses of the grid scene
enum { POSE_TRANSLATE, POSE_SCALE, POSE_SINE, POSE_FLAT, POSE_POINT, POSE_HUGE, POSE_TINY, POSE_COUNT };
static const char* kPoseName[POSE_COUNT] = {"translate", "scale", "sine", "flat", "point", "huge", "tiny"};
static void pose_point(int pose, const float* p, float* q) {
    const float x = p[0], y = p[1], z = p[2];
    switch (pose) {
        case POSE_TRANSLATE: q[0] = x + 1000.f; q[1] = y - 2000.f; q[2] = z + 3000.f; break;
        case POSE_SCALE: q[0] = x * 37.f; q[1] = y * 0.01f; q[2] = z; break;
        case POSE_SINE: q[0] = x; q[1] = y; q[2] = z + 0.3f * std::sin(5.f * x) * std::cos(3.f * y); break;
        case POSE_FLAT: q[0] = x; q[1] = y; q[2] = 0.f; break;
        case POSE_POINT: q[0] = 0.5f; q[1] = -0.25f; q[2] = 2.f; break;
        case POSE_HUGE: q[0] = x * 1e6f; q[1] = y * 1e6f; q[2] = z * 1e6f; break;
        default: q[0] = x * 1e-6f; q[1] = y * 1e-6f; q[2] = z * 1e-6f; break;
    }
}
static void make_pose(const FixScene& s, int pose, Pose& P) {
    P.v1 = s.v1; P.v2 = s.v2; P.v3 = s.v3;
    for (size_t t = 0; t < s.tm.size(); t++) {
        pose_point(pose, &s.v1[3 * t], &P.v1[3 * t]);
        pose_point(pose, &s.v2[3 * t], &P.v2[3 * t]);
        pose_point(pose, &s.v3[3 * t], &P.v3[3 * t]);
    }
}

// ---- checks from first principles
struct Box {
    float lo[3], hi[3];
    Box() { for (int k = 0; k < 3; k++) { lo[k] = INFINITY; hi[k] = -INFINITY; } }
    void grow(const Box& o) { for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], o.lo[k]); hi[k] = std::max(hi[k], o.hi[k]); } }
};
// the padded box of a triangle as the header and DESIGN.md §4c state it
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
static Box union_under(const Twin& W, const Pose& P, int64_t ni, std::vector<int>& seen);
static Box slot_union(const Twin& W, const Pose& P, const uint32_t* w, int k, std::vector<int>& seen) {
    const int nin = (int)((w[3] >> 24) & 15u);
    if (k < nin) return union_under(W, P, (int64_t)w[4] + k, seen);
    const uint32_t ci = (w[5] + (uint32_t)k) & 0x7FFFFFFFu;
    const uint32_t w0 = W.chunks[(size_t)ci * 32];
    Box b;
    for (uint32_t t = 0; t <= ((w0 >> 29) & 3u); t++) b.grow(padded(P, W.T.src_of_pos[(w0 & 0x1FFFFFFFu) + t]));
    return b;
}
static Box union_under(const Twin& W, const Pose& P, int64_t ni, std::vector<int>& seen) {
    seen[(size_t)ni]++;
    const uint32_t* w = &W.nodes[(size_t)ni * 32];
    const int nc = (int)(w[3] >> 28);
    Box all;
    float origin[3] = {INFINITY, INFINITY, INFINITY};
    for (int k = 0; k < 8; k++) {
        float lo[3], hi[3];
        pt::bvh8_child_box(w, k, lo, hi);
        if (k >= nc) { CHECK(lo[0] == INFINITY && hi[0] == -INFINITY); continue; }
        const Box u = slot_union(W, P, w, k, seen);
        for (int ax = 0; ax < 3; ax++) {
            CHECK(lo[ax] <= u.lo[ax] && hi[ax] >= u.hi[ax]);
            origin[ax] = std::min(origin[ax], u.lo[ax]);
        }
        all.grow(u);
    }
    for (int ax = 0; ax < 3; ax++) CHECK(pt::refit_bits(origin[ax]) == w[ax]);
    return all;
}

static void check_pose(FixScene& s, const pt::HostScene& H0, int pose) {
    Pose P;
    make_pose(s, pose, P);
    Twin W;
    twin_of(H0, W);
    twin_update(W, P);
    const int before = failures;
    // containment, origins, every node reached once
    std::vector<int> seen((size_t)W.T.num_nodes, 0);
    const Box all = union_under(W, P, 0, seen);
    for (int v : seen) CHECK(v == 1);
    // the root box: the union of the root's slot boxes, holding every triangle
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
    grid_scene(f);
    f.v1 = P.v1; f.v2 = P.v2; f.v3 = P.v3;   // same sizes: the pointers in f.d stay valid
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
        CHECK(!std::memcmp(&W.recs[i * 32], &F.recs[(size_t)fp * 32], 128));   // rows 0-5 and the uv rows
    }
    for (int64_t ci = 0; ci < W.T.num_chunks; ci++) {
        const uint32_t w0 = W.chunks[(size_t)ci * 32];
        for (uint32_t t = 0; t <= ((w0 >> 29) & 3u); t++) {
            const int64_t fp = fresh_pos[(size_t)W.T.src_of_pos[(w0 & 0x1FFFFFFFu) + t]];
            if (fp < 0) continue;
            CHECK(!std::memcmp(&W.chunks[(size_t)ci * 32 + 1 + 9 * t], &F.chunks[(size_t)fresh_chunk[(size_t)fp] * 32 + 1 + 9 * (size_t)fresh_slot[(size_t)fp]], 36));
        }
    }
    CHECK(W.lights.size() == F.lights.size());
    for (size_t i = 0; i < W.lights.size() && i < F.lights.size(); i++) CHECK(!std::memcmp(&W.lights[i], &F.lights[i], sizeof(pt::DevLight)));
    std::printf("pose %-9s %s\n", kPoseName[pose], failures == before ? "ok" : "FAILED");
}

static void check_identity(FixScene& s, const char* name, int min_levels) {
    pt::HostScene H;
    if (compile(s, H) != PT_OK) { failures++; return; }
    Twin A, B;
    twin_of(H, A);
    twin_of(H, B);
    Pose P{s.v1, s.v2, s.v3};
    // scratch the coordinate words first, so a word the refit does not write shows
    for (size_t i = 0; i < B.nodes.size(); i += 32) {
        for (int k = 0; k < 3; k++) B.nodes[i + k] ^= 0x00400000u;
        B.nodes[i + 3] ^= 0x00010101u;
        for (int k = 8; k < 32; k++) B.nodes[i + k] = 0x12345678u;
    }
    for (size_t i = 0; i < B.chunks.size(); i += 32)
        for (int k = 1; k < 32; k++) B.chunks[i + k] = 0x3F800000u;
    for (size_t i = 0; i < B.recs.size(); i += 32)
        for (int k = 0; k < 12; k++) B.recs[i + k] = 0x3F800000u;
    std::memset(B.box, 0, sizeof B.box);
    const int before = failures;
    twin_update(B, P);
    CHECK(A.nodes == B.nodes);
    CHECK(A.chunks == B.chunks);
    CHECK(A.recs == B.recs);
    CHECK(!std::memcmp(A.box, B.box, sizeof A.box));
    // with the normals given too (rows 3-5 scratched but the material word)
    for (size_t i = 0; i < B.recs.size(); i += 32)
        for (int k = 12; k < 24; k++) if (k != 21) B.recs[i + k] = 0x3F800000u;
    twin_update(B, P, s.n1.data(), s.n2.data(), s.n3.data());
    CHECK(A.recs == B.recs);
    CHECK((int)A.T.level_off.size() - 1 >= min_levels);
    // tables: every node once, parents on lower levels than their children
    std::vector<int> level((size_t)A.T.num_nodes, -1);
    CHECK((int64_t)A.T.level_nodes.size() == A.T.num_nodes);
    for (size_t l = 0; l + 1 < A.T.level_off.size(); l++)
        for (uint32_t i = A.T.level_off[l]; i < A.T.level_off[l + 1]; i++) {
            const uint32_t ni = A.T.level_nodes[i];
            CHECK((int64_t)ni < A.T.num_nodes && level[ni] == -1);
            if ((int64_t)ni < A.T.num_nodes) level[ni] = (int)l;
        }
    for (int64_t ni = 0; ni < A.T.num_nodes; ni++) {
        CHECK(level[(size_t)ni] >= 0);
        const uint32_t* w = &A.nodes[(size_t)ni * 32];
        for (uint32_t k = 0; k < ((w[3] >> 24) & 15u); k++) CHECK(level[w[4] + k] > level[(size_t)ni]);
    }
    if (A.T.num_nodes) CHECK(level[0] == 0 && A.T.level_off[1] == 1);
    std::printf("identity %-8s %lld nodes, %lld chunks, %zu triangles, %zu levels: %s\n", name, (long long)A.T.num_nodes,
                (long long)A.T.num_chunks, A.T.src_of_pos.size(), A.T.level_off.size() - 1, failures == before ? "ok" : "FAILED");
}

template <class T>
static void dump(const std::string& dir, const char* name, const T* p, size_t n) {
    const std::string path = dir + "/" + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); failures++; }
    if (f) std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "--dump")) {   // the sine pose, normals given: inputs and outputs as raw arrays
        const std::string dir = argv[2];
        FixScene s;
        grid_scene(s);
        pt::HostScene H;
        if (compile(s, H) != PT_OK) return 1;
        Twin W;
        twin_of(H, W);
        Pose P;
        make_pose(s, POSE_SINE, P);
        std::vector<float> n1 = s.n1, n2 = s.n2, n3 = s.n3;
        for (size_t i = 0; i < n1.size(); i++) { n1[i] += 0.5f; n2[i] -= 0.25f; n3[i] *= 2.f; }
        dump(dir, "nodes0.u32", W.nodes.data(), W.nodes.size());
        dump(dir, "chunks0.u32", W.chunks.data(), W.chunks.size());
        dump(dir, "recs0.u32", W.recs.data(), W.recs.size());
        dump(dir, "src_of_pos.i32", W.T.src_of_pos.data(), W.T.src_of_pos.size());
        dump(dir, "v1.f32", P.v1.data(), P.v1.size()); dump(dir, "v2.f32", P.v2.data(), P.v2.size()); dump(dir, "v3.f32", P.v3.data(), P.v3.size());
        dump(dir, "n1.f32", n1.data(), n1.size()); dump(dir, "n2.f32", n2.data(), n2.size()); dump(dir, "n3.f32", n3.data(), n3.size());
        twin_update(W, P, n1.data(), n2.data(), n3.data());
        dump(dir, "nodes1.u32", W.nodes.data(), W.nodes.size());
        dump(dir, "chunks1.u32", W.chunks.data(), W.chunks.size());
        dump(dir, "recs1.u32", W.recs.data(), W.recs.size());
        dump(dir, "box1.f32", W.box, 6);
        return failures ? 1 : 0;
    }
    {
        FixScene s; grid_scene(s); check_identity(s, "grid", 4);
        FixScene s1; row_scene(s1, 1); check_identity(s1, "one", 1);
        FixScene s2; row_scene(s2, 2); check_identity(s2, "two", 1);
        FixScene s9; row_scene(s9, 9); check_identity(s9, "nine", 1);
    }
    {
        FixScene s;
        grid_scene(s);
        pt::HostScene H;
        if (compile(s, H) != PT_OK) return 1;
        for (int pose = 0; pose < POSE_COUNT; pose++) check_pose(s, H, pose);
        // sequence: A then B is B
        Pose A, B;
        make_pose(s, POSE_SCALE, A);
        make_pose(s, POSE_SINE, B);
        Twin W1, W2;
        twin_of(H, W1);
        twin_of(H, W2);
        twin_update(W1, A);
        CHECK(!same_state(W1, W2));
        twin_update(W1, B);
        twin_update(W2, B);
        CHECK(same_state(W1, W2));
        CHECK(W1.lights.size() == W2.lights.size() && !std::memcmp(W1.lights.data(), W2.lights.data(), W1.lights.size() * sizeof(pt::DevLight)));
        // and back to the rest pose: the compile's bytes again
        Pose R{s.v1, s.v2, s.v3};
        twin_update(W1, R);
        Twin W0;
        twin_of(H, W0);
        CHECK(same_state(W1, W0));
    }
    {   // the lone-leaf root and the nine-triangle root after a move: still boxes of their triangles
        for (int n : {1, 2, 9}) {
            FixScene s;
            row_scene(s, n);
            pt::HostScene H;
            if (compile(s, H) != PT_OK) return 1;
            Twin W;
            twin_of(H, W);
            Pose P;
            make_pose(s, POSE_TRANSLATE, P);
            twin_update(W, P);
            std::vector<int> seen((size_t)W.T.num_nodes, 0);
            const Box all = union_under(W, P, 0, seen);
            for (int ax = 0; ax < 3; ax++) CHECK(W.box[ax] <= all.lo[ax] && W.box[3 + ax] >= all.hi[ax]);
        }
    }
    std::printf("refit_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
