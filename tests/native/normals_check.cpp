// normals_check.cpp — the arithmetic of pt_update_triangles_normals (ptsharp_amd/csrc/pt_normals.h) on the host: a
// CPU twin of pt_normals.hip (the shared functions driven in the kernels' order: a face normal per triangle, a key
// per corner, a stable sort of the corners by key, one normals_segment call per sorted position) on scenes built in
// C++ (scene_fixture.h), the groups taken from the scene compile's table, checked bit for bit against
//   the face normal of pt_obj.cpp   the posed triangles written as an OBJ file without normals and loaded by
//                                   pt_obj_load, whose Triangle.FixNormals fills in the face normal;
//   pt_mesh_smooth_normals          run on each mesh's range of those face normals (NaNs compared by position).
// The scene: a 40x40 grid as two meshes (rows 0-19 and 20-39) that share the seam's positions, a fan of 300
// triangles around one hub (two turns over 150 rim points) as a third mesh, three loose triangles (one before the
// first mesh, one between the two grid meshes, one after the fan).  Poses: translate, scale, sine, huge, tiny, zero-sign (the seam vertex at x = 0
// is -0 in its even triangles and +0 in the odd ones), degenerate (four grid triangles collapsed to a point).
// Also a single triangle as a mesh, and an empty mesh.
// `--dump DIR` writes the group table and every pose's inputs and outputs as raw arrays (tests/normals_ref.py is
// checked against them).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../ptsharp_amd/csrc/pt_normals.h"
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

constexpr int kGrid = 40, kFan = 300;
constexpr int kHalf = kGrid * kGrid;   // triangles of one grid mesh
enum { MAT_GREY = 0, MAT_EMIT = 1 };

static void grid_vertex(int i, int j, float* p) {
    p[0] = (float)i * 0.1f - 2.f;
    p[1] = (float)j * 0.1f - 2.f;
    p[2] = 0.25f * std::cos(1.5f * p[0]) * std::sin(2.f * p[1]);
}
static void grid_rows(FixScene& s, int j0, int j1) {
    for (int j = j0; j < j1; j++)
        for (int i = 0; i < kGrid; i++) {
            float a[3], b[3], c[3], e[3];
            grid_vertex(i, j, a); grid_vertex(i + 1, j, b); grid_vertex(i, j + 1, c); grid_vertex(i + 1, j + 1, e);
            s.triangle(a, b, c, MAT_GREY);
            s.triangle(b, e, c, MAT_GREY);
        }
}
// source order: loose 0 | grid rows 0-19 (mesh 0) | loose 1, emissive | grid rows 20-39 (mesh 1) | the fan (mesh 2) | loose 2
static void normals_scene(FixScene& s) {
    s.material(0.9, 0.9, 0.9, 0);
    s.material(1, 1, 1, 10);
    const float l0[3][3] = {{-3.f, 0.f, 1.f}, {-2.5f, 0.f, 1.f}, {-3.f, 0.5f, 1.2f}};
    const float l1[3][3] = {{0.f, 0.f, 2.f}, {0.5f, 0.f, 2.f}, {0.f, 0.5f, 2.f}};
    const float l2[3][3] = {{3.f, 3.f, -1.f}, {3.5f, 3.f, -1.f}, {3.f, 3.5f, -1.5f}};
    const int t0 = s.triangle(l0[0], l0[1], l0[2], MAT_GREY);
    grid_rows(s, 0, kGrid / 2);
    const int t1 = s.triangle(l1[0], l1[1], l1[2], MAT_EMIT);
    grid_rows(s, kGrid / 2, kGrid);
    const float hub[3] = {3.f, -3.f, 0.5f};
    for (int i = 0; i < kFan; i++) {   // two turns over kFan / 2 rim points: to the next rim point, then to the one after
        const int rim = kFan / 2, at[2] = {i % rim, (i % rim + 1 + i / rim) % rim};
        float r[2][3];
        for (int k = 0; k < 2; k++) {
            const float th = (float)at[k] * (6.2831853f / (float)rim);
            r[k][0] = hub[0] + std::cos(th); r[k][1] = hub[1] + std::sin(th); r[k][2] = hub[2] - 0.3f + 0.2f * std::sin(3.f * th);
        }
        s.triangle(hub, r[0], r[1], MAT_GREY);
    }
    const int t2 = s.triangle(l2[0], l2[1], l2[2], MAT_GREY);
    s.mfirst = {1, 2 + kHalf, 2 + 2 * kHalf}; s.mcount = {kHalf, kHalf, kFan};
    s.shape(PT_SHAPE_TRIANGLE, t0);
    s.shape(PT_SHAPE_MESH, 0);
    s.shape(PT_SHAPE_TRIANGLE, t1);
    s.shape(PT_SHAPE_MESH, 1);
    s.shape(PT_SHAPE_MESH, 2);
    s.shape(PT_SHAPE_TRIANGLE, t2);
    s.shape(PT_SHAPE_SPHERE, s.sphere(0.f, 0.f, 5.f, 0.5, MAT_EMIT));
    s.finish(0);
}

static int compile(FixScene& s, pt::HostScene& H) {
    std::string err;
    const int rc = pt::compile_scene(&s.d, pt::CompileOptions{}, H, err);
    if (rc != PT_OK) std::fprintf(stderr, "compile_scene: %d %s\n", rc, err.c_str());
    return rc;
}

// ---- poses
enum { POSE_TRANSLATE, POSE_SCALE, POSE_SINE, POSE_HUGE, POSE_TINY, POSE_ZERO_SIGN, POSE_DEGENERATE, POSE_COUNT };
static const char* kPoseName[POSE_COUNT] = {"translate", "scale", "sine", "huge", "tiny", "zero-sign", "degenerate"};
static void pose_point(int pose, const float* p, float* q) {
    const float x = p[0], y = p[1], z = p[2];
    switch (pose) {
        case POSE_TRANSLATE: q[0] = x + 1000.f; q[1] = y - 2000.f; q[2] = z + 3000.f; break;
        case POSE_SCALE: q[0] = x * 37.f; q[1] = y * 0.01f; q[2] = z; break;
        case POSE_HUGE: q[0] = x * 1e6f; q[1] = y * 1e6f; q[2] = z * 1e6f; break;
        case POSE_TINY: q[0] = x * 1e-6f; q[1] = y * 1e-6f; q[2] = z * 1e-6f; break;
        default: q[0] = x; q[1] = y; q[2] = z + 0.3f * std::sin(5.f * x) * std::cos(3.f * y); break;   // sine and the two on it
    }
}
struct Pose {
    std::vector<float> v1, v2, v3;
};
static void make_pose(const FixScene& s, int pose, Pose& P) {
    P.v1 = s.v1; P.v2 = s.v2; P.v3 = s.v3;
    std::vector<float>* V[3] = {&P.v1, &P.v2, &P.v3};
    const std::vector<float>* R[3] = {&s.v1, &s.v2, &s.v3};
    for (size_t t = 0; t < s.tm.size(); t++)
        for (int k = 0; k < 3; k++) pose_point(pose, &(*R[k])[3 * t], &(*V[k])[3 * t]);
    if (pose == POSE_ZERO_SIGN) {   // the grid vertex (20, 20), at rest (0, 0, z), shared by three triangles of either mesh
        int flipped = 0, kept = 0;
        for (size_t t = 0; t < s.tm.size(); t++)
            for (int k = 0; k < 3; k++) {
                const float* r = &(*R[k])[3 * t];
                if (r[0] != 0.f || r[1] != 0.f || r[2] >= 1.f) continue;
                if (t % 2 == 0) { (*V[k])[3 * t] = -0.f; flipped++; } else kept++;
            }
        CHECK(flipped >= 2 && kept >= 2);
    }
    if (pose == POSE_DEGENERATE)
        for (size_t t : {(size_t)101, (size_t)102, (size_t)(2 + kHalf + 400), (size_t)(2 + kHalf + 401)})
            for (int k = 0; k < 3; k++) P.v2[3 * t + k] = P.v3[3 * t + k] = P.v1[3 * t + k];
}

// ---- the CPU twin of pt_normals.hip
struct Normals {
    std::vector<float> n1, n2, n3;
};
static void twin_face(const Pose& P, Normals& N) {
    const size_t n = P.v1.size() / 3;
    N.n1.assign(3 * n, 0.f); N.n2 = N.n1; N.n3 = N.n1;
    for (size_t t = 0; t < n; t++) {
        float f[3];
        pt::normals_face(&P.v1[3 * t], &P.v2[3 * t], &P.v3[3 * t], f);
        for (int k = 0; k < 3; k++) N.n1[3 * t + k] = N.n2[3 * t + k] = N.n3[3 * t + k] = f[k];
    }
}
static void twin_smooth(const Pose& P, const std::vector<int32_t>& group, Normals& N) {
    twin_face(P, N);
    const size_t total = P.v1.size();   // 3 corners per triangle
    if (!total) return;
    std::vector<uint32_t> sorted(total);
    std::iota(sorted.begin(), sorted.end(), 0u);
    std::vector<pt::NormalsKey> key(total);
    for (size_t c = 0; c < total; c++) key[c] = pt::normals_key((uint32_t)c, group.data(), P.v1.data(), P.v2.data(), P.v3.data());
    std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return pt::normals_key_less(key[a], key[b]); });
    // the four stable passes over the key words leave this order
    std::vector<uint32_t> lsd(total);
    std::iota(lsd.begin(), lsd.end(), 0u);
    for (int w = 0; w < 4; w++)
        std::stable_sort(lsd.begin(), lsd.end(), [&](uint32_t a, uint32_t b) {
            return pt::normals_key_word(w, a, group.data(), P.v1.data(), P.v2.data(), P.v3.data()) <
                   pt::normals_key_word(w, b, group.data(), P.v1.data(), P.v2.data(), P.v3.data());
        });
    CHECK(lsd == sorted);
    for (size_t i = 0; i < total; i++)
        pt::normals_segment((int64_t)i, (int64_t)total, sorted.data(), group.data(), P.v1.data(), P.v2.data(), P.v3.data(),
                            N.n1.data(), N.n2.data(), N.n3.data());
}

// ---- the references
static bool same_bits(const std::vector<float>& a, const std::vector<float>& b, size_t* nans = nullptr) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) {
        if (std::isnan(a[i]) || std::isnan(b[i])) {
            if (!(std::isnan(a[i]) && std::isnan(b[i]))) return false;
            if (nans) (*nans)++;
            continue;
        }
        if (std::memcmp(&a[i], &b[i], 4)) return false;
    }
    return true;
}
// the face normals pt_obj_load gives the posed triangles (no vn lines: Triangle.FixNormals)
static bool obj_face(const Pose& P, Normals& N) {
    const char* dir = std::getenv("TMPDIR");
    std::string path = std::string(dir && *dir ? dir : "/tmp") + "/normals_check_XXXXXX";
    const int fd = mkstemp(&path[0]);
    if (fd < 0) return false;
    FILE* f = fdopen(fd, "w");
    const size_t n = P.v1.size() / 3;
    for (size_t t = 0; t < n; t++) {
        for (const std::vector<float>* v : {&P.v1, &P.v2, &P.v3})
            std::fprintf(f, "v %.9g %.9g %.9g\n", (double)(*v)[3 * t], (double)(*v)[3 * t + 1], (double)(*v)[3 * t + 2]);
        std::fprintf(f, "f %zu %zu %zu\n", 3 * t + 1, 3 * t + 2, 3 * t + 3);
    }
    std::fclose(f);
    pt_mesh_data m;
    const int rc = pt_obj_load(path.c_str(), &m);
    std::remove(path.c_str());
    if (rc != PT_OK) { std::fprintf(stderr, "pt_obj_load: %s\n", pt_obj_last_error()); return false; }
    bool ok = (size_t)m.num_triangles == n;
    if (ok) {
        ok = !std::memcmp(m.v1, P.v1.data(), n * 12) && !std::memcmp(m.v2, P.v2.data(), n * 12) && !std::memcmp(m.v3, P.v3.data(), n * 12);
        N.n1.assign(m.n1, m.n1 + 3 * n); N.n2.assign(m.n2, m.n2 + 3 * n); N.n3.assign(m.n3, m.n3 + 3 * n);
    }
    pt_mesh_free(&m);
    return ok;
}
// pt_mesh_smooth_normals on each mesh's range of N (face normals on entry)
static bool ref_smooth(const FixScene& s, const Pose& P, Normals& N) {
    for (size_t j = 0; j < s.mfirst.size(); j++) {
        const size_t f = 3 * (size_t)s.mfirst[j];
        if (pt_mesh_smooth_normals(s.mcount[j], P.v1.data() + f, P.v2.data() + f, P.v3.data() + f, N.n1.data() + f, N.n2.data() + f,
                                   N.n3.data() + f) != PT_OK)
            return false;
    }
    return true;
}

template <class T>
static void dump(const std::string& dir, const std::string& name, const T* p, size_t n) {
    const std::string path = dir + "/" + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); failures++; }
    if (f) std::fclose(f);
}

static void check_scene(FixScene& s, const char* what, const std::vector<int>& poses, const std::string& dump_dir) {
    pt::HostScene H;
    if (compile(s, H) != PT_OK) { failures++; return; }
    const std::vector<int32_t>& group = H.refit.tri_group;
    CHECK(group.size() == s.tm.size() && H.refit.num_groups == (int32_t)s.mfirst.size());
    // the group table: the mesh whose range holds the triangle, -1 outside every range
    for (size_t t = 0; t < group.size(); t++) {
        int32_t want = -1;
        for (size_t j = 0; j < s.mfirst.size(); j++)
            if ((int64_t)t >= s.mfirst[j] && (int64_t)t < (int64_t)s.mfirst[j] + s.mcount[j]) want = (int32_t)j;
        CHECK(group[t] == want);
    }
    if (!dump_dir.empty()) {
        dump(dump_dir, "group.i32", group.data(), group.size());
        dump(dump_dir, "mesh_first.i32", s.mfirst.data(), s.mfirst.size());
        dump(dump_dir, "mesh_count.i32", s.mcount.data(), s.mcount.size());
    }
    for (int pose : poses) {
        const int before = failures;
        Pose P;
        make_pose(s, pose, P);
        Normals face, smooth, want_face, want_smooth;
        twin_face(P, face);
        twin_smooth(P, group, smooth);
        CHECK(obj_face(P, want_face));
        size_t face_nans = 0, smooth_nans = 0;
        CHECK(same_bits(face.n1, want_face.n1, &face_nans) && same_bits(face.n2, want_face.n2) && same_bits(face.n3, want_face.n3));
        want_smooth = want_face;
        CHECK(ref_smooth(s, P, want_smooth));
        CHECK(same_bits(smooth.n1, want_smooth.n1, &smooth_nans) && same_bits(smooth.n2, want_smooth.n2, &smooth_nans) &&
              same_bits(smooth.n3, want_smooth.n3, &smooth_nans));
        // loose triangles keep the face normal; a mesh's smooth normals differ from it somewhere
        bool differs = false;
        for (size_t t = 0; t < group.size(); t++) {
            const bool same = !std::memcmp(&smooth.n1[3 * t], &face.n1[3 * t], 12) && !std::memcmp(&smooth.n2[3 * t], &face.n2[3 * t], 12) &&
                              !std::memcmp(&smooth.n3[3 * t], &face.n3[3 * t], 12);
            if (group[t] < 0) CHECK(same);
            else differs = differs || !same;
        }
        CHECK(differs || s.mfirst.empty() || s.tm.size() < 2);
        if (pose == POSE_DEGENERATE) CHECK(face_nans == 4 * 3 && smooth_nans >= 4 * 9 && smooth_nans <= s.tm.size() * 9 / 50);
        else CHECK(face_nans == 0 && smooth_nans == 0);
        if (!dump_dir.empty()) {
            const std::string p = kPoseName[pose];
            dump(dump_dir, p + "_v1.f32", P.v1.data(), P.v1.size()); dump(dump_dir, p + "_v2.f32", P.v2.data(), P.v2.size());
            dump(dump_dir, p + "_v3.f32", P.v3.data(), P.v3.size());
            dump(dump_dir, p + "_face.f32", face.n1.data(), face.n1.size());
            dump(dump_dir, p + "_n1.f32", smooth.n1.data(), smooth.n1.size()); dump(dump_dir, p + "_n2.f32", smooth.n2.data(), smooth.n2.size());
            dump(dump_dir, p + "_n3.f32", smooth.n3.data(), smooth.n3.size());
        }
        std::printf("%s pose %s %s\n", what, kPoseName[pose], failures == before ? "ok" : "FAILED");
    }
}

int main(int argc, char** argv) {
    const std::string dump_dir = argc == 3 && !std::strcmp(argv[1], "--dump") ? argv[2] : "";
    std::vector<int> all;
    for (int p = 0; p < POSE_COUNT; p++) all.push_back(p);
    {
        FixScene s;
        normals_scene(s);
        check_scene(s, "scene", all, dump_dir);
    }
    if (dump_dir.empty()) {
        {   // a single triangle as a mesh: three runs of one corner, every corner its face normal renormalised
            FixScene s;
            s.material(0.9, 0.9, 0.9, 0);
            const float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.75f, 0.f, 0.25f}, c[3] = {0.f, 1.f, 0.5f};
            s.triangle(a, b, c, 0);
            s.mfirst = {0}; s.mcount = {1};
            s.shape(PT_SHAPE_MESH, 0);
            s.finish(0);
            check_scene(s, "single", {POSE_SINE}, "");
        }
        {   // an empty mesh beside a loose triangle, and no triangle at all
            FixScene s;
            s.material(0.9, 0.9, 0.9, 0);
            const float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.75f, 0.f, 0.25f}, c[3] = {0.f, 1.f, 0.5f};
            const int t = s.triangle(a, b, c, 0);
            s.mfirst = {1}; s.mcount = {0};
            s.shape(PT_SHAPE_MESH, 0);
            s.shape(PT_SHAPE_TRIANGLE, t);
            s.finish(0);
            check_scene(s, "empty", {POSE_SINE}, "");
            Pose none;
            Normals N;
            twin_smooth(none, std::vector<int32_t>(), N);
            CHECK(N.n1.empty());
        }
    }
    std::printf("normals_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
