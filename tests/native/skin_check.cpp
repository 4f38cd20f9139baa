// skin_check.cpp — ptsharp_amd/csrc/pt_skin.h's skin_triangle, the one statement of pt_skin_meshes' arithmetic, driven
// on the host against a plain restatement of the blend written here: per live influence, in ascending
// order, the fp64 sums of Matrix.MulPosition / MulDirection (Matrix.cs:134-150) times the weight as a double, the
// first live term taken as the accumulator and the others added, one conversion to fp32, the fp32 Normalize.  Bit for
// bit; a NaN matches any NaN.  skin_triangle runs twice per case, as the kernel instantiates it: 32-bit indices over
// the caller's [B][16] matrices, and 16-bit indices over a packed [B][12] table.
//   skin_check              runs every case, prints "case NAME ok" per case and "skin_check: N failures"
//   skin_check --dump DIR   also writes NAME_matrices.f64 ([B][16]), NAME_group.i32 ([n]: -1 a loose triangle),
//                           NAME_bones.i32 and NAME_weights.f32 ([n][3][4]), NAME_in.f32, NAME_out.f32 (normals blended)
//                           and NAME_outp.f32 (normals kept) ([n][18]: V1 V2 V3 N1 N2 N3), for tests/test_skin_host.py
// Build with -ffp-contract=off (skin.mk), also under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "pt_pose.h"
#include "pt_skin.h"

namespace {

int g_failures = 0;

uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
bool same(float a, float b) { return (isnan(a) && isnan(b)) || bits(a) == bits(b); }

// One corner, restated: v is the rest position (translate) or the rest normal
bool ref_blend(const double* mats, const int32_t* b, const float* w, const float* v, bool translate, float* out) {
    volatile double ax = 0, ay = 0, az = 0;
    bool live = false;
    for (int k = 0; k < 4; k++) {
        if (w[k] == 0.f) continue;   // +-0 only: a NaN compares unequal
        const double* m = mats + 16 * (size_t)b[k];
        const double vx = v[0], vy = v[1], vz = v[2];
        volatile double x = m[0] * vx, y = m[4] * vx, z = m[8] * vx;
        x = x + m[1] * vy; y = y + m[5] * vy; z = z + m[9] * vy;
        x = x + m[2] * vz; y = y + m[6] * vz; z = z + m[10] * vz;
        if (translate) { x = x + m[3]; y = y + m[7]; z = z + m[11]; }
        const double wk = w[k];
        x = wk * x; y = wk * y; z = wk * z;
        if (live) { ax = ax + x; ay = ay + y; az = az + z; }
        else { ax = x; ay = y; az = z; }
        live = true;
    }
    if (live) { out[0] = (float)ax; out[1] = (float)ay; out[2] = (float)az; }
    return live;
}
void ref_triangle(const double* mats, bool moved, bool normals, const int32_t* bones, const float* weights, const float* in, float* out) {
    memcpy(out, in, 18 * sizeof(float));
    if (!moved) return;
    for (int c = 0; c < 3; c++) {
        if (!ref_blend(mats, bones + 4 * c, weights + 4 * c, in + 3 * c, true, out + 3 * c)) continue;
        if (!normals) continue;
        float d[3];
        ref_blend(mats, bones + 4 * c, weights + 4 * c, in + 9 + 3 * c, false, d);
        volatile float xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
        volatile float s = xx + yy;
        s = s + zz;
        const float len = sqrtf(s);
        out[9 + 3 * c] = d[0] / len; out[9 + 3 * c + 1] = d[1] / len; out[9 + 3 * c + 2] = d[2] / len;
    }
}

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 32); }
    double unit() { return next() / 4294967296.0; }               // [0, 1)
    double span(double lo, double hi) { return lo + (hi - lo) * unit(); }
};

struct Case {
    std::string name;
    std::vector<double> mats;      // [B][16]
    std::vector<int32_t> group;    // [n]
    std::vector<int32_t> bones;    // [n][12]
    std::vector<float> weights;    // [n][12]
    std::vector<float> in;         // [n][18]
    size_t n() const { return group.size(); }
    int32_t num_bones() const { return (int32_t)(mats.size() / 16); }
};

void identity(double* m) { for (int i = 0; i < 16; i++) m[i] = (i % 5 == 0) ? 1.0 : 0.0; }

std::vector<double> seeded_matrices(Rng& r, int count) {
    std::vector<double> m(16 * (size_t)count);
    for (int b = 0; b < count; b++) {
        identity(&m[16 * (size_t)b]);
        for (int i = 0; i < 12; i++) m[16 * (size_t)b + i] = (i % 4 == 3) ? r.span(-10, 10) : r.span(-2, 2);
    }
    return m;
}

std::vector<float> seeded_triangles(Rng& r, size_t n, double extent) {
    std::vector<float> in(18 * n);
    for (size_t t = 0; t < n; t++) {
        for (int i = 0; i < 9; i++) in[18 * t + i] = (float)r.span(-extent, extent);
        for (int k = 3; k < 6; k++) {   // unit normals, as an upload holds them
            float v[3] = {(float)r.span(-1, 1), (float)r.span(-1, 1), (float)r.span(-1, 1)};
            const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            for (int i = 0; i < 3; i++) in[18 * t + 3 * k + i] = len > 0 ? v[i] / len : (i == 0 ? 1.f : 0.f);
        }
    }
    return in;
}

// n triangles of one mesh, every corner with 1 to 4 live influences at seeded slots (the dead ones +0 or -0)
void seeded_skin(Rng& r, Case& k, size_t n) {
    k.group.assign(n, 0);
    k.bones.resize(12 * n);
    k.weights.resize(12 * n);
    for (size_t q = 0; q < 3 * n; q++) {
        const int live = 1 + (int)(r.next() % 4);
        bool on[4] = {false, false, false, false};
        for (int placed = 0; placed < live;) {
            const int s = (int)(r.next() % 4);
            if (!on[s]) { on[s] = true; placed++; }
        }
        for (int s = 0; s < 4; s++) {
            k.bones[4 * q + s] = (int32_t)(r.next() % (uint32_t)k.num_bones());
            k.weights[4 * q + s] = on[s] ? (float)r.span(0.05, 1.0) : (r.next() & 1 ? 0.f : -0.f);
        }
    }
}

// one live influence of weight `w` per corner, at slot (corner index % 4); the other slots dead
void single_skin(Rng& r, Case& k, size_t n, float w) {
    k.group.assign(n, 0);
    k.bones.resize(12 * n);
    k.weights.assign(12 * n, 0.f);
    for (size_t q = 0; q < 3 * n; q++) {
        for (int s = 0; s < 4; s++) k.bones[4 * q + s] = (int32_t)(r.next() % (uint32_t)k.num_bones());
        k.weights[4 * q + q % 4] = w;
    }
}

std::vector<Case> cases() {
    std::vector<Case> out;
    Rng r{0x9E3779B97F4A7C15ull};
    const double inf = std::numeric_limits<double>::infinity();
    // seeded: general affine matrices, 1 to 4 live influences per corner, ragged counts; every 13th triangle loose
    const size_t counts[4] = {1, 257, 1000, 3208};
    const int bone_counts[4] = {1, 7, 40, 300};
    for (int c = 0; c < 4; c++) {
        Case k;
        k.name = "seeded" + std::to_string(c);
        k.mats = seeded_matrices(r, bone_counts[c]);
        k.in = seeded_triangles(r, counts[c], c == 3 ? 1000.0 : 4.0);
        seeded_skin(r, k, counts[c]);
        for (size_t t = 5; t < counts[c]; t += 13) k.group[t] = -1;
        out.push_back(k);
    }
    // every weight +0 or -0: the rest values verbatim, -0 positions kept
    {
        Case k;
        k.name = "zero-weights";
        k.mats = seeded_matrices(r, 5);
        k.in = seeded_triangles(r, 200, 4.0);
        seeded_skin(r, k, 200);
        for (size_t i = 0; i < k.weights.size(); i++) k.weights[i] = (i % 3 == 0) ? -0.f : 0.f;
        for (size_t t = 0; t < 200; t += 7) { k.in[18 * t + 1] = -0.f; k.in[18 * t + 8] = -0.f; }
        out.push_back(k);
    }
    // one live influence of weight 1: pose_triangle with that bone's matrix, bit for bit
    {
        Case k;
        k.name = "single-one";
        k.mats = seeded_matrices(r, 9);
        k.in = seeded_triangles(r, 300, 4.0);
        single_skin(r, k, 300, 1.f);
        out.push_back(k);
    }
    // 0.5 + 0.5 on one bone: the same as weight 1 (away from the denormals)
    {
        Case k;
        k.name = "half-half";
        k.mats = seeded_matrices(r, 9);
        k.in = seeded_triangles(r, 300, 4.0);
        single_skin(r, k, 300, 0.5f);
        for (size_t q = 0; q < 3 * 300; q++) {
            const size_t a = q % 4, b = (q + 1 + q / 4 % 3) % 4;
            k.weights[4 * q + b] = 0.5f;
            k.bones[4 * q + b] = k.bones[4 * q + a];
        }
        out.push_back(k);
    }
    // -0, +0 and denormals in every slot, blended
    {
        Case k;
        k.name = "zeros-denormals";
        k.mats = seeded_matrices(r, 4);
        for (size_t b = 0; b < 4; b++) for (int i = 3; i < 12; i += 4) k.mats[16 * b + i] = 0.0;
        const float special[6] = {-0.f, 0.f, 1.4e-45f, -1.4e-45f, 1.1e-38f, -5.9e-39f};
        for (int a = 0; a < 6; a++)
            for (int b = 0; b < 6; b++) {
                float tri[18];
                for (int i = 0; i < 18; i++) tri[i] = special[(a + b * i) % 6];
                tri[3] = 1.f;   // one ordinary component, so that not every skinned vector is a zero
                tri[12] = 0.5f;
                k.in.insert(k.in.end(), tri, tri + 18);
            }
        seeded_skin(r, k, 36);
        out.push_back(k);
    }
    // -0 survives: a matrix of -0 over positive positions sums to -0, and the accumulator is that first term, not
    // +0 plus it (which would be +0); the normals are 0 / 0
    {
        Case k;
        k.name = "minus-zero";
        k.mats.assign(16, -0.0);
        k.in = seeded_triangles(r, 20, 4.0);
        for (size_t t = 0; t < 20; t++) for (int i = 0; i < 9; i++) k.in[18 * t + i] = fabsf(k.in[18 * t + i]) + 0.5f;
        single_skin(r, k, 20, 0.75f);
        out.push_back(k);
    }
    // a translation of 1e30 on some bones: positions lose every rest bit, directions are untouched by it
    {
        Case k;
        k.name = "far";
        k.mats = seeded_matrices(r, 6);
        for (size_t b = 0; b < 6; b += 2) { k.mats[16 * b + 3] = 1e30; k.mats[16 * b + 7] = -1e30; k.mats[16 * b + 11] = 3e38; }
        k.in = seeded_triangles(r, 300, 4.0);
        seeded_skin(r, k, 300);
        out.push_back(k);
    }
    // singular matrices (rank 1, all bones alike; the last 40 triangles' normals along z lie in the kernel: 0 / 0)
    {
        Case k;
        k.name = "singular";
        k.mats.assign(16 * 3, 0.0);
        const double row[4] = {0.5, -1.25, 0.0, 2.0};
        for (size_t b = 0; b < 3; b++) {
            identity(&k.mats[16 * b]);
            for (int i = 0; i < 12; i++) k.mats[16 * b + i] = row[i % 4] * (1 + i / 4) * (double)(b + 1);
        }
        k.in = seeded_triangles(r, 200, 4.0);
        for (size_t t = 160; t < 200; t++)
            for (int q = 3; q < 6; q++) { k.in[18 * t + 3 * q] = 0.f; k.in[18 * t + 3 * q + 1] = 0.f; k.in[18 * t + 3 * q + 2] = q == 4 ? -1.f : 1.f; }
        seeded_skin(r, k, 200);
        out.push_back(k);
    }
    // a NaN weight is live: its corner's position and normal are NaN, its neighbours' are not
    {
        Case k;
        k.name = "nan-weight";
        k.mats = seeded_matrices(r, 5);
        k.in = seeded_triangles(r, 100, 4.0);
        seeded_skin(r, k, 100);
        for (size_t t = 0; t < 100; t += 4) {   // corner t % 3, slot t % 4; the other slots of that corner dead
            const size_t q = 3 * t + t % 3;
            for (int s = 0; s < 4; s++) k.weights[4 * q + s] = 0.f;
            k.weights[4 * q + t % 4] = std::numeric_limits<float>::quiet_NaN();
        }
        out.push_back(k);
    }
    // non-finite matrices on dead influences only: never read, the result is that of finite ones
    {
        Case k;
        k.name = "dead-nonfinite";
        k.mats = seeded_matrices(r, 8);
        for (size_t b = 4; b < 8; b++) for (int i = 0; i < 16; i++) k.mats[16 * b + i] = (i % 3 == 0) ? inf : (i % 3 == 1) ? -inf : (double)NAN;
        k.in = seeded_triangles(r, 300, 4.0);
        seeded_skin(r, k, 300);
        for (size_t i = 0; i < k.bones.size(); i++) k.bones[i] = k.bones[i] % 4 + (k.weights[i] == 0.f ? 4 : 0);
        out.push_back(k);
    }
    return out;
}

void dump(const std::string& path, const void* p, size_t bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) { printf("cannot write %s\n", path.c_str()); g_failures++; }
    if (f) fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
    std::string dir;
    if (argc == 3 && !strcmp(argv[1], "--dump")) dir = argv[2];
    for (const Case& k : cases()) {
        const size_t n = k.n();
        int bad = 0;
        // the kernel's other instantiation: 16-bit indices over the packed 12-double rows
        std::vector<uint16_t> bones16(k.bones.begin(), k.bones.end());
        std::vector<double> rows12(12 * (size_t)k.num_bones());
        for (size_t b = 0; b < (size_t)k.num_bones(); b++) memcpy(&rows12[12 * b], &k.mats[16 * b], 12 * sizeof(double));
        std::vector<float> skinned[2];
        for (int normals = 0; normals < 2; normals++) {
            std::vector<float> got(18 * n, 7.f), got16(18 * n, 8.f), want(18 * n, 9.f);
            for (size_t t = 0; t < n; t++) {
                const bool moved = k.group[t] >= 0;
                pt::skin_triangle(k.mats.data(), 16, moved, normals != 0, &k.bones[12 * t], &k.weights[12 * t], &k.in[18 * t], &got[18 * t]);
                pt::skin_triangle(rows12.data(), 12, moved, normals != 0, &bones16[12 * t], &k.weights[12 * t], &k.in[18 * t], &got16[18 * t]);
                ref_triangle(k.mats.data(), moved, normals != 0, &k.bones[12 * t], &k.weights[12 * t], &k.in[18 * t], &want[18 * t]);
            }
            for (size_t i = 0; i < got.size(); i++) {
                if (!same(got[i], want[i]) && bad++ < 5)
                    printf("  %s normals=%d triangle %zu float %zu: got %a (%08x), want %a (%08x)\n", k.name.c_str(), normals, i / 18,
                           i % 18, got[i], bits(got[i]), want[i], bits(want[i]));
                if (!same(got16[i], got[i]) && bad++ < 5)
                    printf("  %s normals=%d triangle %zu float %zu: the packed instantiation differs\n", k.name.c_str(), normals, i / 18, i % 18);
                // kept values are verbatim, NaN payloads and zero signs included: a loose triangle, a corner with no live
                // influence, and every normal when the normals are not blended
                const size_t t = i / 18, c = i % 9 / 3;
                bool live = false;
                for (int s = 0; s < 4; s++) live = live || k.weights[12 * t + 4 * c + s] != 0.f;
                const bool kept = k.group[t] < 0 || !live || (!normals && i % 18 >= 9);
                if (kept && bits(got[i]) != bits(k.in[i]) && bad++ < 5) printf("  %s: float %zu of a kept value changed\n", k.name.c_str(), i);
            }
            skinned[normals] = got;
        }
        const std::vector<float>& full = skinned[1];
        // what each case is there for
        size_t nan_normals = 0, nan_positions = 0, changed = 0, neg_zero = 0;
        for (size_t i = 0; i < full.size(); i++) {
            if (i % 18 >= 9) { nan_normals += isnan(full[i]); continue; }
            nan_positions += isnan(full[i]);
            changed += bits(full[i]) != bits(k.in[i]);
            neg_zero += bits(full[i]) == 0x80000000u;
        }
        if (k.name == "zero-weights" && (changed != 0 || neg_zero == 0)) { printf("  zero-weights: %zu floats changed, %zu are -0\n", changed, neg_zero); bad++; }
        if (k.name == "single-one" || k.name == "half-half") {
            // Mesh.Transform by the corner's bone: pt_pose.h's pose_triangle, taken corner by corner
            for (size_t t = 0; t < n; t++)
                for (size_t c = 0; c < 3; c++) {
                    const size_t q = 3 * t + c;
                    float posed[18];
                    pt::pose_triangle(&k.mats[16 * (size_t)k.bones[4 * q + q % 4]], true, true, &k.in[18 * t], posed);
                    for (size_t i = 0; i < 3; i++)
                        if ((!same(full[18 * t + 3 * c + i], posed[3 * c + i]) || !same(full[18 * t + 9 + 3 * c + i], posed[9 + 3 * c + i])) && bad++ < 5)
                            printf("  %s: triangle %zu corner %zu differs from pose_triangle\n", k.name.c_str(), t, c);
                }
        }
        if (k.name == "minus-zero" && neg_zero != 9 * n) { printf("  minus-zero: %zu of %zu position floats are -0\n", neg_zero, 9 * n); bad++; }
        if (k.name == "singular" && nan_normals < 40 * 9) { printf("  singular: %zu NaN normal floats, expected at least 360\n", nan_normals); bad++; }
        if (k.name == "nan-weight" && (nan_positions != 25 * 3 || nan_normals != 25 * 3)) {
            printf("  nan-weight: %zu NaN position floats and %zu NaN normal floats, expected 75 and 75\n", nan_positions, nan_normals);
            bad++;
        }
        if (k.name != "singular" && k.name != "nan-weight" && k.name != "zeros-denormals" && k.name != "minus-zero" && k.name != "far" &&
            nan_normals + nan_positions != 0) {
            printf("  %s: %zu NaN floats\n", k.name.c_str(), nan_normals + nan_positions);
            bad++;
        }
        if (k.name.rfind("seeded", 0) == 0 && n > 1 && changed < full.size() / 4) { printf("  %s: only %zu position floats moved\n", k.name.c_str(), changed); bad++; }
        if (bad) g_failures++;
        else printf("case %s ok\n", k.name.c_str());
        if (!dir.empty()) {
            dump(dir + "/" + k.name + "_matrices.f64", k.mats.data(), k.mats.size() * sizeof(double));
            dump(dir + "/" + k.name + "_group.i32", k.group.data(), k.group.size() * sizeof(int32_t));
            dump(dir + "/" + k.name + "_bones.i32", k.bones.data(), k.bones.size() * sizeof(int32_t));
            dump(dir + "/" + k.name + "_weights.f32", k.weights.data(), k.weights.size() * sizeof(float));
            dump(dir + "/" + k.name + "_in.f32", k.in.data(), k.in.size() * sizeof(float));
            dump(dir + "/" + k.name + "_out.f32", full.data(), full.size() * sizeof(float));
            dump(dir + "/" + k.name + "_outp.f32", skinned[0].data(), skinned[0].size() * sizeof(float));
        }
    }
    printf("skin_check: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
