// pose_check.cpp — ptsharp_amd/csrc/pt_pose.h's pose_triangle, the one statement of pt_pose_meshes' arithmetic, driven
// on the host against a plain restatement of Matrix.MulPosition / MulDirection (Matrix.cs:134-150) written here: fp64
// products summed left to right, one conversion to fp32, the fp32 Normalize.  Bit for bit; a NaN matches any NaN.
//   pose_check              runs every case, prints "case NAME ok" per case and "pose_check: N failures"
//   pose_check --dump DIR   also writes NAME_matrix.f64 (16), NAME_in.f32 and NAME_out.f32 ([n][18]: V1 V2 V3 N1 N2 N3;
//                           out is the moved pose with normals), for tests/test_pose_host.py's numpy comparison
// Build with -ffp-contract=off (pose.mk), also under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "pt_pose.h"

namespace {

int g_failures = 0;

uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
bool same(float a, float b) { return (isnan(a) && isnan(b)) || bits(a) == bits(b); }

// Matrix.MulPosition (Matrix.cs:134-141)
void ref_position(const double* m, const float* b, float* out) {
    const double bx = b[0], by = b[1], bz = b[2];
    volatile double x = m[0] * bx, y = m[4] * bx, z = m[8] * bx;
    x = x + m[1] * by; y = y + m[5] * by; z = z + m[9] * by;
    x = x + m[2] * bz; y = y + m[6] * bz; z = z + m[10] * bz;
    x = x + m[3]; y = y + m[7]; z = z + m[11];
    out[0] = (float)x; out[1] = (float)y; out[2] = (float)z;
}
// Matrix.MulDirection (Matrix.cs:144-150): the products, then Vector.Normalize in fp32
void ref_direction(const double* m, const float* b, float* out) {
    const double bx = b[0], by = b[1], bz = b[2];
    volatile double x = m[0] * bx, y = m[4] * bx, z = m[8] * bx;
    x = x + m[1] * by; y = y + m[5] * by; z = z + m[9] * by;
    x = x + m[2] * bz; y = y + m[6] * bz; z = z + m[10] * bz;
    const float fx = (float)x, fy = (float)y, fz = (float)z;
    volatile float xx = fx * fx, yy = fy * fy, zz = fz * fz;
    volatile float s = xx + yy;
    s = s + zz;
    const float len = sqrtf(s);
    out[0] = fx / len; out[1] = fy / len; out[2] = fz / len;
}
void ref_triangle(const double* m, bool moved, bool normals, const float* in, float* out) {
    memcpy(out, in, 18 * sizeof(float));
    if (!moved) return;
    for (int k = 0; k < 3; k++) ref_position(m, in + 3 * k, out + 3 * k);
    if (normals)
        for (int k = 3; k < 6; k++) ref_direction(m, in + 3 * k, out + 3 * k);
}

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 32); }
    double unit() { return next() / 4294967296.0; }               // [0, 1)
    double span(double lo, double hi) { return lo + (hi - lo) * unit(); }
};

struct Case {
    std::string name;
    double m[16];
    std::vector<float> in;   // [n][18]
};

void identity(double* m) { for (int i = 0; i < 16; i++) m[i] = (i % 5 == 0) ? 1.0 : 0.0; }

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

std::vector<Case> cases() {
    std::vector<Case> out;
    Rng r{0x9E3779B97F4A7C15ull};
    // seeded: general affine matrices (rotation-like, sheared, non-uniformly scaled, translated), ragged counts
    const size_t counts[4] = {1, 257, 1000, 3208};
    for (int c = 0; c < 4; c++) {
        Case k;
        k.name = "seeded" + std::to_string(c);
        identity(k.m);
        for (int i = 0; i < 12; i++) k.m[i] = (i % 4 == 3) ? r.span(-10, 10) : r.span(-2, 2);
        k.in = seeded_triangles(r, counts[c], c == 3 ? 1000.0 : 4.0);
        out.push_back(k);
    }
    // -0, +0 and denormals in every slot, under a general matrix
    {
        Case k;
        k.name = "zeros-denormals";
        identity(k.m);
        for (int i = 0; i < 12; i++) k.m[i] = (i % 4 == 3) ? 0.0 : r.span(-2, 2);
        const float special[6] = {-0.f, 0.f, 1.4e-45f, -1.4e-45f, 1.1e-38f, -5.9e-39f};
        for (int a = 0; a < 6; a++)
            for (int b = 0; b < 6; b++) {
                float tri[18];
                for (int i = 0; i < 18; i++) tri[i] = special[(a + b * i) % 6];
                tri[3] = 1.f;   // one ordinary component, so that not every posed vector is a zero
                tri[12] = 0.5f;
                k.in.insert(k.in.end(), tri, tri + 18);
            }
        out.push_back(k);
    }
    // a translation of 1e30: positions lose every rest bit, directions are untouched by it
    {
        Case k;
        k.name = "far";
        identity(k.m);
        k.m[3] = 1e30; k.m[7] = -1e30; k.m[11] = 3e38;
        k.in = seeded_triangles(r, 300, 4.0);
        out.push_back(k);
    }
    // a singular matrix (rank 1; the last 40 triangles under the zero matrix' kernel: normals along z give 0 / 0)
    {
        Case k;
        k.name = "singular";
        identity(k.m);
        const double row[4] = {0.5, -1.25, 0.0, 2.0};
        for (int i = 0; i < 12; i++) k.m[i] = row[i % 4] * (1 + i / 4);
        k.in = seeded_triangles(r, 200, 4.0);
        for (size_t t = 160; t < 200; t++)
            for (int q = 3; q < 6; q++) { k.in[18 * t + 3 * q] = 0.f; k.in[18 * t + 3 * q + 1] = 0.f; k.in[18 * t + 3 * q + 2] = q == 4 ? -1.f : 1.f; }
        out.push_back(k);
    }
    // identity: the rest values as values; -0 becomes +0 (x + 0 * y + 0 * z + 0)
    {
        Case k;
        k.name = "identity";
        identity(k.m);
        k.in = seeded_triangles(r, 200, 4.0);
        for (size_t t = 0; t < 200; t += 7) { k.in[18 * t + 1] = -0.f; k.in[18 * t + 8] = -0.f; }
        out.push_back(k);
    }
    return out;
}

void compare(const Case& k, bool moved, bool normals, const std::vector<float>& got, const std::vector<float>& want, int& bad) {
    for (size_t i = 0; i < got.size(); i++)
        if (!same(got[i], want[i])) {
            if (bad++ < 5)
                printf("  %s moved=%d normals=%d triangle %zu float %zu: got %a (%08x), want %a (%08x)\n", k.name.c_str(), (int)moved,
                       (int)normals, i / 18, i % 18, got[i], bits(got[i]), want[i], bits(want[i]));
        }
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
        const size_t n = k.in.size() / 18;
        int bad = 0;
        std::vector<float> posed;
        for (int moved = 0; moved < 2; moved++)
            for (int normals = 0; normals < 2; normals++) {
                std::vector<float> got(18 * n, 7.f), want(18 * n, 9.f);
                for (size_t t = 0; t < n; t++) {
                    pt::pose_triangle(k.m, moved, normals, &k.in[18 * t], &got[18 * t]);
                    ref_triangle(k.m, moved, normals, &k.in[18 * t], &want[18 * t]);
                }
                compare(k, moved, normals, got, want, bad);
                // not moved: verbatim, NaN payloads and zero signs included; moved without normals: the normals verbatim
                for (size_t i = 0; i < got.size(); i++)
                    if ((!moved || (!normals && i % 18 >= 9)) && bits(got[i]) != bits(k.in[i])) {
                        if (bad++ < 5) printf("  %s: float %zu of a kept value changed\n", k.name.c_str(), i);
                    }
                if (moved && normals) posed = got;
            }
        // what each case is there for
        size_t nan_normals = 0, flipped = 0, changed = 0;
        for (size_t i = 0; i < posed.size(); i++) {
            if (i % 18 >= 9 && isnan(posed[i])) nan_normals++;
            if (i % 18 >= 9) continue;   // positions from here on (an identity still renormalises the normals)
            if (bits(k.in[i]) == 0x80000000u && bits(posed[i]) == 0u) flipped++;
            if (bits(k.in[i]) != bits(posed[i])) changed++;
        }
        if (k.name == "singular" && nan_normals != 40 * 9) { printf("  singular: %zu NaN normal floats, expected 360\n", nan_normals); bad++; }
        if (k.name != "singular" && k.name != "zeros-denormals" && nan_normals != 0) {   // (a zero normal stays a 0 / 0)
            printf("  %s: %zu NaN normal floats\n", k.name.c_str(), nan_normals);
            bad++;
        }
        if (k.name == "identity" && (flipped == 0 || changed != flipped)) {
            printf("  identity: %zu position floats changed, %zu of them -0 to +0\n", changed, flipped);
            bad++;
        }
        if (k.name.rfind("seeded", 0) == 0 && changed < posed.size() / 4) { printf("  %s: only %zu position floats moved\n", k.name.c_str(), changed); bad++; }
        if (bad) g_failures++;
        else printf("case %s ok\n", k.name.c_str());
        if (!dir.empty()) {
            dump(dir + "/" + k.name + "_matrix.f64", k.m, sizeof k.m);
            dump(dir + "/" + k.name + "_in.f32", k.in.data(), k.in.size() * sizeof(float));
            dump(dir + "/" + k.name + "_out.f32", posed.data(), posed.size() * sizeof(float));
        }
    }
    printf("pose_check: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
