// morph_check.cpp — ptsharp_amd/csrc/pt_morph.h, the one statement of pt_morph_meshes' arithmetic and of pt_set_morph's
// packed layout, driven on the host.  Each case is a morph in pt_morph_desc's form; it is checked,
// packed, and evaluated twice with pt_morph.h: by morph_corner over the desc's own deltas gathered per corner, and by a
// walk of the packed planes written as the kernel walks them (one lane per corner, a slice's len steps, padding and
// dead targets skipped by a branch, morph_begin / morph_add / morph_end).  Both are compared with a plain restatement
// written here: per component a = (double)p, then a = a + (double)w * (double)d over the corner's live deltas in
// ascending target order, one conversion to fp32, the fp32 Normalize for the normal.  Bit for bit; a NaN matches any NaN.
// Also: unpack(pack(x)) is x bit for bit, the padded entry count is 64 times the sum over slices of the busiest
// corner's deltas (counted here), every step of every plane of the device layout (pt_update_layout.h) starts on a
// 128-byte line, and morph_check refuses each malformed input.
//   morph_check              runs every case, prints "case NAME ok" per case and "morph_check: N failures"
//   morph_check --dump DIR   also writes NAME_group.i32 ([n]: -1 a loose triangle), NAME_first.i64 ([T + 1]),
//                            NAME_corner.i32 ([D]), NAME_dpos.f32 ([D][3]), NAME_dnrm.f32 ([D][3], only with normal
//                            deltas), NAME_weights.f32 ([T]), NAME_in.f32, NAME_out.f32 (normals_mode 0) and
//                            NAME_outp.f32 (normals kept) ([n][18]: V1 V2 V3 N1 N2 N3), for tests/test_morph_host.py
// Build with -ffp-contract=off (morph.mk), also under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "pt_morph.h"
#include "pt_update_layout.h"

namespace {

int g_failures = 0;

uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
bool same(float a, float b) { return (isnan(a) && isnan(b)) || bits(a) == bits(b); }

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 32); }
    double unit() { return next() / 4294967296.0; }               // [0, 1)
    double span(double lo, double hi) { return lo + (hi - lo) * unit(); }
};

struct Case {
    std::string name;
    std::vector<int32_t> group;     // [n]
    std::vector<int64_t> first;     // [T + 1]
    std::vector<int32_t> corner;    // [D]
    std::vector<float> dpos, dnrm;  // [D][3]; dnrm empty: no normal deltas
    std::vector<float> weights;     // [T]
    std::vector<float> in;          // [n][18]
    size_t n() const { return group.size(); }
    int32_t targets() const { return (int32_t)first.size() - 1; }
    const float* dn() const { return dnrm.empty() ? nullptr : dnrm.data(); }
    // one more target: its corners ascending
    void add(const std::vector<int32_t>& q, Rng& r, double scale, bool with_n) {
        if (first.empty()) first.push_back(0);
        for (const int32_t c : q) {
            corner.push_back(c);
            for (int i = 0; i < 3; i++) {
                dpos.push_back((float)r.span(-scale, scale));
                if (with_n) dnrm.push_back((float)r.span(-0.5, 0.5));
            }
        }
        first.push_back((int64_t)corner.size());
    }
};

// The restatement: one corner q from the desc's arrays; v the rest position or normal, d the deltas of that kind
bool ref_sum(const Case& k, int32_t q, const float* d, const float* v, float* out) {
    volatile double ax = v[0], ay = v[1], az = v[2];
    bool live = false;
    for (int32_t t = 0; t < k.targets(); t++) {
        if (k.weights[(size_t)t] == 0.f) continue;   // +-0 only: a NaN compares unequal
        for (int64_t i = k.first[(size_t)t]; i < k.first[(size_t)t + 1]; i++) {
            if (k.corner[(size_t)i] != q) continue;
            const double w = k.weights[(size_t)t];
            volatile double px = w * (double)d[3 * i], py = w * (double)d[3 * i + 1], pz = w * (double)d[3 * i + 2];
            ax = ax + px; ay = ay + py; az = az + pz;
            live = true;
        }
    }
    if (live) { out[0] = (float)ax; out[1] = (float)ay; out[2] = (float)az; }
    return live;
}
// (ref_sum scans every delta per corner; the reference of a large case indexes the deltas by corner first)
struct ByCorner {
    std::vector<std::vector<std::pair<int32_t, int64_t>>> at;   // per corner: (target, delta) ascending by target
    explicit ByCorner(const Case& k) : at(3 * k.n()) {
        for (int32_t t = 0; t < k.targets(); t++)
            for (int64_t i = k.first[(size_t)t]; i < k.first[(size_t)t + 1]; i++) at[(size_t)k.corner[(size_t)i]].push_back({t, i});
    }
};
bool ref_sum_indexed(const Case& k, const ByCorner& B, int32_t q, const float* d, const float* v, float* out) {
    volatile double ax = v[0], ay = v[1], az = v[2];
    bool live = false;
    for (const auto& e : B.at[(size_t)q]) {
        if (k.weights[(size_t)e.first] == 0.f) continue;
        const double w = k.weights[(size_t)e.first];
        const int64_t i = e.second;
        volatile double px = w * (double)d[3 * i], py = w * (double)d[3 * i + 1], pz = w * (double)d[3 * i + 2];
        ax = ax + px; ay = ay + py; az = az + pz;
        live = true;
    }
    if (live) { out[0] = (float)ax; out[1] = (float)ay; out[2] = (float)az; }
    return live;
}
void ref_triangle(const Case& k, const ByCorner& B, size_t t, bool normals, float* out) {
    const float* in = &k.in[18 * t];
    memcpy(out, in, 18 * sizeof(float));
    if (k.group[t] < 0) return;
    for (int c = 0; c < 3; c++) {
        const int32_t q = (int32_t)(3 * t + c);
        const bool scan = k.corner.size() <= 2000;   // small cases: the plain scan, and the index against it
        float p[3];
        const bool live = scan ? ref_sum(k, q, k.dpos.data(), in + 3 * c, p) : ref_sum_indexed(k, B, q, k.dpos.data(), in + 3 * c, p);
        if (scan) {
            float p2[3] = {0, 0, 0};
            const bool live2 = ref_sum_indexed(k, B, q, k.dpos.data(), in + 3 * c, p2);
            if (live2 != live || (live && (!same(p[0], p2[0]) || !same(p[1], p2[1]) || !same(p[2], p2[2])))) {
                printf("  %s: the check's two restatements differ at corner %d\n", k.name.c_str(), q);
                g_failures++;
            }
        }
        if (!live) continue;
        memcpy(out + 3 * c, p, sizeof p);
        if (!normals || k.dnrm.empty()) continue;
        float d[3];
        ref_sum_indexed(k, B, q, k.dnrm.data(), in + 9 + 3 * c, d);
        volatile float xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
        volatile float s = xx + yy;
        s = s + zz;
        const float len = sqrtf(s);
        out[9 + 3 * c] = d[0] / len; out[9 + 3 * c + 1] = d[1] / len; out[9 + 3 * c + 2] = d[2] / len;
    }
}

// pt_morph.h's morph_corner over the desc's deltas gathered per corner
void header_triangle(const Case& k, const ByCorner& B, size_t t, bool normals, float* out) {
    const float* in = &k.in[18 * t];
    const bool blend = normals && !k.dnrm.empty();
    for (int c = 0; c < 3; c++) {
        const auto& list = B.at[3 * t + c];
        std::vector<int32_t> target;
        std::vector<float> dp, dn;
        for (const auto& e : list) {
            target.push_back(e.first);
            for (int i = 0; i < 3; i++) {
                dp.push_back(k.dpos[3 * (size_t)e.second + i]);
                if (blend) dn.push_back(k.dnrm[3 * (size_t)e.second + i]);
            }
        }
        pt::morph_corner(k.group[t] >= 0, blend, k.weights.data(), (int64_t)target.size(), target.data(), dp.data(),
                         blend ? dn.data() : nullptr, in + 3 * c, in + 9 + 3 * c, out + 3 * c, out + 9 + 3 * c);
    }
}

// The packed planes walked as k_morph_meshes walks them: slice s = c * S + t / 64, lane t % 64
void packed_triangles(const Case& k, const pt::MorphPacked& P, bool normals, std::vector<float>& out) {
    const int64_t n = (int64_t)k.n(), S = pt::morph_slices_per_corner(n);
    const bool blend = normals && P.has_dnrm;
    for (int64_t s = 0; s < P.slices; s++)
        for (int lane = 0; lane < pt::kMorphSlice; lane++) {
            const int64_t c = s / S, t = (s - c * S) * pt::kMorphSlice + lane;
            if (t >= n) continue;
            const float* in = &k.in[18 * (size_t)t];
            pt::MorphAcc acc;
            pt::morph_begin(acc, in + 3 * c, in + 9 + 3 * c);
            if (k.group[(size_t)t] >= 0)
                for (int64_t step = 0; step < P.len[(size_t)s]; step++) {
                    const size_t e = (size_t)((P.first[(size_t)s] + step) * pt::kMorphSlice + lane);
                    const uint16_t g = P.target[e];
                    if (g == pt::kMorphPad) continue;
                    const float w = k.weights[g];
                    if (!pt::morph_live(w)) continue;
                    pt::morph_add(acc, w, &P.dpos[3 * e], blend ? &P.dnrm[3 * e] : nullptr, blend);
                }
            pt::morph_end(acc, blend, in + 3 * c, in + 9 + 3 * c, &out[18 * (size_t)t + 3 * c], &out[18 * (size_t)t + 9 + 3 * c]);
        }
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
std::vector<int32_t> all_corners(size_t n) {
    std::vector<int32_t> q(3 * n);
    for (size_t i = 0; i < q.size(); i++) q[i] = (int32_t)i;
    return q;
}
// a seeded ascending subset of the corners: each with probability p
std::vector<int32_t> some_corners(Rng& r, size_t n, double p) {
    std::vector<int32_t> q;
    for (size_t i = 0; i < 3 * n; i++) if (r.unit() < p) q.push_back((int32_t)i);
    return q;
}
void seeded_weights(Rng& r, Case& k) {
    k.weights.resize((size_t)k.targets());
    for (float& w : k.weights) w = r.unit() < 0.3 ? (r.next() & 1 ? 0.f : -0.f) : (float)r.span(-1.0, 1.5);
    k.weights[0] = 0.75f;
}

std::vector<Case> cases() {
    std::vector<Case> out;
    Rng r{0x9E3779B97F4A7C15ull};
    const float inf = std::numeric_limits<float>::infinity(), qnan = std::numeric_limits<float>::quiet_NaN();
    // seeded: the slice boundaries (1, 63, 64, 65, 257) and 3,208 = 50 * 64 + 8; every 13th triangle loose, with deltas
    const size_t counts[6] = {1, 63, 64, 65, 257, 3208};
    const int target_counts[6] = {3, 5, 8, 8, 40, 300};
    for (int c = 0; c < 6; c++) {
        Case k;
        k.name = "seeded" + std::to_string(c);
        const size_t n = counts[c];
        k.in = seeded_triangles(r, n, c == 5 ? 1000.0 : 4.0);
        k.group.assign(n, 0);
        for (size_t t = 5; t < n; t += 13) k.group[t] = -1;
        for (int t = 0; t < target_counts[c]; t++) k.add(some_corners(r, n, t == 0 ? 0.9 : t % 7 == 3 ? 0.0 : 0.5 / (1 + t % 5)), r, 0.3, true);
        seeded_weights(r, k);
        out.push_back(k);
    }
    // no normal deltas: the normals are the rest's
    {
        Case k;
        k.name = "no-dnrm";
        k.in = seeded_triangles(r, 200, 4.0);
        k.group.assign(200, 0);
        k.group[17] = -1;
        for (int t = 0; t < 12; t++) k.add(some_corners(r, 200, 0.3), r, 0.3, false);
        seeded_weights(r, k);
        out.push_back(k);
    }
    // 128 triangles: corner array 0's first slice has one corner with 40 deltas beside 63 with none (all padding but
    // one lane), its second slice one delta on every corner; array 1 holds corners with 0, 1 and 5 deltas in one slice;
    // array 2 has no delta at all (two slices of length 0)
    {
        Case k;
        k.name = "lengths";
        k.in = seeded_triangles(r, 128, 4.0);
        k.group.assign(128, 0);
        for (int t = 0; t < 40; t++) {
            std::vector<int32_t> q{3 * 9};                                        // triangle 9, corner 0
            if (t == 0) for (int32_t j = 64; j < 128; j++) q.push_back(3 * j);    // the second slice, once
            if (t < 5) q.push_back(3 * 20 + 1);                                   // triangle 20, corner 1: five deltas
            if (t == 7) q.push_back(3 * 21 + 1);                                  // triangle 21, corner 1: one
            std::sort(q.begin(), q.end());
            k.add(q, r, 0.3, true);
        }
        k.weights.assign(40, 0.f);
        for (int t = 0; t < 40; t++) k.weights[(size_t)t] = (float)r.span(0.1, 1.0);
        out.push_back(k);
    }
    // the highest target index, an empty target and a target touching every corner
    {
        Case k;
        k.name = "targets";
        k.in = seeded_triangles(r, 70, 4.0);
        k.group.assign(70, 0);
        k.add(all_corners(70), r, 0.3, true);
        k.add({}, r, 0.3, true);
        k.first.resize((size_t)pt::kMorphMaxTargets, k.first.back());   // targets 2 .. 65533: empty
        k.add({0, 100, 209}, r, 0.3, true);                              // target 65534
        k.weights.assign((size_t)k.targets(), 0.25f);
        k.weights[0] = 1.f;
        k.weights.back() = -2.f;
        out.push_back(k);
    }
    // every weight +0 or -0: the rest values verbatim, -0 positions kept
    {
        Case k;
        k.name = "zero-weights";
        k.in = seeded_triangles(r, 200, 4.0);
        k.group.assign(200, 0);
        for (size_t t = 0; t < 200; t += 7) { k.in[18 * t + 1] = -0.f; k.in[18 * t + 8] = -0.f; }
        for (int t = 0; t < 9; t++) k.add(some_corners(r, 200, 0.6), r, 0.3, true);
        k.weights.assign(9, 0.f);
        for (size_t t = 0; t < 9; t += 2) k.weights[t] = -0.f;
        out.push_back(k);
    }
    // a weight of -0 among live ones: its target is dead, although its deltas are huge
    {
        Case k;
        k.name = "neg-zero-weight";
        k.in = seeded_triangles(r, 100, 4.0);
        k.group.assign(100, 0);
        k.add(some_corners(r, 100, 0.5), r, 0.3, true);
        k.add(all_corners(100), r, 1e20, true);
        k.add(some_corners(r, 100, 0.5), r, 0.3, true);
        k.weights = {0.5f, -0.f, 1.25f};
        out.push_back(k);
    }
    // a NaN weight is live: the corners of its target are NaN, position and normal, the others are not
    {
        Case k;
        k.name = "nan-weight";
        k.in = seeded_triangles(r, 100, 4.0);
        k.group.assign(100, 0);
        k.add(some_corners(r, 100, 0.5), r, 0.3, true);
        std::vector<int32_t> q;
        for (int32_t j = 0; j < 25; j++) q.push_back(12 * j + j % 3);
        k.add(q, r, 0.3, true);
        k.weights = {0.5f, qnan};
        out.push_back(k);
    }
    // non-finite deltas on dead targets only: skipped by the branch, the result is finite
    {
        Case k;
        k.name = "dead-nonfinite";
        k.in = seeded_triangles(r, 150, 4.0);
        k.group.assign(150, 0);
        for (int t = 0; t < 6; t++) k.add(some_corners(r, 150, 0.5), r, 0.3, true);
        k.weights = {0.5f, 0.f, 1.f, -0.f, -0.75f, 0.f};
        for (int t = 1; t < 6; t += 2)
            for (int64_t i = 3 * k.first[(size_t)t]; i < 3 * k.first[(size_t)t + 1]; i++) {
                k.dpos[(size_t)i] = i % 3 == 0 ? inf : i % 3 == 1 ? -inf : qnan;
                k.dnrm[(size_t)i] = i % 3 == 0 ? qnan : inf;
            }
        out.push_back(k);
    }
    // denormal deltas (alone they vanish in the fp64 sum's conversion, or survive on a zero position) and a 1e30 delta
    {
        Case k;
        k.name = "denormal-far";
        k.in = seeded_triangles(r, 60, 4.0);
        k.group.assign(60, 0);
        for (size_t t = 0; t < 60; t += 3) for (int i = 0; i < 9; i++) k.in[18 * t + i] = (i % 2) ? 0.f : -0.f;
        k.add(all_corners(60), r, 0.3, true);
        k.add(some_corners(r, 60, 0.3), r, 0.3, true);
        k.add(some_corners(r, 60, 0.3), r, 0.3, true);
        const float special[4] = {1.4e-45f, -1.4e-45f, 1.1e-38f, -5.9e-39f};
        for (size_t i = 0; i < 3 * (size_t)k.first[1]; i++) k.dpos[i] = special[i % 4];
        for (int64_t i = 3 * k.first[2]; i < 3 * k.first[3]; i++) k.dpos[(size_t)i] = (i % 2) ? 1e30f : -1e30f;
        k.weights = {1.f, 0.5f, 3.f};
        out.push_back(k);
    }
    // a zero-length resulting normal: rest normal (0, 0, 1), delta (0, 0, -1), weight 1: 0 / 0, as Normalize gives
    {
        Case k;
        k.name = "zero-normal";
        k.in = seeded_triangles(r, 10, 4.0);
        k.group.assign(10, 0);
        for (size_t t = 0; t < 10; t++) for (int q = 3; q < 6; q++) { k.in[18 * t + 3 * q] = 0.f; k.in[18 * t + 3 * q + 1] = 0.f; k.in[18 * t + 3 * q + 2] = 1.f; }
        k.add(all_corners(10), r, 0.3, true);
        for (size_t i = 0; i < k.dnrm.size(); i++) k.dnrm[i] = i % 3 == 2 ? -1.f : 0.f;
        k.weights = {1.f};
        out.push_back(k);
    }
    return out;
}

void dump(const std::string& path, const void* p, size_t bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || (bytes && fwrite(p, 1, bytes, f) != bytes)) { printf("cannot write %s\n", path.c_str()); g_failures++; }
    if (f) fclose(f);
}

// morph_check refuses each malformed input, and says which
void refusals() {
    int bad = 0;
    const int64_t n = 10;
    const std::vector<int64_t> first{0, 3, 3, 6};
    const std::vector<int32_t> corner{0, 4, 29, 1, 2, 3};
    std::string why;
    const auto refused = [&](const char* what, int32_t targets, std::vector<int64_t> f, std::vector<int32_t> q, const char* word) {
        why.clear();
        if (pt::morph_check(n, targets, f.data(), q.data(), &why) || why.find(word) == std::string::npos) {
            printf("  refusals: %s was %s (%s)\n", what, why.empty() ? "accepted" : "refused without the word", why.c_str());
            bad++;
        }
    };
    if (!pt::morph_check(n, 3, first.data(), corner.data(), &why)) { printf("  refusals: the well-formed morph was refused: %s\n", why.c_str()); bad++; }
    refused("no targets", 0, first, corner, "num_targets");
    refused("negative targets", -1, first, corner, "num_targets");
    refused("65536 targets", 65536, first, corner, "num_targets");
    refused("target_first[0] = 1", 3, {1, 3, 3, 6}, corner, "target_first[0]");
    refused("target_first decreasing", 3, {0, 3, 2, 6}, corner, "below");
    refused("target_first decreasing at the end", 3, {0, 3, 3, 2}, corner, "below");
    refused("a bad corner at position 0", 3, first, {-1, 4, 29, 1, 2, 3}, "outside");
    refused("a corner of 3n at position 0", 3, first, {30, 4, 29, 1, 2, 3}, "outside");
    refused("a bad corner at the last delta", 3, first, {0, 4, 29, 1, 2, 30}, "outside");
    refused("a negative corner at the last delta", 3, first, {0, 4, 29, 1, 2, -5}, "outside");
    refused("a duplicate corner within a target", 3, first, {0, 4, 4, 1, 2, 3}, "not above");
    refused("a descending corner within a target", 3, first, {0, 4, 29, 1, 3, 2}, "not above");
    // ascending only within a target: the next target may start lower (the well-formed one does), and with no triangle
    // every corner is outside
    why.clear();
    const std::vector<int64_t> one{0, 1};
    const std::vector<int32_t> zero{0};
    if (pt::morph_check(0, 1, one.data(), zero.data(), &why)) { printf("  refusals: a corner of a scene with no triangle was accepted\n"); bad++; }
    const std::vector<int64_t> none{0, 0};
    if (!pt::morph_check(0, 1, none.data(), zero.data(), &why)) { printf("  refusals: an empty morph was refused\n"); bad++; }
    if (bad) g_failures++;
    else printf("case refusals ok\n");
}

}  // namespace

int main(int argc, char** argv) {
    std::string dir;
    if (argc == 3 && !strcmp(argv[1], "--dump")) dir = argv[2];
    refusals();
    for (const Case& k : cases()) {
        const size_t n = k.n();
        int bad = 0;
        std::string why;
        if (!pt::morph_check((int64_t)n, k.targets(), k.first.data(), k.corner.data(), &why)) {
            printf("  %s: refused: %s\n", k.name.c_str(), why.c_str());
            g_failures++;
            continue;
        }
        pt::MorphPacked P;
        pt::morph_pack((int64_t)n, k.targets(), k.first.data(), k.corner.data(), k.dpos.data(), k.dn(), P);
        const ByCorner B(k);
        // the padded count, counted here: per slice of 64 triangles of one corner array, its busiest corner
        const int64_t S = ((int64_t)n + 63) / 64;
        int64_t steps = 0;
        for (int64_t c = 0; c < 3; c++)
            for (int64_t j = 0; j < S; j++) {
                size_t most = 0;
                for (int64_t t = 64 * j; t < 64 * (j + 1) && t < (int64_t)n; t++) most = std::max(most, B.at[(size_t)(3 * t + c)].size());
                if (P.len[(size_t)(c * S + j)] != (int32_t)most || P.first[(size_t)(c * S + j)] != steps) {
                    if (bad++ < 5) printf("  %s: slice %lld has len %d first %lld, counted %zu and %lld\n", k.name.c_str(), (long long)(c * S + j),
                                          P.len[(size_t)(c * S + j)], (long long)P.first[(size_t)(c * S + j)], most, (long long)steps);
                }
                steps += (int64_t)most;
            }
        if (P.slices != 3 * S || P.steps != steps || P.padded() != 64 * steps || P.deltas != (int64_t)k.corner.size() ||
            (int64_t)P.target.size() != 64 * steps || (int64_t)P.dpos.size() != 192 * steps ||
            (int64_t)P.dnrm.size() != (k.dnrm.empty() ? 0 : 192 * steps)) {
            printf("  %s: %lld slices, %lld steps, %lld padded entries; counted %lld, %lld, %lld\n", k.name.c_str(), (long long)P.slices,
                   (long long)P.steps, (long long)P.padded(), (long long)(3 * S), (long long)steps, (long long)(64 * steps));
            bad++;
        }
        // every entry is a delta or padding, and there are exactly `deltas` of the former
        int64_t held = 0;
        for (const uint16_t g : P.target) held += g != pt::kMorphPad;
        if (held != P.deltas) { printf("  %s: the planes hold %lld deltas of %lld\n", k.name.c_str(), (long long)held, (long long)P.deltas); bad++; }
        // the device layout: every step of every plane on a 128-byte line
        const pt::MorphDev L = pt::morph_layout(P.slices, P.steps, P.has_dnrm, P.num_targets, nullptr);
        for (int64_t s = 0; s < steps; s++) {
            const uintptr_t a = (uintptr_t)(L.target + 64 * s), b = (uintptr_t)(L.dpos + 192 * s), c = P.has_dnrm ? (uintptr_t)(L.dnrm + 192 * s) : 0;
            if ((a % 128 || b % 128 || c % 128) && bad++ < 5) printf("  %s: step %lld of a plane is not on a 128-byte line\n", k.name.c_str(), (long long)s);
        }
        if ((uintptr_t)L.len % 128 || (uintptr_t)L.first % 128 || (uintptr_t)L.weights % 128 || (P.has_dnrm != (L.dnrm != nullptr))) {
            printf("  %s: the layout's parts are misplaced\n", k.name.c_str());
            bad++;
        }
        // unpack(pack(x)) == x, bit for bit
        {
            std::vector<int64_t> first(k.first.size(), -1);
            std::vector<int32_t> corner(k.corner.size(), -1);
            std::vector<float> dpos(k.dpos.size(), 7.f), dnrm(k.dnrm.size(), 8.f);
            if (!pt::morph_unpack(P, first.data(), corner.data(), dpos.data(), dnrm.empty() ? nullptr : dnrm.data())) { printf("  %s: unpack refused the planes\n", k.name.c_str()); bad++; }
            const auto same_bits = [](const std::vector<float>& x, const std::vector<float>& y) {
                return x.size() == y.size() && (x.empty() || !memcmp(x.data(), y.data(), x.size() * sizeof(float)));
            };
            if (first != k.first || corner != k.corner || !same_bits(dpos, k.dpos) || !same_bits(dnrm, k.dnrm)) {
                printf("  %s: unpack(pack(x)) differs from x\n", k.name.c_str());
                bad++;
            }
            pt::MorphPacked broken = P;
            if (!broken.target.empty()) {
                for (uint16_t& g : broken.target) if (g != pt::kMorphPad) { g = (uint16_t)k.targets(); break; }
                if (held && k.targets() < pt::kMorphMaxTargets && pt::morph_unpack(broken, nullptr, nullptr, nullptr, nullptr)) {
                    printf("  %s: unpack accepted a target index of num_targets\n", k.name.c_str());
                    bad++;
                }
            }
        }
        std::vector<float> morphed[2];
        for (int normals = 0; normals < 2; normals++) {
            std::vector<float> got(18 * n, 7.f), walked(18 * n, 8.f), want(18 * n, 9.f);
            for (size_t t = 0; t < n; t++) {
                header_triangle(k, B, t, normals != 0, &got[18 * t]);
                ref_triangle(k, B, t, normals != 0, &want[18 * t]);
            }
            packed_triangles(k, P, normals != 0, walked);
            for (size_t i = 0; i < got.size(); i++) {
                if (!same(got[i], want[i]) && bad++ < 5)
                    printf("  %s normals=%d triangle %zu float %zu: got %a (%08x), want %a (%08x)\n", k.name.c_str(), normals, i / 18, i % 18,
                           got[i], bits(got[i]), want[i], bits(want[i]));
                if (!same(walked[i], got[i]) && bad++ < 5)
                    printf("  %s normals=%d triangle %zu float %zu: the walk of the packed planes differs\n", k.name.c_str(), normals, i / 18, i % 18);
                // kept values are verbatim, NaN payloads and zero signs included: a loose triangle, a corner with no live
                // delta, and every normal when the normals are not blended
                const size_t t = i / 18, c = i % 9 / 3;
                bool live = false;
                for (const auto& e : B.at[3 * t + c]) live = live || k.weights[(size_t)e.first] != 0.f;
                const bool kept = k.group[t] < 0 || !live || ((!normals || k.dnrm.empty()) && i % 18 >= 9);
                if (kept && (bits(got[i]) != bits(k.in[i]) || bits(walked[i]) != bits(k.in[i])) && bad++ < 5)
                    printf("  %s: float %zu of a kept value changed\n", k.name.c_str(), i);
            }
            morphed[normals] = got;
        }
        const std::vector<float>& full = morphed[1];
        // what each case is there for
        size_t nan_normals = 0, nan_positions = 0, changed = 0, neg_zero = 0, loose_with_deltas = 0;
        for (size_t i = 0; i < full.size(); i++) {
            if (i % 18 >= 9) { nan_normals += isnan(full[i]); continue; }
            nan_positions += isnan(full[i]);
            changed += bits(full[i]) != bits(k.in[i]);
            neg_zero += bits(full[i]) == 0x80000000u;
        }
        for (size_t t = 0; t < n; t++) if (k.group[t] < 0) for (int c = 0; c < 3; c++) loose_with_deltas += !B.at[3 * t + c].empty();
        int32_t most = 0;
        for (const int32_t l : P.len) most = std::max(most, l);
        if (k.name.rfind("seeded", 0) == 0 && n > 13 && (loose_with_deltas == 0 || changed < full.size() / 8)) {
            printf("  %s: %zu loose corners with deltas, %zu position floats moved\n", k.name.c_str(), loose_with_deltas, changed);
            bad++;
        }
        if (k.name == "lengths") {
            // slice 0: 40 steps for one lane; slice 1: one step, full; corner array 1's first slice: five; the rest empty
            const int32_t want_len[6] = {40, 1, 5, 0, 0, 0};
            for (int s = 0; s < 6; s++) if (P.len[(size_t)s] != want_len[s]) { printf("  lengths: slice %d has len %d\n", s, P.len[(size_t)s]); bad++; }
            int64_t pad0 = 0;
            for (int64_t e = 0; e < 40 * 64; e++) pad0 += P.target[(size_t)e] == pt::kMorphPad;
            if (pad0 != 40 * 63 || P.padded() != 46 * 64) { printf("  lengths: %lld padding entries in slice 0, %lld entries in all\n", (long long)pad0, (long long)P.padded()); bad++; }
        }
        if (k.name == "targets") {
            bool top = false;
            for (const uint16_t g : P.target) top = top || g == 65534;
            if (!top || k.targets() != 65535 || most != 2) { printf("  targets: the highest index is %s, %d targets, longest slice %d\n", top ? "held" : "missing", k.targets(), most); bad++; }
        }
        if (k.name == "zero-weights" && (changed != 0 || neg_zero == 0 || memcmp(full.data(), k.in.data(), full.size() * 4))) {
            printf("  zero-weights: %zu floats changed, %zu are -0\n", changed, neg_zero);
            bad++;
        }
        if (k.name == "neg-zero-weight") {
            for (size_t i = 0; i < full.size(); i++) if (i % 18 < 9 && fabsf(full[i]) > 100.f) { printf("  neg-zero-weight: the dead target moved float %zu\n", i); bad++; break; }
        }
        if (k.name == "nan-weight" && (nan_positions != 25 * 3 || nan_normals != 25 * 3)) {
            printf("  nan-weight: %zu NaN position floats and %zu NaN normal floats, expected 75 and 75\n", nan_positions, nan_normals);
            bad++;
        }
        if (k.name == "zero-normal" && (nan_normals != 90 || nan_positions != 0)) { printf("  zero-normal: %zu NaN normal floats of 90\n", nan_normals); bad++; }
        if (k.name == "denormal-far") {
            size_t tiny = 0, far = 0;
            for (size_t i = 0; i < full.size(); i++) if (i % 18 < 9) { tiny += full[i] != 0.f && fabsf(full[i]) < 1.2e-38f; far += fabsf(full[i]) > 1e29f; }
            if (tiny == 0 || far == 0) { printf("  denormal-far: %zu denormal results, %zu far ones\n", tiny, far); bad++; }
        }
        if (k.name != "nan-weight" && k.name != "zero-normal" && nan_normals + nan_positions != 0) {
            printf("  %s: %zu NaN floats\n", k.name.c_str(), nan_normals + nan_positions);
            bad++;
        }
        if (bad) g_failures++;
        else printf("case %s ok\n", k.name.c_str());
        if (!dir.empty()) {
            dump(dir + "/" + k.name + "_group.i32", k.group.data(), k.group.size() * sizeof(int32_t));
            dump(dir + "/" + k.name + "_first.i64", k.first.data(), k.first.size() * sizeof(int64_t));
            dump(dir + "/" + k.name + "_corner.i32", k.corner.data(), k.corner.size() * sizeof(int32_t));
            dump(dir + "/" + k.name + "_dpos.f32", k.dpos.data(), k.dpos.size() * sizeof(float));
            if (!k.dnrm.empty()) dump(dir + "/" + k.name + "_dnrm.f32", k.dnrm.data(), k.dnrm.size() * sizeof(float));
            dump(dir + "/" + k.name + "_weights.f32", k.weights.data(), k.weights.size() * sizeof(float));
            dump(dir + "/" + k.name + "_in.f32", k.in.data(), k.in.size() * sizeof(float));
            dump(dir + "/" + k.name + "_out.f32", full.data(), full.size() * sizeof(float));
            dump(dir + "/" + k.name + "_outp.f32", morphed[0].data(), morphed[0].size() * sizeof(float));
        }
    }
    printf("morph_check: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
