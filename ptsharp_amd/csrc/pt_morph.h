// pt_morph.h — the arithmetic and the packed layout of pt_set_morph / pt_morph_meshes, shared by the device kernel
// (pt_morph.hip), the entry points (pt_api.hip) and the host (tests/native/morph_check.cpp): `PT_HD`, no HIP call,
// compiles with g++.  Build with -ffp-contract=off.
//
// Morph targets (blend shapes) over the rest pose.  The arithmetic of one corner:
//   morph_live     a delta of target t is live when weights[t] != 0 (false only for +-0; a NaN weight is live).  A dead
//                  delta is skipped by a branch: its values are never read into the sum.
//   morph_add      one live delta: per component a = a + (double)w * (double)d.  The product of two widened floats
//                  (24 x 24 significand bits, exponents far inside fp64's range) is exact in fp64, so a fused
//                  multiply-add rounds the same sum: the result does not depend on contraction (the build keeps
//                  -ffp-contract=off anyway).
//   morph_corner   the accumulator starts as (double)p, the rest position, takes the corner's live deltas in ascending
//                  target order, and is converted to fp32 once.  With `normals` the normal is accumulated the same way
//                  from the rest normal and the normal deltas, converted once, then normalised by the fp32 normalize
//                  mat_direction ends in.  A corner with no live delta is copied bit for bit, position and normal.
// The packed layout (morph_pack, morph_unpack): a sliced ELL whose slice is one wave.  Corners are numbered
// corner-major inside, q = c * n + t (c = 0, 1, 2 the corner array, t the triangle), so the 64 lanes of a slice abut
// in v1/v2/v3 and n1/n2/n3.  With S = ceil(n / 64), slice c * S + j holds the triangles 64 j .. 64 j + 63 of corner
// array c; its length len[s] is the largest number of deltas any of its corners has, first[s] (int64) its first step.
// Step k of slice s is entry first[s] + k of three planes, each a whole number of 128-byte lines:
//   target  [steps][64] uint16      128 B per step; kMorphPad (0xFFFF): no delta
//   dpos    [steps][64][3] float    768 B per step
//   dnrm    [steps][64][3] float    768 B per step, when the morph carries normal deltas
// A corner's deltas occupy its lane in steps 0.. in ascending target order; the rest of its lane is padding.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pt_ext.h"

namespace pt {

constexpr int kMorphSlice = 64;            // the lanes of a wave
constexpr uint16_t kMorphPad = 0xFFFF;     // a step's target index where the lane has no delta
constexpr int32_t kMorphMaxTargets = 65535;   // PT_MORPH_MAX_TARGETS: every index below kMorphPad

struct MorphAcc {
    double p[3], n[3];
    bool live;
};
PT_HD bool morph_live(float w) { return w != 0.f; }
PT_HD void morph_begin(MorphAcc& a, const float* p, const float* n) {
    for (int i = 0; i < 3; i++) { a.p[i] = (double)p[i]; a.n[i] = (double)n[i]; }
    a.live = false;
}
// one live delta (dn is read only with `normals`)
PT_HD void morph_add(MorphAcc& a, float w, const float* dp, const float* dn, bool normals) {
    const double wd = (double)w;
    for (int i = 0; i < 3; i++) a.p[i] = a.p[i] + wd * (double)dp[i];
    if (normals) for (int i = 0; i < 3; i++) a.n[i] = a.n[i] + wd * (double)dn[i];
    a.live = true;
}
// p, n: the rest values the accumulator was begun with; without `normals` the normal is copied
PT_HD void morph_end(const MorphAcc& a, bool normals, const float* p, const float* n, float* po, float* no) {
    v3 rp = v3{p[0], p[1], p[2]}, rn = v3{n[0], n[1], n[2]};
    if (a.live) {
        rp = mk(a.p[0], a.p[1], a.p[2]);
        if (normals) rn = normalize(mk(a.n[0], a.n[1], a.n[2]));
    }
    po[0] = rp.x; po[1] = rp.y; po[2] = rp.z;
    no[0] = rn.x; no[1] = rn.y; no[2] = rn.z;
}
// One corner from its `count` deltas in ascending target order: target[k] indexes weights, dpos and dnrm are [count][3]
// (dnrm may be NULL without `normals`).  A corner that is not `moved` (of a loose triangle) is copied bit for bit.
template <class Index>
PT_HD void morph_corner(bool moved, bool normals, const float* weights, int64_t count, const Index* target, const float* dpos,
                        const float* dnrm, const float* p, const float* n, float* po, float* no) {
    MorphAcc a;
    morph_begin(a, p, n);
    if (moved)
        for (int64_t k = 0; k < count; k++) {
            const float w = weights[target[k]];
            if (morph_live(w)) morph_add(a, w, dpos + 3 * k, normals ? dnrm + 3 * k : nullptr, normals);
        }
    morph_end(a, normals, p, n, po, no);
}

// pt_morph_desc's arrays against n triangles: false and *why set for a target_first that does not start at 0 or
// decreases, a corner outside [0, 3n) or not strictly ascending within its target.  target_first is read one entry at
// a time, each checked before the deltas it bounds are read.
inline bool morph_check(int64_t n, int32_t num_targets, const int64_t* target_first, const int32_t* corner, std::string* why) {
    if (num_targets < 1 || num_targets > kMorphMaxTargets) {
        *why = "num_targets is " + std::to_string(num_targets) + ", outside [1, " + std::to_string(kMorphMaxTargets) + "]";
        return false;
    }
    if (target_first[0] != 0) {
        *why = "target_first[0] is " + std::to_string(target_first[0]) + ", not 0";
        return false;
    }
    for (int32_t t = 0; t < num_targets; t++) {
        const int64_t a = target_first[t], b = target_first[t + 1];
        if (b < a) {
            *why = "target_first[" + std::to_string(t + 1) + "] is " + std::to_string(b) + ", below target_first[" + std::to_string(t) + "]";
            return false;
        }
        for (int64_t i = a; i < b; i++) {
            const int64_t q = corner[i];
            if (q < 0 || q >= 3 * n) {
                *why = "corner[" + std::to_string(i) + "] is " + std::to_string(q) + ", outside [0, " + std::to_string(3 * n) + ")";
                return false;
            }
            if (i > a && q <= (int64_t)corner[i - 1]) {
                *why = "corner[" + std::to_string(i) + "] is " + std::to_string(q) + ", not above corner[" + std::to_string(i - 1) +
                       "] of the same target";
                return false;
            }
        }
    }
    return true;
}

// The packed morph of n triangles as the device holds it
struct MorphPacked {
    int64_t n = 0, slices = 0, steps = 0, deltas = 0;   // slices = 3 * ceil(n / 64); steps = the sum of len
    int32_t num_targets = 0;
    bool has_dnrm = false;
    std::vector<int32_t> len;       // [slices]
    std::vector<int64_t> first;     // [slices]
    std::vector<uint16_t> target;   // [steps][64]
    std::vector<float> dpos, dnrm;  // [steps][64][3]; dnrm empty without normal deltas
    int64_t padded() const { return steps * kMorphSlice; }   // the entries held, padding included
};
inline int64_t morph_slices_per_corner(int64_t n) { return (n + kMorphSlice - 1) / kMorphSlice; }

// Arrays that passed morph_check, packed.  dnrm may be NULL.
inline void morph_pack(int64_t n, int32_t num_targets, const int64_t* target_first, const int32_t* corner, const float* dpos,
                       const float* dnrm, MorphPacked& P) {
    const int64_t S = morph_slices_per_corner(n);
    P = MorphPacked{};
    P.n = n;
    P.slices = 3 * S;
    P.num_targets = num_targets;
    P.deltas = target_first[num_targets];
    P.has_dnrm = dnrm != nullptr;
    std::vector<int32_t> used((size_t)(3 * n), 0);   // per inner corner c * n + t: its deltas so far
    const auto inner = [n](int32_t q) { return (int64_t)(q % 3) * n + q / 3; };
    for (int64_t i = 0; i < P.deltas; i++) used[(size_t)inner(corner[i])]++;
    P.len.assign((size_t)P.slices, 0);
    for (int64_t c = 0; c < 3; c++)
        for (int64_t t = 0; t < n; t++) {
            int32_t& l = P.len[(size_t)(c * S + t / kMorphSlice)];
            if (used[(size_t)(c * n + t)] > l) l = used[(size_t)(c * n + t)];
        }
    P.first.assign((size_t)P.slices, 0);
    for (int64_t s = 0; s < P.slices; s++) { P.first[(size_t)s] = P.steps; P.steps += P.len[(size_t)s]; }
    P.target.assign((size_t)P.padded(), kMorphPad);
    P.dpos.assign((size_t)P.padded() * 3, 0.f);
    if (P.has_dnrm) P.dnrm.assign((size_t)P.padded() * 3, 0.f);
    std::fill(used.begin(), used.end(), 0);
    for (int32_t g = 0; g < num_targets; g++)   // ascending targets: a corner's steps come out in target order
        for (int64_t i = target_first[g]; i < target_first[g + 1]; i++) {
            const int64_t c = corner[i] % 3, t = corner[i] / 3;
            const int64_t step = P.first[(size_t)(c * S + t / kMorphSlice)] + used[(size_t)(c * n + t)]++;
            const size_t e = (size_t)(step * kMorphSlice + t % kMorphSlice);
            P.target[e] = (uint16_t)g;
            for (int k = 0; k < 3; k++) {
                P.dpos[3 * e + k] = dpos[3 * i + k];
                if (P.has_dnrm) P.dnrm[3 * e + k] = dnrm[3 * i + k];
            }
        }
}

// The packed planes back in pt_morph_desc's form, bit for bit: target_first [num_targets + 1], corner [deltas], dpos
// and dnrm [deltas][3]; any pointer may be NULL (dnrm is written only when the morph carries normal deltas).  false:
// the planes are not a packed morph (a target at or above num_targets, more deltas than P.deltas).
inline bool morph_unpack(const MorphPacked& P, int64_t* target_first, int32_t* corner, float* dpos, float* dnrm) {
    const int64_t S = morph_slices_per_corner(P.n);
    std::vector<int64_t> at((size_t)P.num_targets + 1, 0);
    // a corner's deltas are its lane's steps up to the first padding; triangle by triangle, corner by corner, the
    // corner numbers 3 t + c ascend, so every target's deltas come out in ascending corner order
    const auto walk = [&](auto&& visit) {
        for (int64_t t = 0; t < P.n; t++)
            for (int64_t c = 0; c < 3; c++) {
                const size_t s = (size_t)(c * S + t / kMorphSlice);
                for (int64_t k = 0; k < P.len[s]; k++) {
                    const size_t e = (size_t)((P.first[s] + k) * kMorphSlice + t % kMorphSlice);
                    if (P.target[e] == kMorphPad) break;
                    if (P.target[e] >= P.num_targets) return false;
                    visit(P.target[e], (int32_t)(3 * t + c), e);
                }
            }
        return true;
    };
    if (!walk([&](uint16_t g, int32_t, size_t) { at[(size_t)g + 1]++; })) return false;
    for (int32_t g = 0; g < P.num_targets; g++) at[(size_t)g + 1] += at[(size_t)g];
    if (at[(size_t)P.num_targets] != P.deltas) return false;
    if (target_first) for (int32_t g = 0; g <= P.num_targets; g++) target_first[g] = at[(size_t)g];
    return walk([&](uint16_t g, int32_t q, size_t e) {
        const int64_t i = at[g]++;
        if (corner) corner[i] = q;
        for (int k = 0; k < 3; k++) {
            if (dpos) dpos[3 * i + k] = P.dpos[3 * e + k];
            if (dnrm && P.has_dnrm) dnrm[3 * i + k] = P.dnrm[3 * e + k];
        }
    });
}
}  // namespace pt
