// stack_key_check.cpp — the keyed stack entries of ptsharp_amd/csrc/pt_stack_key.h on the host:
//   * for K = 1..15 the packed pop-time compare never culls an entry the exact test tn > tmax * 1.0000005f keeps
//     (10^7 random pairs of non-negative floats per K, and the ends: 0, denormals, neighbours one ulp apart,
//     FLT_MAX, +inf), and it does cull where the truncated keys differ (so it is not vacuous);
//   * pack then unpack returns the leaf bit and the index, for the largest index every idx_bits allows;
//   * the host's choice of K never overlaps the leaf bit or the index, for counts 1, 2^k - 1, 2^k, 2^k + 1 up to 2^29;
//   * K = 0 entries are the bare refs.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../ptsharp_amd/csrc/pt_stack_key.h"

static long failures = 0;
#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) {                                                                   \
            if (++failures <= 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                                             \
    } while (0)

static float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// node8_step's key of a hit slot: the entry distance's bits without the sign, the slot in the low 3 bits
static uint32_t node_key(float tn, uint32_t slot) { return (pt::stack_f32_bits(tn) & 0x7FFFFFF8u) | slot; }

static long culled_total = 0;
static void pair(int K, float tn, float tmax, uint32_t ref) {
    const uint32_t km = pt::stack_key_mask(K);
    const uint32_t e = pt::stack_entry(ref, node_key(tn, ref & 7u), km);
    const bool cull = pt::stack_entry_culled(e, km, pt::stack_bound_bits(tmax));
    const bool exact = tn > tmax * 1.0000005f;
    if (cull) {
        culled_total++;
        CHECK(exact);
    }
    // the longhand form of the format: keyK > bound >> (31 - K)
    const uint32_t keyK = (node_key(tn, 0u) & 0x7FFFFFFFu) >> (31 - K);
    const uint32_t bb = pt::stack_bound_bits(tmax);
    if (!(bb >> 31)) CHECK(cull == (keyK > (bb >> (31 - K))));
    CHECK(pt::stack_entry_ref(e, km) == ref);
}

static void check_compare() {
    std::mt19937_64 rng(20240607);
    std::vector<float> ends = {0.0f, -0.0f, from_bits(1u), from_bits(2u), from_bits(0x007FFFFFu), FLT_MIN, 1e-30f, 1e-6f,
                               0.5f, 1.0f, from_bits(0x3F800001u), 1.0000005f, 2.0f, 3.0f, 1e6f, 1e30f,
                               from_bits(0x7F7FFFFEu), FLT_MAX, INFINITY};
    for (int K = 1; K <= pt::kStackKeyMaxBits; K++) {
        const long before = culled_total;
        const int idx_bits = 31 - K;
        const uint32_t idx_max = (idx_bits >= 32 ? 0xFFFFFFFFu : (1u << idx_bits) - 1u) & 0x1FFFFFFFu;
        for (long n = 0; n < 10000000; n++) {
            const uint64_t r = rng();
            uint32_t a = (uint32_t)r & 0x7FFFFFFFu, b = (uint32_t)(r >> 32) & 0x7FFFFFFFu;
            if (a > 0x7F800000u) a = 0x7F800000u;   // no NaN: an entry distance and a bound are never one
            if (b > 0x7F800000u) b = 0x7F800000u;
            if (n & 1) b = a + ((uint32_t)(r >> 20) & 0x3FFFFu) - 0x20000u;   // near pairs: within 2^17 ulp
            if (b > 0x7F800000u) b = 0x7F800000u;
            const uint32_t ref = ((n & 2) ? 0x80000000u : 0u) | ((uint32_t)(r >> 7) & idx_max);
            pair(K, from_bits(a), from_bits(b), ref);
        }
        for (float x : ends)
            for (float y : ends) {
                pair(K, x, y, idx_max);
                pair(K, x, y, 0x80000000u | idx_max);
            }
        for (float x : ends) {   // values one ulp apart, both ways, and across a key step
            const uint32_t u = pt::stack_f32_bits(x) & 0x7FFFFFFFu;
            if (u == 0u || u >= 0x7F800000u) continue;
            pair(K, from_bits(u + 1u), from_bits(u), 5u);
            pair(K, from_bits(u), from_bits(u + 1u), 5u);
            pair(K, from_bits(u - 1u), from_bits(u), 5u);
            const uint32_t step = 1u << (31 - K), up = (u | (step - 1u)) + 1u;   // the next key's first value
            if (up < 0x7F800000u) {
                pair(K, from_bits(up), from_bits(up - 1u), 5u);
                pair(K, from_bits(up), from_bits(u), 5u);
            }
        }
        pair(K, 1.0f, -1.0f, 3u);   // a negative bound culls nothing (the kernels never have one)
        CHECK(!pt::stack_entry_culled(pt::stack_entry(3u, node_key(1.0f, 3u), pt::stack_key_mask(K)), pt::stack_key_mask(K),
                                      pt::stack_bound_bits(-1.0f)));
        CHECK(culled_total - before > 1000000);   // the packed compare does cull
        std::printf("K %2d ok: %ld culled\n", K, culled_total - before);
    }
}

static void check_pack() {
    for (int idx_bits = 0; idx_bits <= 29; idx_bits++) {
        const uint64_t count = 1ull << idx_bits;
        CHECK(pt::stack_idx_bits(count) == idx_bits);
        const int K = pt::stack_key_choose(count, 1, pt::kStackKeyMaxBits);
        const uint32_t km = pt::stack_key_mask(K), idx = (uint32_t)(count - 1u);
        for (uint32_t leaf : {0u, 0x80000000u})
            for (uint32_t key : {0u, 0x7FFFFFF8u, 0xFFFFFFFFu, 0x3F800000u}) {
                const uint32_t e = pt::stack_entry(leaf | idx, key, km);
                CHECK(pt::stack_entry_ref(e, km) == (leaf | idx));
                CHECK((e & 0x80000000u) == leaf);
                CHECK((e & 0x1FFFFFFFu & ~km) == idx);
            }
    }
    CHECK(pt::stack_key_mask(12) == 0x7FF80000u && pt::stack_key_mask(15) == 0x7FFF0000u && pt::stack_key_mask(1) == 0x40000000u);
}

static void check_choice() {
    auto one = [](uint64_t count) {
        for (int cap : {0, 1, 4, 12, 15, 31})
            for (int side = 0; side < 2; side++) {
                const int K = side ? pt::stack_key_choose(count, 1, cap) : pt::stack_key_choose(1, count, cap);
                const uint32_t km = pt::stack_key_mask(K);
                CHECK(K >= 0 && K <= pt::kStackKeyMaxBits && K <= cap);
                CHECK(!(km & 0x80000000u));                    // not the leaf bit
                CHECK(!(km & (uint32_t)(count - 1u)));         // not the largest index
                CHECK(count - 1u <= (uint64_t)(0x7FFFFFFFu & ~km));
                CHECK(__builtin_popcount(km) == K);
                const int want = 31 - pt::stack_idx_bits(count);
                CHECK(K == (want < cap ? (want < 15 ? want : 15) : (cap < 15 ? cap : 15)));
            }
    };
    one(1);
    for (int k = 1; k <= 29; k++) {
        one((1ull << k) - 1u);
        one(1ull << k);
        if (k < 29) one((1ull << k) + 1u);
    }
    CHECK(pt::stack_idx_bits(1) == 0 && pt::stack_idx_bits(2) == 1 && pt::stack_idx_bits(3) == 2 && pt::stack_idx_bits(4) == 2 &&
          pt::stack_idx_bits(5) == 3);
    CHECK(pt::stack_key_choose(250000, 493000, 15) == 12);   // the 1M-triangle frame: 19 index bits
    CHECK(pt::stack_key_choose(1u << 29, 1, 15) == 2);
}

static void check_k0() {
    const uint32_t km = pt::stack_key_mask(0);
    CHECK(km == 0u);
    std::mt19937 rng(5);
    for (int n = 0; n < 100000; n++) {
        const uint32_t ref = rng(), key = rng();
        CHECK(pt::stack_entry(ref, key, km) == ref);
        CHECK(pt::stack_entry_ref(ref, km) == ref);
        CHECK(!pt::stack_entry_culled(ref, km, rng()));
    }
    CHECK(pt::stack_key_choose(100, 100, 0) == 0 && pt::stack_key_choose(100, 100, -3) == 0);
}

int main() {
    check_compare();
    check_pack();
    check_choice();
    check_k0();
    std::printf("stack_key_check: %ld failures\n", failures);
    return failures ? 1 : 0;
}
