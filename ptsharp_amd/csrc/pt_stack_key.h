// pt_stack_key.h — keyed traversal-stack entries of the triangle BVH: a pushed child keeps the
// top K bits of its entry distance, so a pop can cull it against the bound the ray has by then.  Plain
// C++ with no HIP header: the kernels (pt_device.h node8_step, pt_wavefront.hip trace_lanes), the scene compile
// (which picks K), tests/native/stack_key_check.cpp and tools/bvh_quality.cpp share these definitions.
//
// Entry: leaf << 31 | keyK << idx_bits | index, with K + idx_bits = 31.  keyK = tn_bits >> idx_bits, the top K
// bits of the 31-bit pattern of the non-negative fp32 entry distance tn (ordered as integers), rounded down.
// Since keyK << idx_bits is tn_bits with its low idx_bits bits cleared, the whole format is one mask:
//     key_mask = 0x7FFFFFFF & ~(2^idx_bits - 1)      (0 at K = 0: the entry is the bare ref)
//     entry    = ref | (tn_bits & key_mask)
//     ref      = entry & ~key_mask
// Pop-time cull: keyK > (bits(tmax * 1.0000005f) >> idx_bits), which for a key field that is a multiple of
// 2^idx_bits is (entry & key_mask) > bits(tmax * 1.0000005f) as unsigned integers (a negative bound has
// bit 31 set and culls nothing).  The bound is the node test's own (tn <= tf * 1.0000005f with tf <= tmax) and
// the key is rounded down, so a culled entry is one its parent's test would have missed under the current bound.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_KEY_HD __host__ __device__
#else
#define PT_KEY_HD
#endif

namespace pt {

constexpr int kStackKeyMaxBits = 15;   // 8 exponent + 7 mantissa bits: a longer key culls no more

PT_KEY_HD inline uint32_t stack_f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// Bits an index below `count` needs: the smallest b with count <= 2^b.
PT_KEY_HD inline int stack_idx_bits(uint64_t count) {
    int b = 0;
    while (b < 63 && (1ull << b) < count) b++;
    return b;
}
// K for a triangle BVH of `nodes` nodes and `chunks` leaf chunks, at most `cap` (0: no key, nothing culled).
PT_KEY_HD inline int stack_key_choose(uint64_t nodes, uint64_t chunks, int cap) {
    const int ib = stack_idx_bits(nodes > chunks ? nodes : chunks);
    int k = 31 - ib;
    if (k > kStackKeyMaxBits) k = kStackKeyMaxBits;
    if (k > cap) k = cap;
    return k < 0 ? 0 : k;
}
PT_KEY_HD inline uint32_t stack_key_mask(int K) { return K <= 0 ? 0u : (0x7FFFFFFFu & ~((1u << (31 - K)) - 1u)); }
PT_KEY_HD inline uint32_t stack_entry(uint32_t ref, uint32_t tn_bits, uint32_t key_mask) { return ref | (tn_bits & key_mask); }
PT_KEY_HD inline uint32_t stack_entry_ref(uint32_t entry, uint32_t key_mask) { return entry & ~key_mask; }
// The cull bound of a ray whose fp32 bound is tmax: the node test's widened far distance, as bits.
PT_KEY_HD inline uint32_t stack_bound_bits(float tmax) { return stack_f32_bits(tmax * 1.0000005f); }
PT_KEY_HD inline bool stack_entry_culled(uint32_t entry, uint32_t key_mask, uint32_t bound_bits) {
    return (entry & key_mask) > bound_bits;
}

}  // namespace pt
