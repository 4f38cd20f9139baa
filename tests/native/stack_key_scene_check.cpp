// stack_key_scene_check.cpp — the scene compile's choice of the stack entries' key field (DevScene::stack_key_mask,
// pt_scene_compile.cpp Compiler::lines) on compiled scenes: it is pt_stack_key.h's choice for the scene's node and
// chunk counts under every CompileOptions::pop_cull_bits, it never covers the leaf flag or an index the scene
// has, and no ref stored in the triangle BVH's nodes carries a bit under it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../ptsharp_amd/csrc/pt_scene_compile.h"
#include "../../ptsharp_amd/csrc/pt_stack_key.h"
#include "scene_fixture.h"

static long failures = 0;
#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) {                                                                   \
            if (++failures <= 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                                             \
    } while (0)

static void check(int ntri, int cap, bool dflt) {
    FixScene s;
    big_scene(s, ntri, 77u + (uint32_t)ntri);
    pt::CompileOptions opt;
    if (!dflt) opt.pop_cull_bits = cap;
    pt::HostScene H;
    std::string err;
    if (pt::compile_scene(&s.d, opt, H, err) != PT_OK) { std::printf("compile: %s\n", err.c_str()); CHECK(false); return; }
    const pt::DevScene& S = H.S;
    const uint64_t nodes = (uint64_t)S.tri_num_nodes, chunks = S.lines_n - S.tri_chunk_line0;
    CHECK(nodes > 0 && chunks > 0);
    const int K = pt::stack_key_choose(nodes, chunks, dflt ? pt::kStackKeyMaxBits : cap);
    const uint32_t km = S.stack_key_mask;
    CHECK(km == pt::stack_key_mask(K));
    CHECK(__builtin_popcount(km) == K);
    if (dflt) CHECK(K == (31 - pt::stack_idx_bits(nodes > chunks ? nodes : chunks) < 15 ? 31 - pt::stack_idx_bits(nodes > chunks ? nodes : chunks) : 15));
    if (!dflt && cap <= 0) CHECK(km == 0u);
    CHECK(!(km & 0x80000000u) && !(km & (uint32_t)(nodes - 1u)) && !(km & (uint32_t)(chunks - 1u)));
    // the refs a node step can push (pt_device.h node8_ref): base_in + k below n_in, leaf0 + k from n_in on
    const uint32_t* w = reinterpret_cast<const uint32_t*>(H.lines.data() + 8 * (size_t)S.tri_node_line0);
    for (uint64_t n = 0; n < nodes; n++) {
        const uint32_t hdr = w[32 * n + 3], nin = (hdr >> 24) & 15u, base_in = w[32 * n + 4], leaf0 = w[32 * n + 5];
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t ref = k < nin ? base_in + k : leaf0 + k;
            const bool leaf = k >= nin;
            if ((ref & 0x1FFFFFFFu) >= (leaf ? chunks : nodes)) continue;   // an empty slot's ref: never kept
            CHECK(!(ref & km));
            CHECK(pt::stack_entry_ref(pt::stack_entry(ref, 0x7FFFFFF8u | k, km), km) == ref);
        }
    }
    std::printf("%d triangles, cap %s%d: %llu nodes, %llu chunks, K %d ok\n", ntri, dflt ? "default " : "", dflt ? 15 : cap,
                (unsigned long long)nodes, (unsigned long long)chunks, K);
}

int main() {
    for (int ntri : {200, 4000, 70000}) {
        check(ntri, 0, true);
        for (int cap : {0, 1, 4, 15, 40, -2}) check(ntri, cap, false);
    }
    std::printf("stack_key_scene_check: %ld failures\n", failures);
    return failures ? 1 : 0;
}
