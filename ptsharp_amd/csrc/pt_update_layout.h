// pt_update_layout.h — how the moving-geometry entry points (pt_api.hip) carve their per-scene
// device workspaces: one allocation each, its parts 256-B aligned and in the order listed; and pt_rebuild_blas' host
// tables (its plans, level lists and tail workgroups).  Host code only: no HIP call, compiles with g++
// (tests/native/rebuild_check.cpp, blas_check.cpp, shapes_check.cpp, blas_rebuild_check.cpp and morph_check.cpp check
// the layouts and tables against what the kernels index).  With a null base the pointers are the parts' offsets.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "pt_blas_rebuild.h"
#include "pt_bvh.h"
#include "pt_rebuild.h"
#include "pt_scene_compile.h"

namespace pt {

// Parts taken one after another from `base`, each rounded up to 256 B
struct Carver {
    uintptr_t base;
    size_t at = 0;
    explicit Carver(void* b) : base((uintptr_t)b) {}
    template <class T>
    T* take(size_t n) {
        T* p = (T*)(base + at);
        at += (n * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
    size_t bytes() const { return at ? at : 256; }   // never an empty allocation
};

// pt_update_triangles: [v1 v2 v3 n1 n2 n3 staged | src_of_pos | level_nodes | an exact box per node | per chunk]
struct RefitDev {
    float* in[6];
    int32_t* src_of_pos;
    uint32_t* level_nodes;
    float* node_box;
    float* chunk_box;
    size_t bytes;
};
inline RefitDev refit_layout(const RefitTables& T, void* base) {
    Carver c(base);
    RefitDev r{};
    for (float*& a : r.in) a = c.take<float>((size_t)T.num_triangles * 3);
    r.src_of_pos = c.take<int32_t>(T.src_of_pos.size());
    // room for the tables pt_rebuild_meshes may put in their place: its balanced tree can have a few more nodes than
    // the uploaded one (never more chunks), and the layout is made once per scene, from the uploaded tables
    RebuildPlan R;
    const bool planned = rebuild_plan((int64_t)T.src_of_pos.size(), R);
    const size_t nodes = std::max({T.level_nodes.size(), (size_t)T.num_nodes, planned ? (size_t)R.num_nodes : (size_t)0});
    const size_t chunks = std::max((size_t)T.num_chunks, planned ? (size_t)R.num_chunks : (size_t)0);
    r.level_nodes = c.take<uint32_t>(nodes);
    r.node_box = c.take<float>(nodes * 6);
    r.chunk_box = c.take<float>(chunks * 6);
    r.bytes = c.bytes();
    return r;
}

// PT_NORMALS_SMOOTH: [group | keys a b | corners a b | the sort's temporary]
struct NormalsDev {
    int32_t* group;
    uint32_t* keys[2];
    uint32_t* vals[2];
    void* temp;
    size_t temp_bytes, bytes;
};
inline NormalsDev normals_layout(const RefitTables& T, size_t temp_bytes, void* base) {
    Carver c(base);
    NormalsDev r{};
    r.group = c.take<int32_t>((size_t)T.num_triangles);
    for (uint32_t*& a : r.keys) a = c.take<uint32_t>((size_t)T.num_triangles * 3);
    for (uint32_t*& a : r.vals) a = c.take<uint32_t>((size_t)T.num_triangles * 3);
    r.temp = c.take<char>(temp_bytes);
    r.temp_bytes = temp_bytes;
    r.bytes = c.bytes();
    return r;
}

// pt_update_shapes: [the staged parameters | xbox | rec_box | node_box | level_nodes | the transformed shapes' inner
// kind, index and box]
struct ShapesDev {
    float* sphere_center;
    double* sphere_radius;
    float* cube_min;
    float* cube_max;
    double* xf_matrix;
    double* xf_inverse;
    float* xbox;
    float* rec_box;
    float* node_box;
    uint32_t* level_nodes;
    int32_t* xf_kind;
    int32_t* xf_index;
    float* xf_inner_box;
    size_t bytes;
};
inline ShapesDev shapes_layout(const ShapeRefitTables& T, void* base) {
    Carver c(base);
    ShapesDev r{};
    const size_t ns = (size_t)T.num_spheres, nc = (size_t)T.num_cubes, nx = (size_t)T.num_transformed;
    r.sphere_center = c.take<float>(ns * 3);
    r.sphere_radius = c.take<double>(ns);
    r.cube_min = c.take<float>(nc * 3);
    r.cube_max = c.take<float>(nc * 3);
    r.xf_matrix = c.take<double>(nx * 16);
    r.xf_inverse = c.take<double>(nx * 16);
    r.xbox = c.take<float>(nx * 6);
    r.rec_box = c.take<float>((size_t)T.num_recs * 6);
    r.node_box = c.take<float>((size_t)T.num_nodes * 6);
    r.level_nodes = c.take<uint32_t>(T.level_nodes.size());
    r.xf_kind = c.take<int32_t>(nx);
    r.xf_index = c.take<int32_t>(nx);
    r.xf_inner_box = c.take<float>(nx * 6);
    r.bytes = c.bytes();
    return r;
}

// k_blas_bounds' blocks: each folds up to `span` positions (pt::blas_bounds_span()) of one BLAS
struct BlasBlocks {
    std::vector<int32_t> blas, first, off;   // per block its BLAS and first position; per BLAS its first block (and the end)
};
inline void blas_blocks(const BlasRefitTables& T, int64_t span, BlasBlocks& B) {
    for (size_t b = 0; b < T.num_blas(); b++) {
        B.off.push_back((int32_t)B.blas.size());
        const int64_t r0 = T.desc[4 * b + 2], n = T.desc[4 * b + 3];
        for (int64_t at = 0; at < n; at += span) {
            B.blas.push_back((int32_t)b);
            B.first.push_back((int32_t)(r0 + at));
        }
    }
    B.off.push_back((int32_t)B.blas.size());
}
// pt_update_meshes on instanced meshes: [the tables | tri_box | node_box | block_part | blas_box]
struct BlasDev {
    int32_t* desc;
    int32_t* src_of_pos;
    uint32_t* level_nodes;
    int32_t* level_blas;
    int32_t* block_blas;
    int32_t* block_first;
    int32_t* blas_block_off;
    int32_t* xf_blas;
    float* tri_box;
    float* node_box;
    float* block_part;
    float* blas_box;
    size_t num_blocks, bytes;
};
inline BlasDev blas_layout(const BlasRefitTables& T, size_t num_blocks, void* base) {
    Carver c(base);
    BlasDev r{};
    const size_t nb = T.num_blas();
    r.desc = c.take<int32_t>(T.desc.size());
    r.src_of_pos = c.take<int32_t>(T.src_of_pos.size());
    r.level_nodes = c.take<uint32_t>(T.level_nodes.size());
    r.level_blas = c.take<int32_t>(T.level_blas.size());
    r.block_blas = c.take<int32_t>(num_blocks);
    r.block_first = c.take<int32_t>(num_blocks);
    r.blas_block_off = c.take<int32_t>(nb + 1);
    r.xf_blas = c.take<int32_t>(T.xf_blas.size());
    r.tri_box = c.take<float>((size_t)T.num_tris * 6);
    r.node_box = c.take<float>((size_t)T.num_nodes * 6);
    r.block_part = c.take<float>(num_blocks * 6);
    r.blas_box = c.take<float>(nb * 6);
    r.num_blocks = num_blocks;
    r.bytes = c.bytes();
    return r;
}

// pt_rebuild_blas' plan for the BLASes of T: four int32 per BLAS (pt_blas_rebuild.hip BlasRbItem: rec_off, n, h,
// node_off), h == 0 for a BLAS that keeps its topology: an empty one, or one whose balanced tree needs more nodes than
// node_cap[b], the count the upload gave it.  false: BLAS *refused needs more than kBlasRebuildMaxLevels levels.
inline bool blas_rebuild_items(const BlasRefitTables& T, const std::vector<int32_t>& node_cap, std::vector<int32_t>& items,
                               size_t* refused) {
    const size_t nb = T.num_blas();
    items.assign(4 * nb, 0);
    for (size_t b = 0; b < nb; b++) {
        const int32_t n = T.desc[4 * b + 3];
        BlasPlan R;
        if (!blas_rebuild_plan(n, R) || blas_rebuild_stack_bound(R) > kStack4Budget) { *refused = b; return false; }
        const bool fits = n > 0 && b < node_cap.size() && R.num_nodes <= (int64_t)node_cap[b];
        items[4 * b] = T.desc[4 * b + 2];
        items[4 * b + 1] = n;
        items[4 * b + 2] = fits ? R.h : 0;
        items[4 * b + 3] = T.desc[4 * b];
    }
    return true;
}
// What follows in T from the new topologies: a rebuilt BLAS's node count (desc) and its levels from its plan, a kept
// one's as they were.  The lists never grow: a rebuilt BLAS has no more nodes than the upload gave it.
inline void blas_rebuild_tables(BlasRefitTables& T, const std::vector<int32_t>& items) {
    const size_t nb = T.num_blas();
    std::vector<std::vector<std::vector<uint32_t>>> kept(nb);   // [BLAS][level] -> its nodes
    for (size_t l = 0; l + 1 < T.level_off.size(); l++)
        for (uint32_t q = T.level_off[l]; q < T.level_off[l + 1]; q++) {
            const size_t b = (size_t)T.level_blas[q];
            if (b >= nb || items[4 * b + 2] > 0) continue;
            if (kept[b].size() <= l) kept[b].resize(l + 1);
            kept[b][l].push_back(T.level_nodes[q]);
        }
    size_t depth = 0;
    std::vector<BlasPlan> plans(nb);
    for (size_t b = 0; b < nb; b++) {
        const int32_t h = items[4 * b + 2];
        if (h > 0) {
            blas_rebuild_plan(T.desc[4 * b + 3], plans[b]);
            T.desc[4 * b + 1] = (int32_t)plans[b].num_nodes;
        }
        depth = std::max(depth, h > 0 ? (size_t)h : kept[b].size());
    }
    T.level_nodes.clear();
    T.level_blas.clear();
    T.level_off.assign(1, 0u);
    for (size_t l = 0; l < depth; l++) {
        for (size_t b = 0; b < nb; b++) {
            const int32_t h = items[4 * b + 2];
            if (h > 0) {
                if ((int32_t)l >= h) continue;
                const int64_t off = blas_rebuild_level_off(plans[b].num_leaves, h, (int)l);
                const int64_t cnt = blas_rebuild_level_count(plans[b].num_leaves, h, (int)l);
                for (int64_t i = 0; i < cnt; i++) { T.level_nodes.push_back((uint32_t)(off + i)); T.level_blas.push_back((int32_t)b); }
            } else if (l < kept[b].size()) {
                for (const uint32_t n : kept[b][l]) { T.level_nodes.push_back(n); T.level_blas.push_back((int32_t)b); }
            }
        }
        T.level_off.push_back((uint32_t)T.level_nodes.size());
    }
}

// The tail's workgroups for the BLASes in `items` (four int32 each: BlasRbItem) and a tail of T positions (0: no tail,
// else 4 * 4^k, at most pt_blas_rebuild.hip's kBlasTailMax): four int32 per workgroup.  A BLAS whose first segment fits T is one workgroup from
// its first shift; a larger one is cut into segments of T positions that start at T's shift.  Depends on n alone.
inline void blas_tail_table(const int32_t* items, int64_t num_blas, int64_t T, std::vector<int32_t>& tail) {
    tail.clear();
    if (T <= 0) return;
    int sT = 0;
    while (((int64_t)4 << sT) < T) sT++;
    for (int64_t b = 0; b < num_blas; b++) {
        const int64_t r0 = items[4 * b], n = items[4 * b + 1], h = items[4 * b + 2];
        if (h <= 0 || n <= 0) continue;
        const int s0 = 2 * (int)h < sT ? 2 * (int)h : sT;
        const int64_t seg = (int64_t)4 << s0;
        for (int64_t at = 0; at < n; at += seg) {
            const int32_t row[4] = {(int32_t)(r0 + at), (int32_t)(at + seg < n ? seg : n - at), s0, 0};
            tail.insert(tail.end(), row, row + 4);
        }
    }
}

// pt_pose_meshes: [rest v1 v2 v3 n1 n2 n3 | group | matrices | mask]
struct PoseDev {
    float* rest[6];
    int32_t* group;
    double* matrices;
    int32_t* mask;
    size_t bytes;
};
inline PoseDev pose_layout(const RefitTables& T, void* base) {
    Carver c(base);
    PoseDev r{};
    for (float*& a : r.rest) a = c.take<float>((size_t)T.num_triangles * 3);
    r.group = c.take<int32_t>((size_t)T.num_triangles);
    r.matrices = c.take<double>((size_t)T.num_groups * 16);
    r.mask = c.take<int32_t>((size_t)T.num_groups);
    r.bytes = c.bytes();
    return r;
}

// pt_set_skin: [bone1 bone2 bone3 | weight1 weight2 weight3 | matrices]: per corner four 16-bit bone indices and four
// fp32 weights per triangle (3 * (8 + 16) = 72 B per triangle), then room for bone_cap matrices of 16 doubles
struct SkinDev {
    uint16_t* bone[3];
    float* weight[3];
    double* matrices;
    int32_t bone_cap;
    size_t bytes;
};
inline SkinDev skin_layout(int32_t num_triangles, int32_t bone_cap, void* base) {
    Carver c(base);
    SkinDev r{};
    for (uint16_t*& a : r.bone) a = c.take<uint16_t>((size_t)num_triangles * 4);
    for (float*& a : r.weight) a = c.take<float>((size_t)num_triangles * 4);
    r.matrices = c.take<double>((size_t)bone_cap * 16);
    r.bone_cap = bone_cap;
    r.bytes = c.bytes();
    return r;
}

// pt_set_morph: [len | first | target | dpos | dnrm | weights]: pt_morph.h's packed planes (per step of a slice 128 B
// of 16-bit targets and 768 B of position deltas, 768 B more with normal deltas; 12 B per slice), then room for one
// fp32 weight per target.  Every part starts on a 256-B boundary and a step is a whole number of 128-B lines, so every
// step of every plane starts on a line.
struct MorphDev {
    int32_t* len;
    int64_t* first;
    uint16_t* target;
    float* dpos;
    float* dnrm;      // NULL: the morph carries no normal deltas
    float* weights;
    size_t bytes;
};
inline MorphDev morph_layout(int64_t slices, int64_t steps, bool has_dnrm, int32_t num_targets, void* base) {
    Carver c(base);
    MorphDev r{};
    r.len = c.take<int32_t>((size_t)slices);
    r.first = c.take<int64_t>((size_t)slices);
    r.target = c.take<uint16_t>((size_t)steps * 64);
    r.dpos = c.take<float>((size_t)steps * 64 * 3);
    float* const dnrm = c.take<float>(has_dnrm ? (size_t)steps * 64 * 3 : 0);
    r.dnrm = has_dnrm ? dnrm : nullptr;
    r.weights = c.take<float>((size_t)num_targets);
    r.bytes = c.bytes();
    return r;
}
// pt_morph_meshes with skin_matrices: the morphed v1 v2 v3 n1 n2 n3 between the two kernels (72 B per triangle), made
// by the first such call
struct MorphTmpDev {
    float* out[6];
    size_t bytes;
};
inline MorphTmpDev morph_tmp_layout(int64_t num_triangles, void* base) {
    Carver c(base);
    MorphTmpDev r{};
    for (float*& a : r.out) a = c.take<float>((size_t)num_triangles * 3);
    r.bytes = c.bytes();
    return r;
}

// pt_intersect_hits' identity tables (pt_query.h): [tri_src | blas_src | tri_slot | ana_slot | plane_slot]
struct QueryDev {
    int32_t* tri_src;
    int32_t* blas_src;
    int32_t* tri_slot;
    int32_t* ana_slot;
    int32_t* plane_slot;
    size_t bytes;
};
inline QueryDev query_layout(const RefitTables& T, const BlasRefitTables& B, const QueryTables& Q, void* base) {
    Carver c(base);
    QueryDev r{};
    r.tri_src = c.take<int32_t>(T.src_of_pos.size());
    r.blas_src = c.take<int32_t>(B.src_of_pos.size());
    r.tri_slot = c.take<int32_t>(Q.tri_slot.size());
    r.ana_slot = c.take<int32_t>(Q.ana_slot.size());
    r.plane_slot = c.take<int32_t>(Q.plane_slot.size());
    r.bytes = c.bytes();
    return r;
}

}  // namespace pt
