// pt_query.h — what pt_intersect_hits' kernel (pt_query.hip) takes beside the DevScene: its own argument structs, so
// that DevScene and WfQueues, which go by value into every render kernel, stay as they are.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "pt_scene.h"

namespace pt {

constexpr int64_t kQueryChunkMax = (int64_t)1 << 22;   // rays staged and launched at a time (PT_QUERY_CHUNK lowers it)
constexpr int64_t kQueryChunkMin = 64;

// The identity tables on the device, each with its length: a lookup outside a table gives -1
struct QueryDevTables {
    const int32_t* tri_src;      // world BVH position -> source triangle (RefitTables::src_of_pos as it stands)
    const int32_t* blas_src;     // BLAS position -> source triangle (BlasRefitTables::src_of_pos)
    const int32_t* tri_slot;     // source triangle -> Scene.Shapes slot   (QueryTables, pt_scene_compile.h)
    const int32_t* ana_slot;     // analytic (kind, index) -> slot: entry ana_off[kind] + index
    const int32_t* plane_slot;   // plane -> slot
    int64_t tri_src_n, blas_src_n, tri_slot_n, ana_slot_n, plane_slot_n;
    int32_t ana_off[8], ana_cnt[8];
    int32_t num_blas;            // entries of DevScene::blas
};

// pt_hit_arrays' pointers as device addresses of the staged chunk; NULL: not wanted
struct QueryOut {
    double* t;
    int32_t* kind;
    int32_t* index;
    int32_t* prim;
    int32_t* shape;
    float* position;
    float* normal;
    int32_t* inside;
    int32_t* material;
    double* albedo;
    double* gloss;
};
inline bool query_wants_info(const QueryOut& o) {
    return o.position || o.normal || o.inside || o.material || o.albedo || o.gloss;
}

// n <= kQueryChunkMax rays on `stream`
hipError_t launch_intersect_hits(const DevScene& S, const QueryDevTables& T, int64_t n, const float* o3, const float* d3,
                                 const QueryOut& out, hipStream_t stream);

}  // namespace pt
