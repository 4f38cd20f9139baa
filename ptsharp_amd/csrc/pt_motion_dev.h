// pt_motion_dev.h — what pt_motion.hip's kernels take beside the DevScene and pt_query.h's tables: their own
// argument structs, so that DevScene, which goes by value into every render kernel, stays as it is.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "pt_motion.h"
#include "pt_query.h"
#include "pt_scene.h"

namespace pt {

// "The previous frame": pt_motion_snapshot's copies.  have == 0: no snapshot (every pointer may be NULL).
struct MotionSnap {
    const float4* tris;      // [num_src][3] world triangle records {v1, e1, e2}, by source triangle
    const float4* blas;      // [num_src][3] BLAS triangle records, by source triangle
    const float4* ana;       // [num_ana][3] analytic records, by record position
    const DevXform* xforms;  // [num_xforms]
    const float4* ext;       // [num_ext][3] the transformed shapes' inner records (kept with the rest; the inner shape is
                             // taken as rigid, so the motion pass does not read them)
    int64_t num_src, num_ana, num_xforms, num_ext;
    MotionCamera cam;
    int32_t have;
};

// pt_read_motion's arrays (motion_of)
struct MotionOut {
    double* prev_xy;
    double* depth;
    double* prev_depth;
    int32_t* shape;
    int32_t* prim;
    int32_t* prev_pixel;
    int32_t* status;
};

// One history set (temporal_set_of): the temporal result and the identity it was made with
struct TemporalSet {
    double* m;
    double* v;
    double* depth;
    int32_t* n;
    int32_t* shape;
    int32_t* prim;
};

size_t motion_bytes(int32_t W, int32_t H);
MotionOut motion_of(void* base, int32_t W, int32_t H);
size_t temporal_set_bytes(int32_t W, int32_t H);
TemporalSet temporal_set_of(void* base, int32_t W, int32_t H);

hipError_t launch_motion_snapshot_tris(int64_t num_pos, const float4* recs, int32_t stride, const int32_t* src_of_pos,
                                       int64_t num_src, float4* snap, hipStream_t stream);
hipError_t launch_motion(const DevScene& S, const QueryDevTables& T, const MotionSnap& N, const DevCamera& cam, const MotionOut& M,
                         int32_t W, int32_t H, hipStream_t stream);
hipError_t launch_temporal_merge(int32_t W, int32_t H, const double* m, const double* v, const int32_t* n, const MotionOut& M,
                                 const TemporalSet& hist, bool have_history, int32_t max_history, double sigma_depth,
                                 const TemporalSet& out, int32_t* status, hipStream_t stream);

}  // namespace pt
