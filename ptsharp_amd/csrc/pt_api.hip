// pt_api.hip — C-ABI implementation of libptsharp_hip.so (include/ptsharp_hip.h).
//
// Host runtime around the gfx950 render kernels: upload of the compiled scene
// (pt_scene_compile.cpp flattens it and builds the BVHs on the host), HBM-resident
// Welford buffer (Renderer.PBuffer, Renderer.cs:20), pass launch and timing
// (RenderParallel + its stopwatch, Renderer.cs:199-213,470), ray statistics
// (Scene.rays, Scene.cs:70-79), and the multi-GPU Buffer gather over RCCL.
// No exception crosses the ABI: every entry point returns a pt_status and
// leaves a thread-local message for pt_last_error (the OIDN convention,
// OIDN.cs:85-86).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/ptsharp_hip.h"
#include "pt_blas_refit.h"
#include "pt_blas_rebuild.h"
#include "pt_bvh.h"
#include "pt_device.h"
#include "pt_math.h"
#include "pt_pass_plan.h"
#include "pt_query.h"
#include "pt_rebuild.h"
#include "pt_scene.h"
#include "pt_scene_compile.h"
#include "pt_shape_refit.h"
#include "pt_morph.h"
#include "pt_motion_dev.h"
#include "pt_skin.h"
#include "pt_texture.h"
#include "pt_update_layout.h"
#include "pt_volume_update.h"
#include "pt_wavefront.h"

#pragma clang fp contract(off)

namespace pt {
// After a gather the root's Buffer holds every rank's tiles; before its next pass adds to
// its own tiles (and before a firefly snapshot is all-reduced) the other ranks' pixels are
// cleared again, so every context's Buffer holds exactly its own tiles between gathers.
__global__ __launch_bounds__(256) void k_clear_foreign(DevBuffer B, int32_t width, int32_t height, int32_t tiles_x,
                                                       const uint8_t* own) {
    const size_t P = (size_t)width * (size_t)height;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % (size_t)width), y = (int)(i / (size_t)width);
        if (own[(y >> 5) * tiles_x + (x >> 5)]) continue;
        B.n[i] = 0;
        for (int k = 0; k < 3; k++) { B.m[3 * i + k] = 0.0; B.v[3 * i + k] = 0.0; }
    }
}
// Packed tiles (pt_read_tiles / pt_write_tiles, the tile-compacted gather): entry s of a run
// is pixel (s & 31, (s >> 5) & 31) of tile ids[s >> 10], row-major inside the tile; pack
// copies {M, V, N} out (zeros outside the image), unpack writes a run into the Buffer.
__global__ __launch_bounds__(256) void k_tiles_pack(DevBuffer B, int32_t width, int32_t height, int32_t tiles_x,
                                                    const int32_t* ids, uint32_t nt, double* pm, double* pv,
                                                    int32_t* pn, int unpack) {
    const size_t total = (size_t)nt * 1024u;
    for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < total; s += (size_t)gridDim.x * blockDim.x) {
        const int tile = ids[s >> 10];
        const int x = (tile % tiles_x) * 32 + (int)(s & 31u), y = (tile / tiles_x) * 32 + (int)((s >> 5) & 31u);
        const bool in = x < width && y < height;
        const size_t i = (size_t)y * (size_t)width + (size_t)x;
        if (unpack) {
            if (!in) continue;
            B.n[i] = pn[s];
            for (int k = 0; k < 3; k++) { B.m[3 * i + k] = pm[3 * s + k]; B.v[3 * i + k] = pv[3 * s + k]; }
        } else {
            pn[s] = in ? B.n[i] : 0;
            for (int k = 0; k < 3; k++) { pm[3 * s + k] = in ? B.m[3 * i + k] : 0.0; pv[3 * s + k] = in ? B.v[3 * i + k] : 0.0; }
        }
    }
}
__global__ void k_iota(int32_t* a, int32_t n) {
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) a[i] = i;
}
hipError_t launch_render_pass(const DevScene& S, const DevCamera& cam, const DevSampler& smp, const DevPass& P,
                              const DevBuffer& B, int num_tiles, bool count, hipStream_t stream);
hipError_t launch_intersect(const DevScene& S, uint32_t n, const float* o3, const float* d3, const double* tl,
                            double* out_t, int32_t* out_kind, hipStream_t stream);
// pt_image.hip
size_t image_staging_bytes(int32_t W, int32_t H);
hipError_t launch_image_resolve(int channel, int format, const double* m, const double* v, const int32_t* n,
                                int32_t* max_n, uint32_t* out, int32_t W, int32_t H, hipStream_t stream);
// pt_denoise.hip
size_t denoise_workspace_bytes(int32_t W, int32_t H);
hipError_t launch_denoise(const double* m, const double* v, const int32_t* n, void* ws, int32_t W, int32_t H,
                          int32_t iterations, double sigma, int* out_pair, hipStream_t stream);
hipError_t launch_denoise_guided(const double* m, const double* v, const int32_t* n, void* ws, const void* guide,
                                 int32_t W, int32_t H, int32_t iterations, double sigma, double sigma_albedo,
                                 double sigma_normal, double sigma_depth, int* out_pair, hipStream_t stream);
// pt_features.hip
size_t features_bytes(int32_t W, int32_t H);
void* features_part(void* base, int32_t W, int32_t H, int part, size_t* bytes);
const void* features_guide(void* base, int32_t W, int32_t H);
hipError_t launch_features(const DevScene& S, const DevCamera& cam, void* base, int32_t W, int32_t H, hipStream_t stream);
hipError_t launch_features_pack(void* base, int32_t W, int32_t H, hipStream_t stream);
// pt_refit.hip
hipError_t launch_refit(int64_t num_chunks, int64_t num_levels, const uint32_t* level_off, const uint32_t* level_nodes,
                        uint32_t* nodes, uint32_t* chunks, uint32_t* recs, const int32_t* src_of_pos, const float* v1,
                        const float* v2, const float* v3, const float* n1, const float* n2, const float* n3,
                        float* node_box, float* chunk_box, hipStream_t stream);
// pt_shape_refit.hip
hipError_t launch_shape_refit(const ShapeParams& P, int64_t num_nodes, int64_t num_recs, int64_t num_heavy, int64_t num_levels,
                              const uint32_t* level_off, const uint32_t* level_nodes, uint32_t* nodes, uint32_t* recs,
                              uint32_t* ext_recs, DevXform* xforms, uint32_t* heavy, const int32_t* inner_kind,
                              const int32_t* inner_index, const float* inner_box, float* xbox, float* rec_box, float* node_box,
                              hipStream_t stream);
// pt_blas_refit.hip
int64_t blas_bounds_span();
hipError_t launch_blas_refit(int64_t num_blas, int64_t num_pos, int64_t num_nodes, int64_t num_triangles, int64_t num_transformed,
                             int64_t num_blocks, int64_t num_levels, const uint32_t* level_off, const uint32_t* level_nodes,
                             const int32_t* level_blas, const int32_t* desc, const int32_t* src_of_pos, const int32_t* block_blas,
                             const int32_t* block_first, const int32_t* blas_block_off, const int32_t* xf_blas, uint32_t* nodes,
                             uint32_t* recs, uint32_t* shade, const float* v1, const float* v2, const float* v3, const float* n1,
                             const float* n2, const float* n3, float* tri_box, float* node_box, float* block_part, float* blas_box,
                             float* xf_inner_box, hipStream_t stream);
// pt_normals.hip
hipError_t normals_sort_temp_bytes(int64_t corners, int32_t num_groups, size_t* out);
hipError_t launch_normals(bool smooth, int64_t n, const float* v1, const float* v2, const float* v3, float* n1, float* n2,
                          float* n3, const int32_t* group, int32_t num_groups, uint32_t* keys_a, uint32_t* keys_b,
                          uint32_t* vals_a, uint32_t* vals_b, void* temp, size_t temp_bytes, hipStream_t stream);
hipError_t launch_normals_gather(int64_t num_pos, const uint32_t* recs, const int32_t* src_of_pos, float* n1, float* n2,
                                 float* n3, hipStream_t stream);
// pt_rebuild.hip
hipError_t rebuild_workspace_bytes(int64_t P, size_t* temp_bytes, size_t* bytes);
hipError_t launch_rebuild(const RebuildPlan& R, void* ws, size_t temp_bytes, uint32_t* nodes, uint32_t* chunks, uint32_t* recs,
                          int32_t* src_of_pos, uint32_t* level_nodes, const float* v1, const float* v2, const float* v3,
                          hipStream_t stream);
hipError_t bvh_cost_workspace_bytes(int64_t num_nodes, size_t* bytes);
hipError_t launch_bvh_cost(int64_t num_nodes, const uint32_t* nodes, void* ws, double* sums, hipStream_t stream);
// pt_blas_rebuild.hip
int64_t blas_tail_max();
hipError_t blas_rebuild_workspace_bytes(int64_t num_blas, int64_t P, size_t* temp_bytes, size_t* bytes);
hipError_t blas_rebuild_upload(void* ws, size_t temp_bytes, int64_t num_blas, int64_t P, const int32_t* pos_blas, hipStream_t stream);
hipError_t launch_blas_rebuild(void* ws, size_t temp_bytes, int64_t num_blas, int64_t P, int64_t total_nodes, const int32_t* items,
                               const int32_t* tail, int64_t num_tail, int64_t tail_T, uint32_t* nodes, uint32_t* shade, uint32_t* uv,
                               int32_t* src_of_pos, const float* v1, const float* v2, const float* v3, hipStream_t stream);
size_t blas_cost_workspace_bytes(int64_t total_nodes);
hipError_t launch_blas_cost(int64_t num_blas, int64_t total_nodes, int64_t max_nodes, const int32_t* desc, const uint32_t* nodes,
                            void* ws, double* out, hipStream_t stream);
// pt_pose.hip
hipError_t launch_pose(int64_t n, int32_t num_meshes, const int32_t* group, const int32_t* mask, const double* matrices,
                       bool normals, const float* const rest[6], float* const out[6], hipStream_t stream);
// pt_skin.hip
hipError_t launch_skin(int64_t n, int32_t num_bones, const int32_t* group, const double* matrices, bool normals,
                       const uint16_t* const bone[3], const float* const weight[3], const float* const rest[6], float* const out[6],
                       hipStream_t stream);
// pt_morph.hip
hipError_t launch_morph(int64_t n, int32_t num_targets, const int32_t* group, const float* weights, int normals, const int32_t* len,
                        const int64_t* first, const uint16_t* target, const float* dpos, const float* dnrm, const float* const rest[6],
                        float* const out[6], hipStream_t stream);
// pt_volume.hip
hipError_t launch_vol_rebuild(const DevVolume& v, bool new_data, hipStream_t stream);
// pt_texture.hip
hipError_t launch_tex_decode(const uint8_t* src, uint64_t src_off, int format, uint64_t pixels, const double* lut, double* dst,
                             hipStream_t stream);
}

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define PT_HIP(call)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail(PT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));               \
    } while (0)

struct DeviceArray {
    void* ptr = nullptr;
    size_t bytes = 0;
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
};

// hipEvent pairs around each launch of a pass (PT_PASS_KERNEL_TIMING): device
// time per kernel class, read after the pass' final synchronisation.
struct EventTimer : pt::LaunchTimer {
    std::vector<hipEvent_t> pool;
    std::vector<int> cls;
    size_t used = 0;
    hipStream_t stream = nullptr;
    bool failed = false;
    void reset(hipStream_t s) { stream = s; used = 0; cls.clear(); failed = false; }
    void record(int c, bool is_begin, hipStream_t s) {
        if (used == pool.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) { failed = true; return; }
            pool.push_back(e);
        }
        if (hipEventRecord(pool[used], s ? s : stream) != hipSuccess) failed = true;
        if (is_begin) cls.push_back(c);
        used++;
    }
    void begin(int c, hipStream_t s) override { record(c, true, s); }
    void end(int c, hipStream_t s) override { record(c, false, s); }
    hipError_t collect(double* ms, uint32_t* launches) {
        for (size_t i = 0; i + 1 < used; i += 2) {
            float t = 0.f;
            hipError_t e = hipEventElapsedTime(&t, pool[i], pool[i + 1]);
            if (e != hipSuccess) return e;
            ms[cls[i / 2]] += t;
            launches[cls[i / 2]]++;
        }
        return hipSuccess;
    }
    void destroy() { for (auto e : pool) (void)hipEventDestroy(e); pool.clear(); }
};

// A per-scene device workspace of the moving-geometry entry points: one allocation that comes with the first call
// that needs it (ensure_workspace), its carved parts (pt_update_layout.h) kept beside it, and goes with the scene
template <class L>
struct Workspace {
    DeviceArray mem;
    L at{};
    void release() { mem.release(); at = L{}; }
};
// pt_rebuild_meshes' workspace (the sort's keys, values and temporary, the segments' bounds and the records' scratch
// copy) is carved by pt_rebuild.hip: what its launch takes
struct RebuildDev {
    size_t temp_bytes, bytes;
};
// Everything the moving-geometry entry points keep per scene.  free_scene replaces it by a fresh value, so a field
// added here is reset with the rest; a device allocation added here goes into release_device.
struct SceneDyn {
    // the host tables of the last upload (pt_scene_compile.h); shape_refit with the parameters the device holds now
    pt::RefitTables refit;
    pt::ShapeRefitTables shape_refit;
    pt::BlasRefitTables blas_refit;
    pt::QueryTables query;                // the slot tables pt_intersect_hits uploads at its first call
    std::vector<pt::DevLight> h_lights;   // the uploaded lights; the ones that follow geometry are moved by the updates
    bool has_blas = false;                // an instanced mesh: pt_update_triangles and pt_rebuild_meshes refuse
    // pt_update_volumes: the volumes' headers with their device addresses and zero_sign as the device
    // holds them, the window rows it holds now (volume i's start at vol_win_off[i]), the light test's inputs; no grid
    pt::VolumeTables volume_update;
    std::vector<pt::DevVolume> vols;
    std::vector<pt::DevWindow> vol_windows;
    std::vector<size_t> vol_win_off;
    Workspace<pt::RefitDev> refit_ws;       // first update, or pt_read_tri_normals
    Workspace<pt::NormalsDev> normals_ws;   // first PT_NORMALS_SMOOTH
    Workspace<pt::ShapesDev> shapes_ws;     // first pt_update_shapes, or pt_update_meshes on instanced meshes
    Workspace<pt::BlasDev> blas_ws;         // first pt_update_meshes on instanced meshes
    Workspace<pt::PoseDev> pose_ws;         // pt_set_rest_pose
    Workspace<pt::SkinDev> skin_ws;         // pt_set_skin
    int32_t skin_bones = 0;                 // the installed skin's num_bones (0: none)
    Workspace<pt::MorphDev> morph_ws;       // pt_set_morph: the packed planes (pt_morph.h)
    Workspace<pt::MorphTmpDev> morph_tmp_ws;   // first pt_morph_meshes with skin_matrices: the morphed arrays the skin reads
    int32_t morph_targets = 0;              // the installed morph's num_targets (0: none), its deltas, slices and steps
    int64_t morph_deltas = 0, morph_slices = 0, morph_steps = 0;
    Workspace<RebuildDev> rebuild_ws;       // first pt_rebuild_meshes
    Workspace<pt::QueryDev> query_ws;       // first pt_intersect_hits: its own copies of the identity tables
    bool query_src_stale = false;           // a pt_rebuild_meshes permuted refit.src_of_pos after query_ws took its copy
    // pt_rebuild_blas: its workspace (carved by pt_blas_rebuild.hip), the upload's DevBlas rows with the
    // node counts the device holds now, the node count the upload gave each BLAS, and the host tables its copies are
    // issued from (they live until the call's synchronisation)
    Workspace<RebuildDev> blas_rebuild_ws;   // first pt_rebuild_blas on instanced meshes
    std::vector<pt::DevBlas> h_blas;
    std::vector<int32_t> blas_node_cap;
    std::vector<int32_t> blas_items, blas_tail, blas_pos;
    bool query_blas_src_stale = false;       // a pt_rebuild_blas permuted blas_refit.src_of_pos after query_ws took its copy
    // pt_set_rest_pose: the rest vertices of every loose triangle of Scene.Shapes, laid out as look.tri_verts (a light
    // that is one returns to them at every pose)
    std::vector<float> rest_tri_verts;
    // pt_update_materials and pt_update_textures: the slots the light test runs over, with the loose
    // triangles' vertices as the device holds them now; the material table the device holds (the scene's rows, then
    // `new Material()`); the entries S.lights has room for; the textures with their device addresses; the byte
    // staging of the 8-bit formats (every texture's table, then 4 B per texel of the scene)
    pt::LookTables look;
    std::vector<pt::DevMaterial> h_mats;
    size_t lights_cap = 0;
    std::vector<pt::DevTexture> texs;
    DeviceArray tex_stage;
    // motion vectors and temporal accumulation: pt_motion_snapshot's copies (pt_motion_dev.h MotionSnap,
    // carved by motion_snap_layout) and its camera; the last pt_render_motion's arrays; the two history sets and the
    // merge's status.  All of it goes with the scene.
    int64_t num_xforms = 0, num_ext_recs = 0;   // entries of DevScene::xforms, records of DevScene::ext_recs
    DeviceArray motion_snap, motion_out, temporal;
    pt::MotionSnap snap{};
    bool have_motion = false;            // motion_out holds a pt_render_motion's result
    bool motion_fresh = false;           // ... rendered since the last pt_accumulate_temporal or pt_reset_temporal
    bool have_history = false;           // temporal's set temporal_cur holds a history
    bool have_temporal = false;          // ... which is the last pt_accumulate_temporal's result
    int temporal_cur = 0;
    bool pose_staged = false;            // refit_ws' staged arrays hold the last pose, skin or morph (pt_read_pose)
    bool blas_boxes_on_device = false;   // blas_ws holds the meshes' boxes (after the first pt_update_meshes)
    void release_device() {
        refit_ws.release();
        normals_ws.release();
        shapes_ws.release();
        blas_ws.release();
        pose_ws.release();
        skin_ws.release();
        morph_ws.release();
        morph_tmp_ws.release();
        rebuild_ws.release();
        blas_rebuild_ws.release();
        query_ws.release();
        tex_stage.release();
        motion_snap.release();
        motion_out.release();
        temporal.release();
    }
};

struct Ctx {
    int device = 0;
    int width = 0, height = 0;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;                          // shadow passes (pt::WfPlan::side)
    hipEvent_t ev_main = nullptr, ev_side[2] = {nullptr, nullptr};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // Welford buffer
    double* d_m = nullptr;
    double* d_v = nullptr;
    int32_t* d_n = nullptr;
    unsigned long long* d_counters = nullptr;   // [pt::kCounterAllocWords] the pass' counters (pt::DevBuffer::counters)
    unsigned long long* h_counters = nullptr;   // [pt::kCounterAllocWords] pinned: their read-back
    uint8_t* d_image = nullptr;                 // pt_read_image's staging image, then its max-N word (first use)
    void* d_denoise = nullptr;                  // pt_denoise's workspace: two {c, s2} pairs and the validity bytes (first use)
    int denoise_pair = -1;                      // the pair that holds the last pt_denoise's or pt_denoise_guided's result (-1: none yet)
    void* d_features = nullptr;                 // first-hit features and their guide records (pt_features.hip; first use)
    bool have_features = false;                 // pt_render_features or pt_write_features filled d_features
    double query_kernel_ms = 0;                 // the last pt_intersect_hits' kernels (pt_query_kernel_ms)
    int32_t* d_tiles = nullptr;
    int32_t tiles_cap = 0;
    std::vector<int32_t> h_tiles;               // the tile list in d_tiles (uploaded when it changes)
    // scene
    bool has_scene = false;
    std::vector<DeviceArray> scene_arrays;
    pt::DevScene S{};
    // stats
    pt_stats stats{};
    // RCCL
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    bool gathered = false;          // other ranks' tiles are in the Buffer (a gather, pt_write_tiles) until the next pass
    bool loaded = false;            // pt_write_buffer put a whole checkpoint in (foreign pixels once the context has a communicator)
    uint8_t* d_own = nullptr;       // [tiles] 1 = a tile of this context's last tile list
    int32_t pass_tiles = 0;         // tiles of the last pass (0: the whole image); their ids are in d_tiles
    // tile-compacted gather workspace (allocated by the first gather): ids, M, V, N of up to
    // every tile of the image, the rank counts, and the ids 0..tiles-1 of a whole-image rank
    int32_t* g_ids = nullptr;
    double* g_m = nullptr;
    double* g_v = nullptr;
    int32_t* g_n = nullptr;
    int32_t* g_cnts = nullptr;      // [nranks + 1]: all ranks' tile counts, then this rank's
    int32_t* g_all = nullptr;
    // wavefront queues (allocated on first use, grown on demand)
    pt::WfQueues Q{};
    std::vector<DeviceArray> wf_arrays;
    uint32_t wf_cap = 0, wf_scap = 0;
    bool wf_two_sets = false;      // a second shadow-ray set allocated (the side stream's shadow passes need it)
    int32_t acc_passes = 0;        // passes of per-pixel accumulators allocated (a batch needs one set per pass)
    uint32_t wf_max_cap = 0;       // queue capacity bound (wf_max_cap()), once per context
    // adaptive / firefly phases (allocated on first use, with the queues)
    uint32_t* d_plist = nullptr;   // [P] firefly candidates (ping-pong with d_plist2 over the rounds)
    uint32_t* d_plist2 = nullptr;
    uint32_t* d_fcount = nullptr;  // [2] list lengths
    double* d_snap = nullptr;      // [P][3] M at the start of the firefly phase
    pt::FixAcc acc_s{};            // [acc_s_cap] per-sample accumulators (own allocation; Q.acc_s points at it)
    uint64_t acc_s_cap = 0;
    int last_engine = 0;
    pt::WfGrids grids{};           // persistent grid sizes (pt::wavefront_grids), once per context
    EventTimer timer;
    double tri_build_ms = 0;       // last upload: host time to build (or wait for, or find) the triangle BVH
    std::shared_ptr<const pt::TriBvhBuild> tri_build;   // that build, shared with the other contexts of its geometry
                                                    // (released at the next upload and at pt_destroy)
    SceneDyn dyn;                  // moving geometry: born after an upload, gone with the scene (free_scene)
};

// The device time between Ctx::ev0 and Ctx::ev1, after the stream that recorded them was synchronised
int kernel_ms(Ctx* c, double* out_kernel_ms) {
    if (!out_kernel_ms) return PT_OK;
    float ms = 0.f;
    PT_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *out_kernel_ms = ms;
    return PT_OK;
}

int check_hip(hipError_t e, const char* what) {
    return e == hipSuccess ? PT_OK : fail(PT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
// Host arrays to the device on one stream; after an error the rest are skipped
struct Uploader {
    hipStream_t stream;
    hipError_t err = hipSuccess;
    void copy(void* dst, const void* src, size_t bytes) {
        if (err == hipSuccess && bytes) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
    }
    template <class T>
    void operator()(T* dst, const std::vector<T>& v) { copy(dst, v.data(), v.size() * sizeof(T)); }
};

// A workspace allocated once per scene, else reused; *first tells which.  layout(base) carves it (called with NULL
// for the size, then with the allocation); upload(parts, Uploader&) copies what the first use puts there, on the
// context's stream.  "Allocated" means "tables uploaded": when an upload fails the workspace is released, so the
// next call starts over.
template <class L, class Layout, class Upload>
int ensure_workspace(Ctx* c, Workspace<L>& W, const char* name, Layout&& layout, Upload&& upload, bool* first = nullptr) {
    if (first) *first = !W.mem.ptr;
    if (W.mem.ptr) return PT_OK;
    const size_t bytes = layout(nullptr).bytes;
    if (hipMalloc(&W.mem.ptr, bytes) != hipSuccess) {
        W.mem.ptr = nullptr;
        (void)hipGetLastError();
        return fail(PT_ERR_OUT_OF_MEMORY, std::string(name) + " workspace allocation");
    }
    W.mem.bytes = bytes;
    W.at = layout(W.mem.ptr);
    Uploader up{c->stream};
    upload(W.at, up);
    const int rc = check_hip(up.err, (std::string(name) + " workspace tables").c_str());
    if (rc != PT_OK) W.release();
    return rc;
}

#ifndef PT_VOL_DEFER
#define PT_VOL_DEFER 1   // split traversal: Volumes deferred to k_wf_vol_hits / k_wf_vol_shadow (0: marched in place)
#endif

// The context's queue capacity bound (pt_pass_plan.h: the budget and what it counts), found at its first pass:
// from PT_WF_MAX_CAP if the environment sets it, else from the device's memory.
uint32_t wf_max_cap(Ctx* c, const pt::PassKnobs& knobs) {
    if (c->wf_max_cap) return c->wf_max_cap;
    if (knobs.wf_max_cap_set) return c->wf_max_cap = pt::wf_cap_for_limit(knobs.wf_max_cap);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = total_b = (size_t)pt::kWfMinCapLimit * pt::kWfBytesPerEntry * 4;
    return c->wf_max_cap = pt::wf_cap_for_budget(std::min(total_b / 2, free_b / 2));
}

void free_wavefront(Ctx* c) {
    for (auto& a : c->wf_arrays) a.release();
    c->wf_arrays.clear();
    c->Q = pt::WfQueues{};
    c->wf_cap = c->wf_scap = 0;
    c->wf_two_sets = false;
    c->acc_passes = 0;
    c->d_plist = nullptr;
    c->d_plist2 = nullptr;
    c->d_fcount = nullptr;
    c->d_snap = nullptr;
    if (c->acc_s.w) { (void)hipFree(c->acc_s.w); (void)hipFree(c->acc_s.hi); (void)hipFree(c->acc_s.big); }
    c->acc_s = pt::FixAcc{};
    c->acc_s_cap = 0;
}

template <class T>
int wf_alloc(Ctx* c, T** out, size_t n) {
    DeviceArray a;
    a.bytes = n * sizeof(T);
    hipError_t e = hipMalloc(&a.ptr, a.bytes);
    if (e != hipSuccess) return fail(PT_ERR_OUT_OF_MEMORY, std::string("hipMalloc wavefront queues: ") + hipGetErrorString(e));
    c->wf_arrays.push_back(a);
    *out = (T*)a.ptr;
    return PT_OK;
}

// two_sets: the shadow passes run on the side stream beside the next depth (pt::WfPlan::side), so the shadow rays
// of depth d and d + 1 live at once, in sets by depth parity; on one stream a depth's shadow rays are consumed
// before the next depth's shade writes its own, and both sets are the same memory.
int ensure_wavefront(Ctx* c, uint32_t cap, uint32_t scap, int32_t acc_passes, bool two_sets) {
    // the split traversal's deferred-record queues (pt_wavefront.hip k_wf_vol_* / k_wf_sdf_*)
    const bool want_sdf = c->S.num_sdf > 0 || (PT_VOL_DEFER && c->S.num_vol > 0);
    const bool want_vol = PT_VOL_DEFER && c->S.num_vol > 0;
    const bool want_heavy = c->S.route != 0;  // the routed split's queues of rays that reach a row-4 shape's box
    if (c->wf_cap >= cap && c->wf_scap >= scap && c->Q.acc.w && c->acc_passes >= acc_passes && (!two_sets || c->wf_two_sets) &&
        (!want_sdf || c->Q.sdfq) && (!want_vol || c->Q.volq) &&
        (!want_heavy || c->Q.hq))
        return PT_OK;
    cap = std::max(cap, c->wf_cap);
    scap = std::max(scap, c->wf_scap);
    acc_passes = std::max(acc_passes, c->acc_passes);
    two_sets = two_sets || c->wf_two_sets;
    free_wavefront(c);
    pt::WfQueues Q{};
    int rc;
    for (int q = 0; q < 2; q++) {
        if ((rc = wf_alloc(c, &Q.q_o[q], cap))) return rc;
        if ((rc = wf_alloc(c, &Q.q_d[q], cap))) return rc;
        if ((rc = wf_alloc(c, &Q.q_t[q], cap))) return rc;
        if ((rc = wf_alloc(c, &Q.q_k[q], cap))) return rc;
    }
    if ((rc = wf_alloc(c, &Q.hits, cap))) return rc;
    if (want_sdf && (rc = wf_alloc(c, &Q.sdfq, cap))) return rc;
    if (want_vol && (rc = wf_alloc(c, &Q.volq, cap))) return rc;
    for (int q = 0; q < (two_sets ? 2 : 1); q++) {   // shadow-ray sets by depth parity
        if ((rc = wf_alloc(c, &Q.n_o[q], scap))) return rc;
        if ((rc = wf_alloc(c, &Q.n_n[q], scap))) return rc;
        if ((rc = wf_alloc(c, &Q.n_w[q], 2 * (size_t)scap))) return rc;
        if ((rc = wf_alloc(c, &Q.n_lit[q], scap))) return rc;
    }
    if (!two_sets) {   // one stream: set 1 is set 0's memory
        Q.n_o[1] = Q.n_o[0];
        Q.n_n[1] = Q.n_n[0];
        Q.n_w[1] = Q.n_w[0];
        Q.n_lit[1] = Q.n_lit[0];
    }
    if (want_sdf && (rc = wf_alloc(c, &Q.sdfq_sh, scap))) return rc;   // one shadow pass at a time uses it
    if (want_vol && (rc = wf_alloc(c, &Q.volq_sh, scap))) return rc;
    if (want_heavy && (rc = wf_alloc(c, &Q.hq, cap))) return rc;
    if (want_heavy && (rc = wf_alloc(c, &Q.hq_sh, scap))) return rc;   // one shadow pass at a time uses it
    // the head pass' lists (pt_wavefront.hip k_wf_trace_head / k_wf_shadow_head)
    if ((rc = wf_alloc(c, &Q.tlist, cap))) return rc;
    if ((rc = wf_alloc(c, &Q.slist, scap))) return rc;   // one shadow pass at a time uses it
    if ((rc = wf_alloc(c, &Q.counts, pt::kCountWords))) return rc;
    Q.overflow = c->d_counters + pt::kOverflowCounter;
    // spill columns: one region for the closest-hit kernels, one for the shadow kernels (they
    // can run at the same time on the side stream)
    const size_t ovf_words = (size_t)(pt::kStackMax - pt::kLdsStack) * pt::kWfMaxThreads;
    if ((rc = wf_alloc(c, &Q.ovf, 2 * ovf_words))) return rc;
    Q.ovf_sh = Q.ovf + ovf_words;
    // per-pixel accumulators of one pass, or of each pass of a batch (pt_pass_params.passes)
    size_t P = (size_t)c->width * (size_t)c->height * (size_t)acc_passes;
    if ((rc = wf_alloc(c, &Q.acc.w, P * pt::kFixWords))) return rc;
    if ((rc = wf_alloc(c, &Q.acc.hi, P * pt::kFixWords))) return rc;
    if ((rc = wf_alloc(c, &Q.acc.big, P * 3))) return rc;
    Q.acc.n = P;   // channel-planar (pt_accum.h FixAcc)
    PT_HIP(hipMemsetAsync(Q.acc.w, 0, P * pt::kFixWords * sizeof(unsigned long long), c->stream));
    PT_HIP(hipMemsetAsync(Q.acc.hi, 0, P * pt::kFixWords * sizeof(unsigned long long), c->stream));
    PT_HIP(hipMemsetAsync(Q.acc.big, 0, P * 3 * sizeof(double), c->stream));
    PT_HIP(hipMemsetAsync(Q.counts, 0, pt::kCountWords * sizeof(uint32_t), c->stream));
    Q.cap = cap;
    Q.s_cap = scap;
    Q.pcap = cap / pt::kParts;
    Q.spcap = scap / pt::kParts;
    c->Q = Q;
    c->wf_cap = cap;
    c->wf_scap = scap;
    c->wf_two_sets = two_sets;
    c->acc_passes = acc_passes;
    return PT_OK;
}

// Buffers of the adaptive / firefly phases: per-sample accumulators for one chunk
// of camera samples, the candidate list and the M snapshot.
int ensure_extra(Ctx* c, uint64_t chunk) {
    if (c->acc_s.w && c->acc_s_cap >= chunk) { c->Q.acc_s = c->acc_s; return PT_OK; }
    int rc;
    const size_t P = (size_t)c->width * (size_t)c->height;
    if (!c->d_plist) {
        if ((rc = wf_alloc(c, &c->d_plist, P))) return rc;
        if ((rc = wf_alloc(c, &c->d_plist2, P))) return rc;
        if ((rc = wf_alloc(c, &c->d_fcount, 2))) return rc;
        if ((rc = wf_alloc(c, &c->d_snap, P * 3))) return rc;
    }
    if (c->acc_s.w) {
        (void)hipFree(c->acc_s.w); (void)hipFree(c->acc_s.hi); (void)hipFree(c->acc_s.big);
        c->acc_s = pt::FixAcc{}; c->acc_s_cap = 0;
    }
    c->Q.acc_s = pt::FixAcc{};
    if (hipMalloc(&c->acc_s.w, chunk * pt::kFixWords * sizeof(unsigned long long)) != hipSuccess)
        return fail(PT_ERR_OUT_OF_MEMORY, "hipMalloc per-sample accumulators");
    if (hipMalloc(&c->acc_s.hi, chunk * pt::kFixWords * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&c->acc_s.big, chunk * 3 * sizeof(double)) != hipSuccess) {
        (void)hipFree(c->acc_s.w);
        if (c->acc_s.hi) (void)hipFree(c->acc_s.hi);
        c->acc_s = pt::FixAcc{};
        return fail(PT_ERR_OUT_OF_MEMORY, "hipMalloc per-sample accumulators");
    }
    c->acc_s_cap = chunk;
    c->acc_s.n = chunk;
    PT_HIP(hipMemsetAsync(c->acc_s.w, 0, chunk * pt::kFixWords * sizeof(unsigned long long), c->stream));
    PT_HIP(hipMemsetAsync(c->acc_s.hi, 0, chunk * pt::kFixWords * sizeof(unsigned long long), c->stream));
    PT_HIP(hipMemsetAsync(c->acc_s.big, 0, chunk * 3 * sizeof(double), c->stream));
    c->Q.acc_s = c->acc_s;
    return PT_OK;
}

template <class T>
int upload(Ctx* c, const std::vector<T>& host, const T** out) {
    *out = nullptr;
    if (host.empty()) return PT_OK;
    DeviceArray a;
    a.bytes = host.size() * sizeof(T);
    hipError_t e = hipMalloc(&a.ptr, a.bytes);
    if (e != hipSuccess) return fail(PT_ERR_OUT_OF_MEMORY, std::string("hipMalloc scene: ") + hipGetErrorString(e));
    c->scene_arrays.push_back(a);
    PT_HIP(hipMemcpyAsync(a.ptr, host.data(), a.bytes, hipMemcpyHostToDevice, c->stream));
    *out = (const T*)a.ptr;
    return PT_OK;
}

void free_scene(Ctx* c) {
    for (auto& a : c->scene_arrays) a.release();
    c->scene_arrays.clear();
    c->dyn.release_device();
    c->dyn = SceneDyn{};
    c->S = pt::DevScene{};
    c->has_scene = false;
}

bool env_off(const char* name) {   // "0": the option is off for this upload (tests)
    const char* v = std::getenv(name);
    return v && !std::strcmp(v, "0");
}

// Copies a compiled scene's arrays (pt_scene_compile.h) to the device and returns its DevScene with the
// pointer fields derived from their addresses.  The host arrays are in use until the stream is synchronised.
int upload_host_scene(Ctx* c, const pt::HostScene& H, std::vector<pt::DevTexture>& texs, std::vector<pt::DevVolume>& vols,
                      pt::DevScene& S) {
    int rc;
    S = H.S;
    if ((rc = upload(c, H.lines, &S.lines))) return rc;
    S.ana_nodes = S.tri_node_line0 == 0 ? nullptr : S.lines;
    S.tri_nodes = S.tri_chunk_line0 == S.tri_node_line0 ? nullptr : S.lines + 8 * (size_t)S.tri_node_line0;
    S.tri_chunks = S.lines_n == S.tri_chunk_line0 ? nullptr : S.lines + 8 * (size_t)S.tri_chunk_line0;
    const float4* d_tri_sh = nullptr;
    if ((rc = upload(c, H.tri_sh, &d_tri_sh))) return rc;
    S.tri_recs = d_tri_sh;
    S.tri_shade = d_tri_sh ? d_tri_sh + 3 : nullptr;
    S.tri_uv = d_tri_sh && H.tri_uv ? d_tri_sh + 6 : nullptr;
    if ((rc = upload(c, H.ana_recs, &S.ana_recs))) return rc;
    if ((rc = upload(c, H.planes, &S.planes))) return rc;
    if ((rc = upload(c, H.mats, &S.mats))) return rc;
    if ((rc = upload(c, H.lights, &S.lights))) return rc;
    const double* d_tex = nullptr;
    if ((rc = upload(c, H.tex_data, &d_tex))) return rc;
    for (const pt::HostTexture& t : H.texs) texs.push_back(pt::DevTexture{d_tex + t.off, t.w, t.h});
    if ((rc = upload(c, texs, &S.texs))) return rc;
    if ((rc = upload(c, H.sdf_prog, &S.sdf_prog))) return rc;
    if ((rc = upload(c, H.sdf_params, &S.sdf_params))) return rc;
    if ((rc = upload(c, H.sdf_shapes, &S.sdf_shapes))) return rc;
    const double* d_vox = nullptr;
    const pt::DevWindow* d_win = nullptr;
    const int8_t* d_runs = nullptr;
    const double* d_cells = nullptr;
    if ((rc = upload(c, H.vox, &d_vox))) return rc;
    if ((rc = upload(c, H.windows, &d_win))) return rc;
    if ((rc = upload(c, H.vol_runs, &d_runs))) return rc;
    if ((rc = upload(c, H.vol_cells, &d_cells))) return rc;
    for (const pt::HostVolume& v : H.volumes) {
        vols.push_back(v.v);
        vols.back().data = d_vox + v.vox_off;
        vols.back().windows = d_win ? d_win + v.win_off : nullptr;
        vols.back().runs = d_runs ? d_runs + v.runs_off : nullptr;
        vols.back().cells = v.cells_off >= 0 ? d_cells + v.cells_off : nullptr;
    }
    if ((rc = upload(c, vols, &S.volumes))) return rc;
    if ((rc = upload(c, H.xforms, &S.xforms))) return rc;
    if ((rc = upload(c, H.ext_recs, &S.ext_recs))) return rc;
    if ((rc = upload(c, H.blas, &S.blas))) return rc;
    if ((rc = upload(c, H.blas_nodes, &S.blas_nodes))) return rc;
    if ((rc = upload(c, H.blas_recs, &S.blas_recs))) return rc;
    if ((rc = upload(c, H.blas_shade, &S.blas_shade))) return rc;
    if ((rc = upload(c, H.blas_uv, &S.blas_uv))) return rc;
    return upload(c, H.heavy, &S.heavy);
}

}  // namespace

extern "C" {

int pt_get_version(void) { return PT_ABI_VERSION; }

const char* pt_last_error(void) { return g_last_error.c_str(); }

int pt_device_count(int32_t* out_count) {
    if (!out_count) return fail(PT_ERR_INVALID_ARG, "out_count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *out_count = 0; return fail(PT_ERR_NO_DEVICE, hipGetErrorString(e)); }
    *out_count = n;
    return PT_OK;
}

int pt_create(const pt_device_opts* opts, void** out_ctx) {
    if (!opts || !out_ctx) return fail(PT_ERR_INVALID_ARG, "NULL argument");
    *out_ctx = nullptr;
    // A Buffer one pixel wide or high can be loaded and resolved to an image, not rendered into
    // (render_pass_impl); a single pixel is no image.
    if (opts->width < 1 || opts->height < 1 || (opts->width == 1 && opts->height == 1))
        return fail(PT_ERR_INVALID_ARG, "width/height must be >= 1 and not both 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PT_ERR_NO_DEVICE, "no HIP device");
    if (opts->device < 0 || opts->device >= ndev) return fail(PT_ERR_INVALID_ARG, "device ordinal out of range");
    Ctx* c = new (std::nothrow) Ctx();
    if (!c) return fail(PT_ERR_OUT_OF_MEMORY, "context allocation");
    c->device = opts->device;
    c->width = opts->width;
    c->height = opts->height;
    auto cleanup = [&](int code) { pt_destroy(c); return code; };
    if (hipSetDevice(c->device) != hipSuccess) return cleanup(fail(PT_ERR_HIP, "hipSetDevice"));
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return cleanup(fail(PT_ERR_HIP, "stream"));
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess)
        return cleanup(fail(PT_ERR_HIP, "events"));
    if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_side[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_side[1], hipEventDisableTiming) != hipSuccess)
        return cleanup(fail(PT_ERR_HIP, "side stream"));
    size_t P = (size_t)c->width * (size_t)c->height;
    if (hipMalloc(&c->d_m, P * 3 * sizeof(double)) != hipSuccess || hipMalloc(&c->d_v, P * 3 * sizeof(double)) != hipSuccess ||
        hipMalloc(&c->d_n, P * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&c->d_counters, pt::kCounterAllocWords * sizeof(unsigned long long)) != hipSuccess ||
        hipHostMalloc(&c->h_counters, pt::kCounterAllocWords * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess)
        return cleanup(fail(PT_ERR_OUT_OF_MEMORY, "buffer allocation"));
    int rc = pt_reset_buffer(c);
    if (rc != PT_OK) return cleanup(rc);
    *out_ctx = c;
    return PT_OK;
}

int pt_reset_buffer(void* ctx) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    PT_HIP(hipSetDevice(c->device));
    size_t P = (size_t)c->width * (size_t)c->height;
    PT_HIP(hipMemsetAsync(c->d_m, 0, P * 3 * sizeof(double), c->stream));
    PT_HIP(hipMemsetAsync(c->d_v, 0, P * 3 * sizeof(double), c->stream));
    PT_HIP(hipMemsetAsync(c->d_n, 0, P * sizeof(int32_t), c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    c->stats.rays_total = 0;
    c->stats.total_ms = 0;
    c->stats.passes = 0;
    return PT_OK;
}

int pt_upload_scene(void* ctx, const pt_scene_desc* d) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    std::string err;
    int rc = pt::validate_scene(d, err);   // a scene that does not validate leaves the context's scene as it is
    if (rc != PT_OK) return fail(rc, err);
    pt::CompileOptions opt;   // read at each upload: tests flip them between uploads
    opt.vol_cells = !env_off("PT_VOL_CELLS");
    opt.vol_lds = !env_off("PT_VOL_LDS");
    opt.route = !env_off("PT_ROUTE");
    if (const char* f = std::getenv("PT_POP_CULL_BITS")) opt.pop_cull_bits = std::max(0, std::min(opt.pop_cull_bits, std::atoi(f)));
    if (env_off("PT_POP_CULL")) opt.pop_cull_bits = 0;
    PT_HIP(hipSetDevice(c->device));
    auto t0 = std::chrono::steady_clock::now();
    free_scene(c);
    pt::HostScene H;
    rc = pt::compile_scene(d, opt, H, err);
    // the previous upload's build goes after the new one was looked up, so re-uploading a geometry finds it;
    // a failed compile leaves the context without scene and without build
    const auto t1 = std::chrono::steady_clock::now();
    pt::tri_bvh_release(c->tri_build);
    c->tri_build = std::move(H.tri_build);
    c->tri_build_ms = H.tri_build_ms + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    if (rc != PT_OK) return fail(rc, err);
    std::vector<pt::DevTexture> texs;
    std::vector<pt::DevVolume> vols;
    pt::DevScene S{};
    if ((rc = upload_host_scene(c, H, texs, vols, S))) return rc;
    PT_HIP(hipStreamSynchronize(c->stream));
    c->S = S;
    c->has_scene = true;
    c->dyn.refit = std::move(H.refit);
    c->dyn.shape_refit = std::move(H.shape_refit);
    c->dyn.blas_refit = std::move(H.blas_refit);
    c->dyn.query = std::move(H.query);
    c->dyn.h_lights = std::move(H.lights);
    c->dyn.lights_cap = c->dyn.h_lights.size();
    c->dyn.look = std::move(H.look);
    c->dyn.h_mats = std::move(H.mats);
    c->dyn.texs = std::move(texs);
    c->dyn.has_blas = !H.blas.empty();
    c->dyn.num_xforms = (int64_t)H.xforms.size();
    c->dyn.num_ext_recs = (int64_t)H.ext_recs.size() / 3;
    c->dyn.h_blas = H.blas;
    for (const pt::DevBlas& b : H.blas) c->dyn.blas_node_cap.push_back(b.num_nodes);
    c->dyn.volume_update = std::move(H.volume_update);
    c->dyn.vols = std::move(vols);
    c->dyn.vol_windows = std::move(H.windows);
    for (const pt::HostVolume& v : H.volumes) c->dyn.vol_win_off.push_back(v.win_off);
    c->stats.bvh_nodes = H.bvh_nodes;
    c->stats.traversal_bytes = H.traversal_bytes;
    c->stats.bvh_bytes = H.bvh_bytes;
    c->stats.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PT_OK;
}

// Passes one batch may hold (pt::batch_passes_for): its accumulator sets, pt::kFixWords 64-bit words twice + 3 fp64
// side sums per pixel and pass.
static int32_t batch_passes_max(Ctx* c, const pt::PassKnobs& knobs) {
    const size_t per_pass = (size_t)c->width * (size_t)c->height *
                            (2 * pt::kFixWords * sizeof(unsigned long long) + 3 * sizeof(double));
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || total_b == 0) total_b = (size_t)8 << 30;
    return pt::batch_passes_for(total_b, per_pass, knobs.batch_max_passes);
}

// The environment's switches of a pass (pt::PassKnobs; tests, A/B runs), read at each pt_render_pass call: tests
// change them between the passes of one process.
static pt::PassKnobs read_pass_knobs() {
    pt::PassKnobs k;
    if (const char* f = std::getenv("PT_SHADE_FORM")) k.shade_form = !std::strcmp(f, "direct") ? 1 : !std::strcmp(f, "scan") ? 2 : 0;
    if (const char* f = std::getenv("PT_LANES")) k.lanes = !std::strcmp(f, "0") ? 0 : !std::strcmp(f, "1") ? 1 : -1;
    if (const char* f = std::getenv("PT_HEAD")) k.head = !std::strcmp(f, "0") ? 0 : 1;
    if (const char* f = std::getenv("PT_HEAD_STATS")) k.head_stats = !std::strcmp(f, "1") ? 1 : 0;
    if (const char* f = std::getenv("PT_LINEAR")) k.linear = !std::strcmp(f, "0") ? 0 : -1;
    if (const char* f = std::getenv("PT_SIDE_STREAM")) k.side_stream = !std::strcmp(f, "1") ? 1 : !std::strcmp(f, "0") ? 0 : -1;
    if (const char* f = std::getenv("PT_SHADOW_TAIL")) k.tail_early = !std::strcmp(f, "early") ? 1 : 0;
    if (const char* f = std::getenv("PT_ESCAPE_DROP")) k.escape_drop = !std::strcmp(f, "0") ? 0 : !std::strcmp(f, "all") ? 2 : 1;
    if (const char* f = std::getenv("PT_BATCH_MAX_PASSES")) k.batch_max_passes = std::max(1LL, std::atoll(f));
    if (const char* f = std::getenv("PT_WF_MAX_CAP")) {
        k.wf_max_cap_set = true;
        k.wf_max_cap = std::strtoull(f, nullptr, 10);
    }
    return k;
}

// What a pass' launches take: the kernels' arguments, and on the wavefront engine its plan.
struct PassRun {
    pt::DevCamera cam;
    pt::DevSampler smp;
    pt::DevPass P;
    pt::DevBuffer B;
    pt::WfPlan wf{};
    bool count = false;               // a counted pass
    pt::LaunchTimer* tm = nullptr;    // PT_PASS_KERNEL_TIMING
};

// The pass' tile list on the device, uploaded when it differs from the last pass' (*d_tiles null: every tile).
static int upload_tile_list(Ctx* c, const pt_pass_params* pass, int image_tiles, const int32_t** d_tiles) {
    *d_tiles = nullptr;
    if (pass->num_tiles > 0) {
        if (!pass->tiles) return fail(PT_ERR_INVALID_ARG, "tiles is NULL");
        if (pass->num_tiles > c->tiles_cap) {
            if (c->d_tiles) (void)hipFree(c->d_tiles);
            c->d_tiles = nullptr;
            c->h_tiles.clear();
            PT_HIP(hipMalloc(&c->d_tiles, (size_t)pass->num_tiles * sizeof(int32_t)));
            c->tiles_cap = pass->num_tiles;
        }
        // the same list pass after pass (a rank's tiles): uploaded once
        if (c->h_tiles.size() != (size_t)pass->num_tiles ||
            std::memcmp(c->h_tiles.data(), pass->tiles, (size_t)pass->num_tiles * sizeof(int32_t))) {
            // ids in range, none twice (a tile listed twice would be rendered into its pixels twice)
            if (int rc = pt_tile_lists_check(pass->tiles, pass->num_tiles, image_tiles)) return rc;
            c->h_tiles.assign(pass->tiles, pass->tiles + pass->num_tiles);
            PT_HIP(hipMemcpyAsync(c->d_tiles, c->h_tiles.data(), (size_t)pass->num_tiles * sizeof(int32_t),
                                  hipMemcpyHostToDevice, c->stream));
        }
        *d_tiles = c->d_tiles;
    }
    c->pass_tiles = pass->num_tiles > 0 ? pass->num_tiles : 0;
    return PT_OK;
}

// The wavefront engine's queues and buffers for this plan, and the plan as its launches take it.
static int prepare_wavefront(Ctx* c, const pt_pass_params* pass, const pt::PassPlan& plan, const pt::PassKnobs& knobs,
                             pt::WfPlan& wf) {
    if (!c->grids.complete()) PT_HIP(pt::wavefront_grids(c->grids));
    if (int rc = ensure_wavefront(c, plan.cap, plan.scap, plan.passes_per_launch, plan.use_side)) return rc;
    if (pass->adaptive_samples > 0 || pass->firefly_samples > 0)
        if (int rc = ensure_extra(c, plan.chunk_extra)) return rc;
    static_cast<pt::WfGrids&>(wf) = c->grids;
    static_cast<pt::PassPlan&>(wf) = plan;
    static_cast<pt::PassKnobs&>(wf) = knobs;
    if (plan.use_side) {
        wf.side = c->side;
        wf.ev_main = c->ev_main;
        wf.ev_side[0] = c->ev_side[0];
        wf.ev_side[1] = c->ev_side[1];
    }
    // PT_SHADOW_TAIL=early: k_wf_shadow_lanes hands stack entries to idle lanes from the first claim on, so the
    // tail protocol runs all pass long (pt_stats.tail_handoffs counts it)
    c->Q.tail_early = knobs.tail_early;
    return PT_OK;
}

// After a gather or a loaded checkpoint the Buffer holds other ranks' tiles: a tile-subset pass clears them
// before it adds to its own (k_clear_foreign).
static int clear_foreign_tiles(Ctx* c, const pt_pass_params* pass, const pt::DevBuffer& B, int tiles_x, int image_tiles) {
    if (!(c->gathered || (c->loaded && c->comm))) return PT_OK;
    c->gathered = false;
    c->loaded = false;
    if (pass->num_tiles <= 0) return PT_OK;
    std::vector<uint8_t> own((size_t)image_tiles, 0);
    for (int i = 0; i < pass->num_tiles; i++) own[(size_t)pass->tiles[i]] = 1;
    if (!c->d_own) PT_HIP(hipMalloc(&c->d_own, (size_t)image_tiles));
    PT_HIP(hipMemcpyAsync(c->d_own, own.data(), (size_t)image_tiles, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(pt::k_clear_foreign, dim3(2048), dim3(256), 0, c->stream, B, c->width, c->height, tiles_x,
                       (const uint8_t*)c->d_own);
    PT_HIP(hipGetLastError());
    PT_HIP(hipStreamSynchronize(c->stream));   // `own` is a host temporary
    return PT_OK;
}

// Renderer.Render's extra phases (PT_PASS_SERIAL; Renderer.cs:80-198): after a pixel's main samples,
// AdaptiveSamples individual samples if its σmax ≥ 1 (:153-175), then FireflySamples individual samples
// if its σmax then exceeds 1 (:177-191).  Each decision reads the pixel's own Buffer
// only, so the phases run over all pixels, one after the other.
static int run_extra_serial(Ctx* c, const pt_pass_params* pass, const PassRun& r) {
    const int32_t K[2] = {pass->adaptive_samples, pass->firefly_samples};
    const uint32_t base[2] = {pt::kAdaptiveSampleBase, pt::kFireflySampleBase};
    for (int ph = 0; ph < 2; ph++) {
        if (K[ph] <= 0) continue;
        PT_HIP(pt::select_pixels(r.P, r.B, ph == 0 ? 1 : 0, c->d_plist, c->d_fcount, c->stream));
        uint32_t nsel = 0;
        PT_HIP(hipMemcpyAsync(&nsel, c->d_fcount, sizeof nsel, hipMemcpyDeviceToHost, c->stream));
        PT_HIP(hipStreamSynchronize(c->stream));
        PT_HIP(pt::wavefront_extra(c->S, r.cam, r.smp, r.P, r.B, c->Q, r.wf, r.count, c->stream, r.tm,
                                   ph == 0 ? pt::EXTRA_ADD : pt::EXTRA_ADD_SCALED, K[ph], base[ph], nsel,
                                   c->d_plist, nullptr, nullptr, nullptr));
    }
    return PT_OK;
}

// RenderParallel's extra phases: every pixel's adaptive samples (Renderer.cs:340-410), then the firefly rounds
// (Renderer.cs:412-470).
static int run_extra_parallel(Ctx* c, const pt_pass_params* pass, const PassRun& r) {
    if (pass->adaptive_samples > 0)
        PT_HIP(pt::wavefront_extra(c->S, r.cam, r.smp, r.P, r.B, c->Q, r.wf, r.count, c->stream, r.tm, 0,
                                   pass->adaptive_samples, pt::kAdaptiveSampleBase, (uint64_t)r.P.num_tiles * 1024u,
                                   nullptr, nullptr, nullptr, nullptr));
    if (pass->firefly_samples <= 0) return PT_OK;
    PT_HIP(pt::select_pixels(r.P, r.B, 0, c->d_plist, c->d_fcount, c->stream));
    uint32_t nsel = 0;
    PT_HIP(hipMemcpyAsync(&nsel, c->d_fcount, sizeof nsel, hipMemcpyDeviceToHost, c->stream));
    const size_t npx = (size_t)c->width * (size_t)c->height;
    PT_HIP(hipMemcpyAsync(c->d_snap, c->d_m, npx * 3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (c->comm) {
        // neighbours on other ranks' tiles: the disjoint M buffers sum to the full frame
        ncclResult_t e = ncclAllReduce(c->d_snap, c->d_snap, npx * 3, ncclFloat64, ncclSum, c->comm, c->stream);
        if (e != ncclSuccess) return fail(PT_ERR_RCCL, std::string("ncclAllReduce: ") + ncclGetErrorString(e));
    }
    PT_HIP(hipStreamSynchronize(c->stream));
    // Renderer.cs:430-445 traces a candidate's samples one after another and stops at the first
    // IsFirefly sample: rounds of one sample per still-active pixel, so exactly those samples are
    // traced (and counted in Scene.rays), no more.
    uint32_t* list = c->d_plist;
    uint32_t* next = c->d_plist2;
    for (int j = 0; j < pass->firefly_samples && nsel > 0; j++) {
        PT_HIP(hipMemsetAsync(c->d_fcount + 1, 0, sizeof(uint32_t), c->stream));
        PT_HIP(pt::wavefront_extra(c->S, r.cam, r.smp, r.P, r.B, c->Q, r.wf, r.count, c->stream, r.tm,
                                   pt::EXTRA_FIREFLY_STOP, 1, pt::kFireflySampleBase + (uint32_t)j, nsel, list, c->d_snap,
                                   next, c->d_fcount + 1));
        PT_HIP(hipMemcpyAsync(&nsel, c->d_fcount + 1, sizeof nsel, hipMemcpyDeviceToHost, c->stream));
        PT_HIP(hipStreamSynchronize(c->stream));
        std::swap(list, next);
    }
    return PT_OK;
}

// The pass' launches, between the two events that time it.
static int run_pass(Ctx* c, const pt_pass_params* pass, int engine, const PassRun& r) {
    c->timer.reset(c->stream);
    PT_HIP(hipMemsetAsync(c->d_counters, 0, (r.count ? pt::kCounterAllocWords : pt::kCounterWords) * sizeof(unsigned long long),
                          c->stream));   // and the overflow flag; a counted pass' march clock slots too
    // a counted pass also counts the Volume / SDFShape march steps (counters 9, 10); the launches
    // take the scene by value, so the pointer is cleared again whichever way this call returns
    struct MarchScope {
        pt::DevScene& S;
        ~MarchScope() { S.march = nullptr; }
    } march_scope{c->S};
    c->S.march = r.count ? c->d_counters + 9 : nullptr;
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    if (engine == PT_ENGINE_WAVEFRONT) {
        PT_HIP(pt::wavefront_pass(c->S, r.cam, r.smp, r.P, r.B, c->Q, r.wf, r.count, c->stream, r.tm));
        if (int rc = (pass->flags & PT_PASS_SERIAL) ? run_extra_serial(c, pass, r) : run_extra_parallel(c, pass, r)) return rc;
    } else {
        if (r.tm) r.tm->begin(PT_K_MEGAKERNEL, c->stream);
        PT_HIP(pt::launch_render_pass(c->S, r.cam, r.smp, r.P, r.B, r.P.num_tiles, r.count, c->stream));
        if (r.tm) r.tm->end(PT_K_MEGAKERNEL, c->stream);
    }
    PT_HIP(hipEventRecord(c->ev1, c->stream));
    if (c->timer.failed) return fail(PT_ERR_HIP, "hipEventRecord (kernel timing) failed");
    return PT_OK;
}

// A counted pass' counters as pt_render_pass_counted returns them.
// counters: [0..2] closest-hit rays/nodes/prims, [3] shading fetches, [4..6] shadow rays/nodes/prims
static void read_trace_counters(const unsigned long long* ctr, pt_trace_counters* counted) {
    counted->rays = ctr[0] + ctr[4];
    counted->nodes_visited = ctr[1] + ctr[5];
    counted->prims_tested = ctr[2] + ctr[6];
    counted->shading_fetches = ctr[3];
    counted->shadow_rays = ctr[4];
    counted->shadow_nodes = ctr[5];
    counted->shadow_prims = ctr[6];
    counted->lit_shadow_rays = ctr[7];
    counted->accum_runs = ctr[8];
    counted->volume_samples = ctr[9];
    counted->sdf_evals = ctr[10];
    for (int k = 0; k < 8; k++) {
        counted->march_clock[k] = 0;
        for (int j = 0; j < pt::kMarchSlots; j++) counted->march_clock[k] += ctr[pt::kMarchClockWord + 8 * j + k];
    }
}

// Waits for the pass, reads its counters back and fills pt_stats (and `counted`).
static int collect_stats(Ctx* c, int engine, int32_t passes, bool timing, pt_trace_counters* counted) {
    const unsigned long long* ctr = c->h_counters;
    PT_HIP(hipMemcpyAsync(c->h_counters, c->d_counters, (counted ? pt::kCounterAllocWords : pt::kCounterWords) * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    if (engine == PT_ENGINE_WAVEFRONT && ctr[pt::kOverflowCounter])
        return fail(PT_ERR_OUT_OF_MEMORY, "wavefront queue overflow (pass results are incomplete)");
    float ms = 0.f;
    PT_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    const uint64_t rays = ctr[0] + ctr[4];
    c->stats.rays = rays;
    c->stats.shadow_rays = ctr[4];
    c->stats.tail_handoffs = engine == PT_ENGINE_WAVEFRONT ? ctr[11] : 0;
    c->stats.rays_total += rays;
    c->stats.last_pass_ms = ms;
    c->stats.total_ms += ms;
    c->stats.passes += (uint64_t)passes;
    for (int k = 0; k < PT_K_SLOTS; k++) { c->stats.kernel_ms[k] = 0.0; c->stats.kernel_launches[k] = 0; }
    if (timing) PT_HIP(c->timer.collect(c->stats.kernel_ms, c->stats.kernel_launches));
    if (counted) read_trace_counters(ctr, counted);
    return PT_OK;
}

static int render_pass_impl(Ctx* c, const pt_camera* camera, const pt_sampler* sampler, const pt_pass_params* pass,
                            const pt::PassKnobs& knobs, pt_trace_counters* counted);

// A call's K passes that do not run as one batch (pt::PassPlan::split_step): one after another, or in sub-batches
// of `step` passes, the stats summed.
static int render_passes_split(Ctx* c, const pt_camera* camera, const pt_sampler* sampler, const pt_pass_params* pass,
                               const pt::PassKnobs& knobs, int32_t step) {
    pt_pass_params one = *pass;
    pt_stats sum = c->stats;
    uint64_t rays = 0, shadow = 0, handoffs = 0;
    double ms = 0.0;
    for (int32_t k = 0; k < pass->passes; k += step) {
        one.pass_index = pass->pass_index + (uint32_t)k;
        one.passes = std::min(step, pass->passes - k);
        if (int rc = render_pass_impl(c, camera, sampler, &one, knobs, nullptr)) return rc;
        rays += c->stats.rays;
        shadow += c->stats.shadow_rays;
        handoffs += c->stats.tail_handoffs;
        ms += c->stats.last_pass_ms;
        for (int j = 0; j < PT_K_SLOTS; j++) {
            sum.kernel_ms[j] = (k ? sum.kernel_ms[j] : 0.0) + c->stats.kernel_ms[j];
            sum.kernel_launches[j] = (k ? sum.kernel_launches[j] : 0) + c->stats.kernel_launches[j];
        }
    }
    std::memcpy(c->stats.kernel_ms, sum.kernel_ms, sizeof sum.kernel_ms);
    std::memcpy(c->stats.kernel_launches, sum.kernel_launches, sizeof sum.kernel_launches);
    c->stats.rays = rays;
    c->stats.shadow_rays = shadow;
    c->stats.tail_handoffs = handoffs;
    c->stats.last_pass_ms = ms;
    return PT_OK;
}

// One pt_render_pass call: validate, tile list, plan (pt_pass_plan.h), batch split, queues and buffers, foreign
// tiles, run, stats.
static int render_pass_impl(Ctx* c, const pt_camera* camera, const pt_sampler* sampler, const pt_pass_params* pass,
                            const pt::PassKnobs& knobs, pt_trace_counters* counted) {
    if (!c || !camera || !sampler || !pass) return fail(PT_ERR_INVALID_ARG, "NULL argument");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "pt_render_pass before pt_upload_scene");
    if (c->width <= 1 || c->height <= 1)   // Camera.CastRay divides by w - 1 and h - 1 (Camera.cs:101-102)
        return fail(PT_ERR_INVALID_ARG, "a pass needs width and height > 1");
    const int tiles_x = (c->width + 31) / 32, image_tiles = tiles_x * ((c->height + 31) / 32);
    pt::PassPlanInput in;
    in.width = c->width; in.height = c->height;
    in.num_tiles = pass->num_tiles > 0 ? pass->num_tiles : image_tiles;
    in.spp = pass->spp; in.stratified = pass->stratified; in.engine = pass->engine; in.flags = pass->flags;
    in.adaptive_samples = pass->adaptive_samples; in.firefly_samples = pass->firefly_samples; in.passes = pass->passes;
    in.first_hit_samples = sampler->first_hit_samples; in.max_bounces = sampler->max_bounces;
    in.light_mode = sampler->light_mode; in.specular_mode = sampler->specular_mode;
    in.num_lights = c->S.num_lights;
    in.counted = counted != nullptr;
    in.knobs = knobs;
    // (plan_pass makes these checks first too; here they also come before the tile list's, as they always have)
    pt::PassPlan plan = pt::check_pass_params(in);
    if (plan.rc != PT_OK) return fail(plan.rc, plan.message);
    PT_HIP(hipSetDevice(c->device));
    const int32_t* d_tiles = nullptr;
    if (int rc = upload_tile_list(c, pass, image_tiles, &d_tiles)) return rc;
    in.wf_max_cap = wf_max_cap(c, knobs);
    if (pass->passes > 1) in.batch_passes_max = batch_passes_max(c, knobs);
    plan = pt::plan_pass(in);
    if (plan.rc != PT_OK) return fail(plan.rc, plan.message);
    if (plan.split_step > 0) return render_passes_split(c, camera, sampler, pass, knobs, plan.split_step);
    PassRun r;
    std::memcpy(r.cam.p, camera->p, sizeof r.cam.p); std::memcpy(r.cam.u, camera->u, sizeof r.cam.u);
    std::memcpy(r.cam.v, camera->v, sizeof r.cam.v); std::memcpy(r.cam.w, camera->w, sizeof r.cam.w);
    r.cam.m = camera->m; r.cam.focal_distance = camera->focal_distance; r.cam.aperture_radius = camera->aperture_radius;
    r.smp = pt::DevSampler{sampler->first_hit_samples, sampler->max_bounces, sampler->direct_lighting, sampler->soft_shadows,
                           sampler->light_mode, sampler->specular_mode};
    r.P = pt::DevPass{c->width, c->height, pass->spp, pass->stratified, pass->seed, pass->pass_index, tiles_x, d_tiles,
                      in.num_tiles};
    r.P.passes = plan.passes_per_launch;
    r.P.acc_stride = (uint32_t)((size_t)c->width * (size_t)c->height);
    r.B = pt::DevBuffer{c->d_m, c->d_v, c->d_n, c->d_counters};
    r.count = counted != nullptr;
    r.tm = (pass->flags & PT_PASS_KERNEL_TIMING) ? &c->timer : nullptr;
    if (plan.engine == PT_ENGINE_WAVEFRONT)
        if (int rc = prepare_wavefront(c, pass, plan, knobs, r.wf)) return rc;
    c->last_engine = plan.engine;
    if (int rc = clear_foreign_tiles(c, pass, r.B, tiles_x, image_tiles)) return rc;
    if (int rc = run_pass(c, pass, plan.engine, r)) return rc;
    return collect_stats(c, plan.engine, r.P.passes, r.tm != nullptr, counted);
}

int pt_render_pass(void* ctx, const pt_camera* camera, const pt_sampler* sampler, const pt_pass_params* pass) {
    return render_pass_impl((Ctx*)ctx, camera, sampler, pass, read_pass_knobs(), nullptr);
}

int pt_render_pass_counted(void* ctx, const pt_camera* camera, const pt_sampler* sampler, const pt_pass_params* pass,
                           pt_trace_counters* out) {
    if (!out) return fail(PT_ERR_INVALID_ARG, "out is NULL");
    return render_pass_impl((Ctx*)ctx, camera, sampler, pass, read_pass_knobs(), out);
}

int pt_synchronize(void* ctx) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    PT_HIP(hipSetDevice(c->device));
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_read_buffer(void* ctx, double* out_m, double* out_v, int32_t* out_n) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    PT_HIP(hipSetDevice(c->device));
    size_t P = (size_t)c->width * (size_t)c->height;
    if (out_m) PT_HIP(hipMemcpyAsync(out_m, c->d_m, P * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (out_v) PT_HIP(hipMemcpyAsync(out_v, c->d_v, P * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (out_n) PT_HIP(hipMemcpyAsync(out_n, c->d_n, P * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_write_buffer(void* ctx, const double* m, const double* v, const int32_t* n) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    PT_HIP(hipSetDevice(c->device));
    size_t P = (size_t)c->width * (size_t)c->height;
    if (m) PT_HIP(hipMemcpyAsync(c->d_m, m, P * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (v) PT_HIP(hipMemcpyAsync(c->d_v, v, P * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (n) PT_HIP(hipMemcpyAsync(c->d_n, n, P * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    // The loaded Buffer may hold other ranks' pixels (every rank loads the whole checkpoint): on a
    // context that is part of a communicator the next tile-subset pass clears them first, as after a
    // gather, so a firefly snapshot's all-reduce and a later gather see each pixel on its owner only.
    // A lone context keeps them (a host resuming a frame and then rendering it tile subset by tile
    // subset keeps every restored pixel).
    c->loaded = true;
    return PT_OK;
}

int pt_read_image(void* ctx, int32_t channel, int32_t format, uint8_t* out) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !out) return fail(PT_ERR_INVALID_ARG, "NULL argument");
    if (channel < PT_CHANNEL_COLOR || channel > PT_CHANNEL_NORMAL) return fail(PT_ERR_INVALID_ARG, "channel is not a pt_channel");
    if (format != PT_IMAGE_RGB8 && format != PT_IMAGE_RGBA8) return fail(PT_ERR_INVALID_ARG, "format is not a pt_image_format");
    PT_HIP(hipSetDevice(c->device));
    const size_t P = (size_t)c->width * (size_t)c->height;
    const size_t staging = pt::image_staging_bytes(c->width, c->height);
    if (!c->d_image && hipMalloc(&c->d_image, staging + 16) != hipSuccess) {
        c->d_image = nullptr;
        return fail(PT_ERR_OUT_OF_MEMORY, "image staging allocation");
    }
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    PT_HIP(pt::launch_image_resolve(channel, format, c->d_m, c->d_v, c->d_n, (int32_t*)(c->d_image + staging),
                                    (uint32_t*)c->d_image, c->width, c->height, c->stream));
    PT_HIP(hipEventRecord(c->ev1, c->stream));
    PT_HIP(hipMemcpyAsync(out, c->d_image, P * (format == PT_IMAGE_RGBA8 ? 4 : 3), hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    PT_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->stats.kernel_ms[PT_K_IMAGE] = ms;
    c->stats.kernel_launches[PT_K_IMAGE] = channel == PT_CHANNEL_SAMPLES ? 2 : 1;
    return PT_OK;
}

// pt_denoise on the Welford state {m, v, n}: the Buffer's, or the temporal result's (pt_denoise_temporal)
static int denoise_on(Ctx* c, const pt_denoise_params* params, const double* m, const double* v, const int32_t* n,
                      double* out_kernel_ms) {
    const int32_t iterations = params ? params->iterations : 5;
    const double sigma = params ? params->sigma_colour : 4.0;
    if (iterations < 1 || iterations > 8) return fail(PT_ERR_INVALID_ARG, "denoise: iterations must be 1..8");
    if (params && params->reserved != 0) return fail(PT_ERR_INVALID_ARG, "denoise: reserved must be 0");
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(PT_ERR_INVALID_ARG, "denoise: sigma_colour must be finite and > 0");
    PT_HIP(hipSetDevice(c->device));
    if (!c->d_denoise && hipMalloc(&c->d_denoise, pt::denoise_workspace_bytes(c->width, c->height)) != hipSuccess) {
        c->d_denoise = nullptr;
        (void)hipGetLastError();
        return fail(PT_ERR_OUT_OF_MEMORY, "denoise workspace allocation");
    }
    int pair = -1;
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    PT_HIP(pt::launch_denoise(m, v, n, c->d_denoise, c->width, c->height, iterations, sigma, &pair, c->stream));
    PT_HIP(hipEventRecord(c->ev1, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    c->denoise_pair = pair;
    return kernel_ms(c, out_kernel_ms);
}

int pt_denoise(void* ctx, const pt_denoise_params* params, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    return denoise_on(c, params, c->d_m, c->d_v, c->d_n, out_kernel_ms);
}

int pt_read_denoised(void* ctx, int32_t format, void* out) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !out) return fail(PT_ERR_INVALID_ARG, "NULL argument");
    if (format < PT_DENOISED_RGB8 || format > PT_DENOISED_VARIANCE_F64)
        return fail(PT_ERR_INVALID_ARG, "format is not a pt_denoised_format");
    if (c->denoise_pair < 0) return fail(PT_ERR_INVALID_ARG, "pt_read_denoised before any pt_denoise on this context");
    PT_HIP(hipSetDevice(c->device));
    const size_t P = (size_t)c->width * (size_t)c->height;
    const double* colour = (const double*)c->d_denoise + (size_t)c->denoise_pair * 6 * P;
    if (format == PT_DENOISED_COLOUR_F64 || format == PT_DENOISED_VARIANCE_F64) {
        const double* src = format == PT_DENOISED_COLOUR_F64 ? colour : colour + 3 * P;
        PT_HIP(hipMemcpyAsync(out, src, 3 * P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PT_HIP(hipStreamSynchronize(c->stream));
        return PT_OK;
    }
    // the Color channel's encoding (image_component<kChColor>, image_byte) of the denoised colour
    const size_t staging = pt::image_staging_bytes(c->width, c->height);
    if (!c->d_image && hipMalloc(&c->d_image, staging + 16) != hipSuccess) {
        c->d_image = nullptr;
        (void)hipGetLastError();
        return fail(PT_ERR_OUT_OF_MEMORY, "image staging allocation");
    }
    const int image_format = format == PT_DENOISED_RGBA8 ? PT_IMAGE_RGBA8 : PT_IMAGE_RGB8;
    PT_HIP(pt::launch_image_resolve(PT_CHANNEL_COLOR, image_format, colour, nullptr, nullptr, (int32_t*)(c->d_image + staging),
                                    (uint32_t*)c->d_image, c->width, c->height, c->stream));
    PT_HIP(hipMemcpyAsync(out, c->d_image, P * (image_format == PT_IMAGE_RGBA8 ? 4 : 3), hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}

// ------------------------------------------------------------------ first-hit features, guided denoise
// pt_denoise_guided's default guide sigmas (DESIGN.md §4b has the table they were chosen from)
constexpr double PT_DENOISE_GUIDED_SIGMA_NORMAL = 0.3, PT_DENOISE_GUIDED_SIGMA_ALBEDO = 0.3, PT_DENOISE_GUIDED_SIGMA_DEPTH = 0.1;
static int features_storage(Ctx* c) {
    if (!c->d_features && hipMalloc(&c->d_features, pt::features_bytes(c->width, c->height)) != hipSuccess) {
        c->d_features = nullptr;
        (void)hipGetLastError();
        return fail(PT_ERR_OUT_OF_MEMORY, "features allocation");
    }
    return PT_OK;
}

int pt_render_features(void* ctx, const pt_camera* camera, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !camera) return fail(PT_ERR_INVALID_ARG, "NULL argument");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    PT_HIP(hipSetDevice(c->device));
    const int rc = features_storage(c);
    if (rc != PT_OK) return rc;
    pt::DevCamera cam;
    std::memcpy(cam.p, camera->p, sizeof cam.p); std::memcpy(cam.u, camera->u, sizeof cam.u);
    std::memcpy(cam.v, camera->v, sizeof cam.v); std::memcpy(cam.w, camera->w, sizeof cam.w);
    cam.m = camera->m; cam.focal_distance = camera->focal_distance;
    cam.aperture_radius = 0.0;   // the lens is ignored: one deterministic ray through the pixel
    pt::DevScene S = c->S;
    S.march = nullptr;
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    PT_HIP(pt::launch_features(S, cam, c->d_features, c->width, c->height, c->stream));
    PT_HIP(hipEventRecord(c->ev1, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    c->have_features = true;
    return kernel_ms(c, out_kernel_ms);
}

int pt_read_features(void* ctx, int32_t feature, void* out) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !out) return fail(PT_ERR_INVALID_ARG, "NULL argument");
    if (feature < PT_FEATURE_ALBEDO_F64 || feature > PT_FEATURE_MATERIAL_I32)
        return fail(PT_ERR_INVALID_ARG, "feature is not a pt_feature");
    if (!c->have_features)
        return fail(PT_ERR_INVALID_ARG, "pt_read_features before any pt_render_features or pt_write_features on this context");
    PT_HIP(hipSetDevice(c->device));
    size_t bytes = 0;
    const void* src = pt::features_part(c->d_features, c->width, c->height, feature, &bytes);
    PT_HIP(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_write_features(void* ctx, const double* albedo, const float* normal, const double* depth, const int32_t* kind) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !albedo || !normal || !depth || !kind) return fail(PT_ERR_INVALID_ARG, "NULL argument");
    PT_HIP(hipSetDevice(c->device));
    const int rc = features_storage(c);
    if (rc != PT_OK) return rc;
    const void* src[4] = {albedo, normal, depth, kind};
    for (int part = 0; part < 4; part++) {
        size_t bytes = 0;
        void* dst = pt::features_part(c->d_features, c->width, c->height, part, &bytes);
        PT_HIP(hipMemcpyAsync(dst, src[part], bytes, hipMemcpyHostToDevice, c->stream));
    }
    size_t bytes = 0;
    void* mat = pt::features_part(c->d_features, c->width, c->height, PT_FEATURE_MATERIAL_I32, &bytes);
    PT_HIP(hipMemsetAsync(mat, 0xFF, bytes, c->stream));   // every material id -1
    PT_HIP(pt::launch_features_pack(c->d_features, c->width, c->height, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    c->have_features = true;
    return PT_OK;
}

// pt_denoise_guided on the Welford state {m, v, n}, as denoise_on
static int denoise_guided_on(Ctx* c, const pt_denoise_guided_params* params, const double* m, const double* v, const int32_t* n,
                             double* out_kernel_ms) {
    const int32_t iterations = params ? params->iterations : 5;
    const double sigma = params ? params->sigma_colour : 4.0;
    const double guide[3] = {params ? params->sigma_albedo : PT_DENOISE_GUIDED_SIGMA_ALBEDO,
                             params ? params->sigma_normal : PT_DENOISE_GUIDED_SIGMA_NORMAL,
                             params ? params->sigma_depth : PT_DENOISE_GUIDED_SIGMA_DEPTH};
    if (iterations < 1 || iterations > 8) return fail(PT_ERR_INVALID_ARG, "denoise_guided: iterations must be 1..8");
    if (params && params->reserved != 0) return fail(PT_ERR_INVALID_ARG, "denoise_guided: reserved must be 0");
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(PT_ERR_INVALID_ARG, "denoise_guided: sigma_colour must be finite and > 0");
    for (double g : guide)
        if (!(g >= 0.0) || !std::isfinite(g))
            return fail(PT_ERR_INVALID_ARG, "denoise_guided: sigma_albedo, sigma_normal and sigma_depth must be finite and >= 0");
    if (!c->have_features)
        return fail(PT_ERR_INVALID_ARG, "pt_denoise_guided before any pt_render_features or pt_write_features on this context");
    PT_HIP(hipSetDevice(c->device));
    if (!c->d_denoise && hipMalloc(&c->d_denoise, pt::denoise_workspace_bytes(c->width, c->height)) != hipSuccess) {
        c->d_denoise = nullptr;
        (void)hipGetLastError();
        return fail(PT_ERR_OUT_OF_MEMORY, "denoise workspace allocation");
    }
    int pair = -1;
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    PT_HIP(pt::launch_denoise_guided(m, v, n, c->d_denoise, pt::features_guide(c->d_features, c->width, c->height),
                                     c->width, c->height, iterations, sigma, guide[0], guide[1], guide[2], &pair, c->stream));
    PT_HIP(hipEventRecord(c->ev1, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    c->denoise_pair = pair;
    return kernel_ms(c, out_kernel_ms);
}

int pt_denoise_guided(void* ctx, const pt_denoise_guided_params* params, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    return denoise_guided_on(c, params, c->d_m, c->d_v, c->d_n, out_kernel_ms);
}

static int tile_workspace(Ctx* c);

// Host copies of a tile list's packed {M, V, N} (see k_tiles_pack for the order).
static int tiles_io(void* ctx, const int32_t* tiles, int32_t num_tiles, double* m, double* v, int32_t* n, bool write) {
    Ctx* c = (Ctx*)ctx;
    if (!c || (num_tiles > 0 && (!tiles || !m || !v || !n))) return fail(PT_ERR_INVALID_ARG, "NULL argument");
    if (num_tiles < 0) return fail(PT_ERR_INVALID_ARG, "num_tiles < 0");
    const int32_t all = ((c->width + 31) / 32) * ((c->height + 31) / 32);
    if (num_tiles > all) return fail(PT_ERR_INVALID_ARG, "more tiles than the image has");
    for (int32_t i = 0; i < num_tiles; i++)
        if (tiles[i] < 0 || tiles[i] >= all) return fail(PT_ERR_INVALID_ARG, "tile id out of range");
    if (num_tiles == 0) return PT_OK;
    PT_HIP(hipSetDevice(c->device));
    int rc = tile_workspace(c);
    if (rc) return rc;
    const size_t s = (size_t)num_tiles * 1024u;
    PT_HIP(hipMemcpyAsync(c->g_ids, tiles, (size_t)num_tiles * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (write) {
        PT_HIP(hipMemcpyAsync(c->g_m, m, s * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PT_HIP(hipMemcpyAsync(c->g_v, v, s * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PT_HIP(hipMemcpyAsync(c->g_n, n, s * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        c->gathered = true;   // foreign tiles written (a host-transport gather): cleared before the next subset pass
    }
    pt::DevBuffer B{c->d_m, c->d_v, c->d_n, c->d_counters};
    hipLaunchKernelGGL(pt::k_tiles_pack, dim3(2048), dim3(256), 0, c->stream, B, c->width, c->height,
                       (c->width + 31) / 32, c->g_ids, (uint32_t)num_tiles, c->g_m, c->g_v, c->g_n, write ? 1 : 0);
    PT_HIP(hipGetLastError());
    if (!write) {
        PT_HIP(hipMemcpyAsync(m, c->g_m, s * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PT_HIP(hipMemcpyAsync(v, c->g_v, s * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PT_HIP(hipMemcpyAsync(n, c->g_n, s * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}
int pt_read_tiles(void* ctx, const int32_t* tiles, int32_t num_tiles, double* out_m, double* out_v, int32_t* out_n) {
    return tiles_io(ctx, tiles, num_tiles, out_m, out_v, out_n, false);
}
int pt_write_tiles(void* ctx, const int32_t* tiles, int32_t num_tiles, const double* m, const double* v,
                   const int32_t* n) {
    return tiles_io(ctx, tiles, num_tiles, const_cast<double*>(m), const_cast<double*>(v), const_cast<int32_t*>(n), true);
}

// pt_intersect / pt_occluded: the rays to the device, one launch of k_intersect, the answers back.
static int ray_queries(void* ctx, int64_t n, const float* origins, const float* dirs, const double* t_light,
                       int32_t flags, double* out_t, int32_t* out_i) {
    Ctx* c = (Ctx*)ctx;
    if (!c || (n > 0 && (!origins || !dirs || !out_i || (!t_light && !out_t)))) return fail(PT_ERR_INVALID_ARG, "NULL argument");
    if (n < 0 || n > (int64_t)1 << 30) return fail(PT_ERR_INVALID_ARG, "n out of range [0, 2^30]");
    if (flags & ~(PT_MARCH_LANE | PT_MARCH_WAVE) || (flags & PT_MARCH_LANE && flags & PT_MARCH_WAVE))
        return fail(PT_ERR_INVALID_ARG, "flags: PT_MARCH_LANE or PT_MARCH_WAVE, not both");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return PT_OK;
    PT_HIP(hipSetDevice(c->device));
    const size_t N = (size_t)n;
    const size_t bytes = N * (6 * sizeof(float) + sizeof(double) + sizeof(double) + sizeof(int32_t));
    unsigned char* d = nullptr;
    hipError_t e = hipMalloc(&d, bytes);
    if (e != hipSuccess) return fail(PT_ERR_OUT_OF_MEMORY, std::string("hipMalloc ray queries: ") + hipGetErrorString(e));
    float* d_o = (float*)d;
    float* d_d = d_o + 3 * N;
    double* d_tl = (double*)(d_d + 3 * N);   // 8-B aligned: 24·N bytes precede it
    double* d_t = d_tl + N;
    int32_t* d_i = (int32_t*)(d_t + N);
    pt::DevScene S = c->S;
    if (flags & PT_MARCH_LANE) S.coop_min_lanes = 65;   // fewer than 65 active lanes: always
    if (flags & PT_MARCH_WAVE) S.coop_min_lanes = 1;    // every wave with a pending Volume marches it together
    int rc = PT_OK;
    auto step = [&](hipError_t err, const char* what) {
        if (rc == PT_OK && err != hipSuccess) rc = fail(PT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(err));
    };
    step(hipMemcpyAsync(d_o, origins, 3 * N * sizeof(float), hipMemcpyHostToDevice, c->stream), "origins");
    step(hipMemcpyAsync(d_d, dirs, 3 * N * sizeof(float), hipMemcpyHostToDevice, c->stream), "dirs");
    if (t_light) step(hipMemcpyAsync(d_tl, t_light, N * sizeof(double), hipMemcpyHostToDevice, c->stream), "t_light");
    if (rc == PT_OK) step(pt::launch_intersect(S, (uint32_t)N, d_o, d_d, t_light ? d_tl : nullptr, d_t, d_i, c->stream), "k_intersect");
    if (rc == PT_OK && out_t && !t_light) step(hipMemcpyAsync(out_t, d_t, N * sizeof(double), hipMemcpyDeviceToHost, c->stream), "out_t");
    if (rc == PT_OK) step(hipMemcpyAsync(out_i, d_i, N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream), "out");
    step(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    (void)hipFree(d);
    return rc;
}
int pt_intersect(void* ctx, int64_t n, const float* origins, const float* dirs, int32_t flags, double* out_t,
                 int32_t* out_kind) {
    if (!out_t) return fail(PT_ERR_INVALID_ARG, "out_t is NULL");
    return ray_queries(ctx, n, origins, dirs, nullptr, flags, out_t, out_kind);
}
int pt_occluded(void* ctx, int64_t n, const float* origins, const float* dirs, const double* t_max, int32_t flags,
                int32_t* out_blocked) {
    if (n > 0 && !t_max) return fail(PT_ERR_INVALID_ARG, "t_max is NULL");
    return ray_queries(ctx, n, origins, dirs, t_max, flags, nullptr, out_blocked);
}

}  // extern "C"

// ---- moving geometry: what the entry points of DESIGN.md §4c-§4g share
namespace {
int upload_lights(Ctx* c) {
    const std::vector<pt::DevLight>& L = c->dyn.h_lights;
    PT_HIP(hipMemcpyAsync(const_cast<pt::DevLight*>(c->S.lights), L.data(), L.size() * sizeof(pt::DevLight), hipMemcpyHostToDevice, c->stream));
    return PT_OK;
}

// Three arrays of [num_triangles][3] floats, or six when src[3] is set, to the device
void stage_arrays(Uploader& up, float* const dst[6], const float* const src[6], int32_t num_triangles) {
    for (int k = 0; k < (src[3] ? 6 : 3); k++) up.copy(dst[k], src[k], (size_t)num_triangles * 3 * sizeof(float));
}

// A read-back the caller may not want (dst NULL) or that may be empty
hipError_t read_back(Ctx* c, void* dst, const void* src, size_t bytes) {
    if (!dst || !bytes) return hipSuccess;
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
}

// The argument checks of the mesh entry points; `who` starts the message
int check_arrays(const std::string& who, const float* const a[6]) {
    if (!a[0] || !a[1] || !a[2]) return fail(PT_ERR_INVALID_ARG, who + ": v1, v2 and v3 are required");
    if ((a[3] != nullptr) != (a[4] != nullptr) || (a[3] != nullptr) != (a[5] != nullptr))
        return fail(PT_ERR_INVALID_ARG, who + ": n1/n2/n3 must be all set or all NULL");
    return PT_OK;
}
int check_normals_mode(const std::string& who, int32_t mode) {
    if (mode == 0 || mode == PT_NORMALS_FACE || mode == PT_NORMALS_SMOOTH) return PT_OK;
    return fail(PT_ERR_INVALID_ARG, who + ": normals_mode " + std::to_string(mode) + " is not 0 or a pt_normals_mode");
}
int check_mesh_update(const std::string& who, const pt_mesh_update* u) {
    if (u->reserved[0] != 0 || u->reserved[1] != 0) return fail(PT_ERR_INVALID_ARG, who + ": reserved must be 0");
    if (const int rc = check_normals_mode(who, u->normals_mode)) return rc;
    if (u->normals_mode != 0 && (u->n1 || u->n2 || u->n3))
        return fail(PT_ERR_INVALID_ARG, who + ": n1/n2/n3 are given and normals_mode derives them");
    const float* const a[6] = {u->v1, u->v2, u->v3, u->n1, u->n2, u->n3};
    return check_arrays(who, a);
}

// ---- the shape refit's device side (pt_update_shapes, and pt_update_meshes on instanced meshes ends in it)
int ensure_shapes_ws(Ctx* c) {
    const pt::ShapeRefitTables& T = c->dyn.shape_refit;
    return ensure_workspace(c, c->dyn.shapes_ws, "shape refit", [&](void* base) { return pt::shapes_layout(T, base); },
                            [&](const pt::ShapesDev& D, Uploader& up) {
                                up(D.level_nodes, T.level_nodes);
                                up(D.xf_kind, T.xf_kind);
                                up(D.xf_index, T.xf_index);
                                up(D.xf_inner_box, T.xf_inner_box);
                                up(D.rec_box, T.rec_box);   // top-level SDF and Volume records keep these
                            });
}
// The current parameters (ShapeRefitTables) into their staged copies, on the context's stream
int stage_shape_params(Ctx* c) {
    const pt::ShapeRefitTables& T = c->dyn.shape_refit;
    const pt::ShapesDev& D = c->dyn.shapes_ws.at;
    Uploader up{c->stream};
    up(D.sphere_center, T.sphere_center);
    up(D.sphere_radius, T.sphere_radius);
    up(D.cube_min, T.cube_min);
    up(D.cube_max, T.cube_max);
    up(D.xf_matrix, T.xf_matrix);
    up(D.xf_inverse, T.xf_inverse);
    return check_hip(up.err, "staging the shape parameters");
}
// The shape refit from the staged parameters
int launch_shapes(Ctx* c) {
    const pt::ShapeRefitTables& T = c->dyn.shape_refit;
    const pt::ShapesDev& D = c->dyn.shapes_ws.at;
    const pt::ShapeParams P{T.num_spheres, T.num_cubes, T.num_transformed, D.sphere_center, D.sphere_radius,
                            D.cube_min, D.cube_max, D.xf_matrix, D.xf_inverse};
    PT_HIP(pt::launch_shape_refit(P, T.num_nodes, T.num_recs, T.num_heavy, (int64_t)T.level_off.size() - 1, T.level_off.data(),
                                  D.level_nodes, (uint32_t*)const_cast<float4*>(c->S.ana_nodes),
                                  (uint32_t*)const_cast<float4*>(c->S.ana_recs), (uint32_t*)const_cast<float4*>(c->S.ext_recs),
                                  const_cast<pt::DevXform*>(c->S.xforms), (uint32_t*)const_cast<float4*>(c->S.heavy), D.xf_kind,
                                  D.xf_index, D.xf_inner_box, D.xbox, D.rec_box, D.node_box, c->stream));
    return PT_OK;
}

// ---- pt_update_meshes' part for instanced meshes
// Both workspaces, before the first copy, then the parameters the shape refit at the end runs from
int blas_refit_prepare(Ctx* c) {
    if (const int rc = ensure_shapes_ws(c)) return rc;
    const pt::BlasRefitTables& T = c->dyn.blas_refit;
    pt::BlasBlocks B;
    if (!c->dyn.blas_ws.mem.ptr) pt::blas_blocks(T, pt::blas_bounds_span(), B);
    bool first = false;
    if (const int rc = ensure_workspace(c, c->dyn.blas_ws, "BLAS refit", [&](void* base) { return pt::blas_layout(T, B.blas.size(), base); },
                                        [&](const pt::BlasDev& D, Uploader& up) {
                                            up(D.desc, T.desc);
                                            up(D.src_of_pos, T.src_of_pos);
                                            up(D.level_nodes, T.level_nodes);
                                            up(D.level_blas, T.level_blas);
                                            up(D.block_blas, B.blas);
                                            up(D.block_first, B.first);
                                            up(D.blas_block_off, B.off);
                                            up(D.xf_blas, T.xf_blas);
                                        },
                                        &first))
        return rc;   // (a failed upload released the workspace: hipFree waits for the copies issued from B)
    if (first) {     // B goes out of scope
        const int rc = check_hip(hipStreamSynchronize(c->stream), "BLAS refit workspace tables");
        if (rc != PT_OK) { c->dyn.blas_ws.release(); return rc; }
    }
    return stage_shape_params(c);
}
// The kernels on the context's stream, after the arrays were staged in `in` (in[3..5] NULL: normals kept)
int blas_refit_launch(Ctx* c, int32_t num_triangles, const float* const in[6]) {
    const pt::BlasRefitTables& T = c->dyn.blas_refit;
    const pt::BlasDev& D = c->dyn.blas_ws.at;
    PT_HIP(pt::launch_blas_refit((int64_t)T.num_blas(), T.num_tris, T.num_nodes, num_triangles, (int64_t)T.xf_blas.size(),
                                 (int64_t)D.num_blocks, (int64_t)T.level_off.size() - 1, T.level_off.data(), D.level_nodes,
                                 D.level_blas, D.desc, D.src_of_pos, D.block_blas, D.block_first, D.blas_block_off, D.xf_blas,
                                 (uint32_t*)const_cast<float4*>(c->S.blas_nodes), (uint32_t*)const_cast<float4*>(c->S.blas_recs),
                                 (uint32_t*)const_cast<float4*>(c->S.blas_shade), in[0], in[1], in[2], in[3], in[4], in[5],
                                 D.tri_box, D.node_box, D.block_part, D.blas_box, c->dyn.shapes_ws.at.xf_inner_box, c->stream));
    c->dyn.blas_boxes_on_device = true;
    return launch_shapes(c);
}
// The meshes' boxes back into the host tables and the lights; synchronises the context's stream
int blas_refit_finish(Ctx* c) {
    const pt::BlasRefitTables& T = c->dyn.blas_refit;
    pt::ShapeRefitTables& ST = c->dyn.shape_refit;
    std::vector<float> boxes(T.num_blas() * 6);
    PT_HIP(hipMemcpyAsync(boxes.data(), c->dyn.blas_ws.at.blas_box, boxes.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));   // the lights below need the boxes
    for (size_t t = 0; t < T.xf_blas.size() && 6 * t + 6 <= ST.xf_inner_box.size(); t++) {
        const int64_t b = T.xf_blas[t];
        if (b < 0 || (size_t)b >= T.num_blas()) continue;
        std::memcpy(&ST.xf_inner_box[6 * t], &boxes[6 * (size_t)b], 6 * sizeof(float));
    }
    // lights that are transformed shapes over a mesh follow its box
    if (pt::shape_refit_lights(ST, c->dyn.h_lights)) return upload_lights(c);
    return PT_OK;
}

// ---- pt_rebuild_blas' part for instanced meshes
// PT_BLAS_TAIL, read at each call (tests set it): 0 switches the LDS tail off, else the largest 4 * 4^k in [64, the
// kernel's] that the value holds
int64_t blas_tail_knob() {
    const int64_t most = pt::blas_tail_max();
    const char* e = std::getenv("PT_BLAS_TAIL");
    if (!e || !*e) return most;
    const int64_t v = (int64_t)std::atoll(e);
    if (v <= 0) return 0;
    int64_t t = 64;
    while (t * 4 <= v && t * 4 <= most) t *= 4;
    return t;
}
// The plan of every BLAS and the fallback decision, then the workspace: before anything is staged.  A BLAS whose
// balanced tree needs more nodes than the upload gave it keeps its topology (h == 0 in its item).
int blas_rebuild_prepare(Ctx* c) {
    SceneDyn& Y = c->dyn;
    const pt::BlasRefitTables& T = Y.blas_refit;
    const size_t nb = T.num_blas();
    std::vector<int32_t> items;
    size_t refused = 0;
    if (!pt::blas_rebuild_items(T, Y.blas_node_cap, items, &refused))
        return fail(PT_ERR_UNSUPPORTED, "rebuild blas: " + std::to_string(T.desc[4 * refused + 3]) + " triangles need more than " +
                                            std::to_string(pt::kBlasRebuildMaxLevels) + " levels");
    RebuildDev sized{};   // pt_blas_rebuild.hip sizes and carves this one
    if (!Y.blas_rebuild_ws.mem.ptr) {
        PT_HIP(pt::blas_rebuild_workspace_bytes((int64_t)nb, T.num_tris, &sized.temp_bytes, &sized.bytes));
        Y.blas_pos.assign((size_t)T.num_tris, -1);
        for (size_t b = 0; b < nb; b++)
            for (int64_t q = 0; q < T.desc[4 * b + 3]; q++) {
                const int64_t p = (int64_t)T.desc[4 * b + 2] + q;
                if (p >= 0 && p < T.num_tris) Y.blas_pos[(size_t)p] = (int32_t)b;
            }
    }
    if (const int rc = ensure_workspace(c, Y.blas_rebuild_ws, "BLAS rebuild", [&](void*) { return sized; },
                                        [&](const RebuildDev& D, Uploader& up) {   // each position's BLAS
                                            up.err = pt::blas_rebuild_upload(Y.blas_rebuild_ws.mem.ptr, D.temp_bytes, (int64_t)nb,
                                                                             T.num_tris, Y.blas_pos.data(), c->stream);
                                        }))
        return rc;
    Y.blas_items = std::move(items);
    return PT_OK;
}
// The re-sort and the new topologies on the context's stream, before blas_refit_launch, and what follows from the new
// node counts: the host tables (desc, the level lists) and their device copies, the DevBlas rows
int blas_rebuild_launch(Ctx* c, const float* const in[6]) {
    SceneDyn& Y = c->dyn;
    pt::BlasRefitTables& T = Y.blas_refit;
    const pt::BlasDev& D = Y.blas_ws.at;
    const size_t nb = T.num_blas();
    const int64_t tail_T = blas_tail_knob();
    pt::blas_tail_table(Y.blas_items.data(), (int64_t)nb, tail_T, Y.blas_tail);
    PT_HIP(pt::launch_blas_rebuild(Y.blas_rebuild_ws.mem.ptr, Y.blas_rebuild_ws.at.temp_bytes, (int64_t)nb, T.num_tris, T.num_nodes,
                                   Y.blas_items.data(), Y.blas_tail.data(), (int64_t)Y.blas_tail.size() / 4, tail_T,
                                   (uint32_t*)const_cast<float4*>(c->S.blas_nodes), (uint32_t*)const_cast<float4*>(c->S.blas_shade),
                                   (uint32_t*)const_cast<float4*>(c->S.blas_uv), D.src_of_pos, in[0], in[1], in[2], c->stream));
    pt::blas_rebuild_tables(T, Y.blas_items);
    for (size_t b = 0; b < nb && b < Y.h_blas.size(); b++) Y.h_blas[b].num_nodes = T.desc[4 * b + 1];
    Uploader up{c->stream};
    up(D.desc, T.desc);
    up(D.level_nodes, T.level_nodes);   // no longer than the upload's lists: a rebuilt BLAS has no more nodes than it had
    up(D.level_blas, T.level_blas);
    up(const_cast<pt::DevBlas*>(c->S.blas), Y.h_blas);
    return check_hip(up.err, "the rebuilt BLAS tables");
}

// ---- moving triangles: the path every triangle update takes
int ensure_refit_ws(Ctx* c) {
    const pt::RefitTables& T = c->dyn.refit;
    return ensure_workspace(c, c->dyn.refit_ws, "refit", [&](void* base) { return pt::refit_layout(T, base); },
                            [&](const pt::RefitDev& D, Uploader& up) {
                                if (T.src_of_pos.empty()) return;
                                up(D.src_of_pos, T.src_of_pos);
                                up(D.level_nodes, T.level_nodes);
                            });
}

enum class Normals { Kept, Given, Face, Smooth };   // the device's stay; staged in in[3..5]; derived there from the vertices
Normals normals_of(int32_t mode, bool given) {
    return mode == PT_NORMALS_FACE ? Normals::Face : mode == PT_NORMALS_SMOOTH ? Normals::Smooth : given ? Normals::Given : Normals::Kept;
}
// pt_rebuild_meshes' part of an update: the new topology, and the line its chunks start at (the upload's, or later
// when the balanced tree has more nodes than the uploaded one had: nodes and chunks share one run of lines)
struct RebuildRun {
    pt::RebuildPlan R;
    uint32_t chunk_line0;
};
// One update: update_prepare checks it and makes its workspaces, the caller stages its arrays in the refit
// workspace's `in` after recording Ctx::ev0, update_run runs it
struct UpdateCall {
    int32_t num_triangles;
    Normals normals;
    const float* light_verts[3];   // the vertices of the lights that are loose emissive triangles: the caller's v1, v2, v3
                                   // (pt_scene_desc order), or NULL: the rest vertices pt_set_rest_pose kept
    const RebuildRun* rebuild;     // pt_rebuild_meshes: re-sorted before the refit (NULL: the topology stays)
    bool rebuild_blas = false;     // pt_rebuild_blas: every BLAS re-sorted before its refit (blas_rebuild_prepare planned it)
};
// Whether the scene's instanced meshes take part in an update (update_prepare refused it for an entry point that
// does not refit them)
bool refits_blas(const Ctx* c, const UpdateCall& U) { return c->dyn.has_blas && U.num_triangles > 0; }

// The checks against the scene (meshes: the entry point refits instanced meshes too, it does not refuse them), then
// every workspace, before the first copy (a failed allocation leaves the scene untouched).  *launch is false when
// the scene holds no triangle in any BVH: PT_OK, nothing to run.
int update_prepare(Ctx* c, const UpdateCall& U, bool meshes, double* out_kernel_ms, bool* launch) {
    *launch = false;
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    SceneDyn& Y = c->dyn;
    const pt::RefitTables& T = Y.refit;
    if (U.num_triangles != T.num_triangles)
        return fail(PT_ERR_INVALID_ARG, "update: num_triangles is " + std::to_string(U.num_triangles) + ", the uploaded scene has " +
                                            std::to_string(T.num_triangles));
    if (Y.has_blas && !meshes)
        return fail(PT_ERR_UNSUPPORTED, "update: the scene holds an instanced mesh (a transformed shape over PT_SHAPE_MESH); "
                                        "its BLAS is not refitted");
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    const bool blas = refits_blas(c, U);
    if (T.num_chunks == 0 && !blas) return PT_OK;   // no triangle in a BVH (num_triangles == 0, or none of them in Scene.Shapes)
    PT_HIP(hipSetDevice(c->device));
    const bool smooth = U.normals == Normals::Smooth;
    if (smooth && (int64_t)U.num_triangles * 3 > (int64_t)INT32_MAX)
        return fail(PT_ERR_UNSUPPORTED, "update: PT_NORMALS_SMOOTH numbers corners in 31 bits");
    PT_HIP(hipStreamSynchronize(c->side));   // after every pass issued before, the side stream's work included
    if (smooth) {
        size_t temp = 0;
        if (!Y.normals_ws.mem.ptr) PT_HIP(pt::normals_sort_temp_bytes((int64_t)U.num_triangles * 3, T.num_groups, &temp));
        if (const int rc = ensure_workspace(c, Y.normals_ws, "normals", [&](void* base) { return pt::normals_layout(T, temp, base); },
                                            [&](const pt::NormalsDev& N, Uploader& up) { up(N.group, T.tri_group); }))
            return rc;
    }
    if (const int rc = ensure_refit_ws(c)) return rc;
    if (blas) if (const int rc = blas_refit_prepare(c)) return rc;
    *launch = true;
    return PT_OK;
}

// From the arrays staged in the refit workspace on the context's stream after Ctx::ev0 was recorded there: the
// normals when they are derived, the re-sort of a rebuild, the refit of the world triangle BVH, the BLAS path, the
// root box, the lights, the timing.
int update_run(Ctx* c, const UpdateCall& U, double* out_kernel_ms) {
    SceneDyn& Y = c->dyn;
    pt::RefitTables& T = Y.refit;
    const pt::RefitDev& D = Y.refit_ws.at;
    uint32_t* nodes = (uint32_t*)const_cast<float4*>(c->S.tri_nodes);
    if (U.normals == Normals::Face || U.normals == Normals::Smooth) {
        const bool smooth = U.normals == Normals::Smooth;
        const pt::NormalsDev N = smooth ? Y.normals_ws.at : pt::NormalsDev{};
        PT_HIP(pt::launch_normals(smooth, U.num_triangles, D.in[0], D.in[1], D.in[2], D.in[3], D.in[4], D.in[5], N.group, T.num_groups,
                                  N.keys[0], N.keys[1], N.vals[0], N.vals[1], N.temp, N.temp_bytes, c->stream));
    }
    if (U.rebuild) {
        // the re-sort and the new topology before the refit, which then runs over the new tables: D reserved room for
        // them when it was laid out (pt_update_layout.h refit_layout)
        const pt::RebuildPlan& R = U.rebuild->R;
        if (U.rebuild->chunk_line0 != c->S.tri_chunk_line0) {   // more nodes than the upload had: the chunks start later
            c->S.tri_chunk_line0 = U.rebuild->chunk_line0;
            c->S.tri_chunks = c->S.lines + 8 * (size_t)U.rebuild->chunk_line0;
        }
        PT_HIP(pt::launch_rebuild(R, Y.rebuild_ws.mem.ptr, Y.rebuild_ws.at.temp_bytes, nodes, (uint32_t*)const_cast<float4*>(c->S.tri_chunks),
                                  (uint32_t*)const_cast<float4*>(c->S.tri_recs), D.src_of_pos, D.level_nodes, D.in[0], D.in[1],
                                  D.in[2], c->stream));
        T.num_nodes = R.num_nodes;
        T.num_chunks = R.num_chunks;
        T.level_nodes.resize((size_t)R.num_nodes);
        for (int64_t i = 0; i < R.num_nodes; i++) T.level_nodes[(size_t)i] = (uint32_t)i;
        T.level_off.assign(R.level_off, R.level_off + R.h + 1);
        c->S.tri_num_nodes = (int32_t)R.num_nodes;
        // what the compile derives from the node count follows: the routed split needs a tree of more than 64 nodes
        // (pt_scene_compile.cpp); the stack key's index bits were sized for the upload's counts, and the balanced
        // tree has no more chunks, and no more nodes than chunks (pt_stack_key.h)
        if (c->S.tri_num_nodes <= 64) c->S.route = 0;
    }
    const bool normals = U.normals != Normals::Kept;
    const float* const in[6] = {D.in[0], D.in[1], D.in[2], normals ? D.in[3] : nullptr, normals ? D.in[4] : nullptr,
                                normals ? D.in[5] : nullptr};
    PT_HIP(pt::launch_refit(T.num_chunks, (int64_t)T.level_off.size() - 1, T.level_off.data(), D.level_nodes, nodes,
                            (uint32_t*)const_cast<float4*>(c->S.tri_chunks), (uint32_t*)const_cast<float4*>(c->S.tri_recs),
                            D.src_of_pos, in[0], in[1], in[2], in[3], in[4], in[5], D.node_box, D.chunk_box, c->stream));
    if (U.rebuild_blas && refits_blas(c, U)) if (const int rc = blas_rebuild_launch(c, in)) return rc;
    if (refits_blas(c, U)) if (const int rc = blas_refit_launch(c, U.num_triangles, in)) return rc;
    PT_HIP(hipEventRecord(c->ev1, c->stream));
    // the root box follows (pt_wavefront.hip's refill kernels skip the triangle phase of a ray that misses it)
    uint32_t root[pt::kNode8Words];
    if (T.num_chunks > 0) PT_HIP(hipMemcpyAsync(root, nodes, sizeof root, hipMemcpyDeviceToHost, c->stream));
    if (U.rebuild) {
        PT_HIP(hipMemcpyAsync(T.src_of_pos.data(), D.src_of_pos, T.src_of_pos.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        Y.query_src_stale = true;   // pt_intersect_hits' copy follows at its next call
    }
    if (U.rebuild_blas && refits_blas(c, U)) {
        std::vector<int32_t>& src = Y.blas_refit.src_of_pos;
        PT_HIP(hipMemcpyAsync(src.data(), Y.blas_ws.at.src_of_pos, src.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        Y.query_blas_src_stale = true;
    }
    // the loose triangles' vertices as the device holds them from here on (a later pt_update_materials may make any
    // of them a light), then the lights that are loose emissive triangles: their sphere from the new vertices
    for (const pt::LookSlot& slot : Y.look.slots) {
        if (slot.vert < 0) continue;
        float* m = &Y.look.tri_verts[(size_t)slot.vert];
        const float* const* v = U.light_verts;
        const size_t j = (size_t)slot.index;
        if (v[0]) for (int k = 0; k < 3; k++) std::memcpy(m + 3 * k, v[k] + 3 * j, 3 * sizeof(float));
        else if (Y.rest_tri_verts.size() == Y.look.tri_verts.size()) std::memcpy(m, &Y.rest_tri_verts[(size_t)slot.vert], 9 * sizeof(float));
    }
    bool lights_moved = false;
    for (size_t i = 0; i < Y.h_lights.size() && i < T.light_tri.size(); i++) {
        const int64_t j = T.light_tri[i];
        if (j < 0) continue;
        const float* m = &Y.look.tri_verts[(size_t)Y.look.slots[(size_t)Y.look.light_slot[i]].vert];
        pt::tri_light_sphere(m, m + 3, m + 6, Y.h_lights[i]);
        lights_moved = true;
    }
    if (lights_moved) if (const int rc = upload_lights(c)) return rc;
    if (refits_blas(c, U)) if (const int rc = blas_refit_finish(c)) return rc;
    PT_HIP(hipStreamSynchronize(c->stream));
    if (T.num_chunks > 0) pt::tri_root_box(root, c->S.tri_box);
    return kernel_ms(c, out_kernel_ms);
}

// An update from host arrays: src staged (NULL: the pose, skin or morph left staged is used and stays
// readable), then run
int update_stage_and_run(Ctx* c, const UpdateCall& U, const float* const src[6], double* out_kernel_ms) {
    if (src) {
        c->dyn.pose_staged = false;   // the staged arrays are this update's from here on
        Uploader up{c->stream};
        stage_arrays(up, c->dyn.refit_ws.at.in, src, U.num_triangles);
        if (const int rc = check_hip(up.err, "staging the triangle arrays")) return rc;
    }
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    return update_run(c, U, out_kernel_ms);
}
// pt_update_triangles, pt_update_triangles_normals and pt_update_meshes after their argument checks
int update_triangles(Ctx* c, int32_t num_triangles, const float* const src[6], int32_t mode, bool meshes, double* out_kernel_ms) {
    const UpdateCall U{num_triangles, normals_of(mode, src[3]), {src[0], src[1], src[2]}, nullptr};
    bool launch = false;
    if (const int rc = update_prepare(c, U, meshes, out_kernel_ms, &launch)) return rc;
    return launch ? update_stage_and_run(c, U, src, out_kernel_ms) : PT_OK;
}
}  // namespace

extern "C" {

int pt_update_triangles(void* ctx, int32_t num_triangles, const float* v1, const float* v2, const float* v3, const float* n1,
                        const float* n2, const float* n3, double* out_kernel_ms) {
    if (!ctx) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    const float* const src[6] = {v1, v2, v3, n1, n2, n3};
    if (const int rc = check_arrays("update", src)) return rc;
    return update_triangles((Ctx*)ctx, num_triangles, src, 0, false, out_kernel_ms);
}

int pt_update_triangles_normals(void* ctx, int32_t num_triangles, const float* v1, const float* v2, const float* v3, int32_t mode,
                                double* out_kernel_ms) {
    if (!ctx) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    const float* const src[6] = {v1, v2, v3, nullptr, nullptr, nullptr};
    if (const int rc = check_arrays("update", src)) return rc;
    if (mode != PT_NORMALS_FACE && mode != PT_NORMALS_SMOOTH)
        return fail(PT_ERR_INVALID_ARG, "update: mode " + std::to_string(mode) + " is not a pt_normals_mode");
    return update_triangles((Ctx*)ctx, num_triangles, src, mode, false, out_kernel_ms);
}

int pt_update_meshes(void* ctx, const pt_mesh_update* u, double* out_kernel_ms) {
    if (!ctx) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!u) return fail(PT_ERR_INVALID_ARG, "update meshes: u is NULL");
    if (const int rc = check_mesh_update("update meshes", u)) return rc;
    const float* const src[6] = {u->v1, u->v2, u->v3, u->n1, u->n2, u->n3};
    return update_triangles((Ctx*)ctx, u->num_triangles, src, u->normals_mode, true, out_kernel_ms);
}

int pt_read_tri_normals(void* ctx, float* n1, float* n2, float* n3) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!n1 || !n2 || !n3) return fail(PT_ERR_INVALID_ARG, "read normals: n1, n2 and n3 are required");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    const pt::RefitTables& T = c->dyn.refit;
    if (T.num_triangles <= 0) return PT_OK;
    const size_t arr = (size_t)T.num_triangles * 3 * sizeof(float);
    float* out[3] = {n1, n2, n3};
    if (T.src_of_pos.empty()) {   // no triangle of the scene is in the BVH: the device holds no normal
        for (float* o : out) std::memset(o, 0, arr);
        return PT_OK;
    }
    PT_HIP(hipSetDevice(c->device));
    if (const int rc = ensure_refit_ws(c)) return rc;
    const pt::RefitDev& D = c->dyn.refit_ws.at;
    // the staged normal arrays are free between updates: a triangle outside the BVH reads as zeros
    c->dyn.pose_staged = false;
    for (int k = 3; k < 6; k++) PT_HIP(hipMemsetAsync(D.in[k], 0, arr, c->stream));
    PT_HIP(pt::launch_normals_gather((int64_t)T.src_of_pos.size(), (const uint32_t*)c->S.tri_recs, D.src_of_pos, D.in[3], D.in[4],
                                     D.in[5], c->stream));
    for (int k = 0; k < 3; k++) PT_HIP(hipMemcpyAsync(out[k], D.in[3 + k], arr, hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_read_tri_bvh(void* ctx, int64_t counts[3], uint32_t* nodes, uint32_t* chunks, uint32_t* records, float out_box[6]) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    const pt::RefitTables& T = c->dyn.refit;
    if (counts) { counts[0] = T.num_nodes; counts[1] = T.num_chunks; counts[2] = (int64_t)T.src_of_pos.size(); }
    if (out_box) std::memcpy(out_box, c->S.tri_box, sizeof c->S.tri_box);
    PT_HIP(hipSetDevice(c->device));
    const size_t line = pt::kNode8Words * sizeof(uint32_t);
    PT_HIP(read_back(c, nodes, c->S.tri_nodes, (size_t)T.num_nodes * line));
    PT_HIP(read_back(c, chunks, c->S.tri_chunks, (size_t)T.num_chunks * line));
    PT_HIP(read_back(c, records, c->S.tri_recs, T.src_of_pos.size() * line));
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}

// ---- posing meshes by matrix on the device
int pt_set_rest_pose(void* ctx, int32_t num_triangles, const float* v1, const float* v2, const float* v3, const float* n1,
                     const float* n2, const float* n3) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!v1 || !v2 || !v3 || !n1 || !n2 || !n3) return fail(PT_ERR_INVALID_ARG, "rest pose: v1, v2, v3, n1, n2 and n3 are required");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    SceneDyn& Y = c->dyn;
    const pt::RefitTables& T = Y.refit;
    if (num_triangles != T.num_triangles)
        return fail(PT_ERR_INVALID_ARG, "rest pose: num_triangles is " + std::to_string(num_triangles) + ", the uploaded scene has " +
                                            std::to_string(T.num_triangles));
    PT_HIP(hipSetDevice(c->device));
    const float* const src[6] = {v1, v2, v3, n1, n2, n3};
    // the first rest pose goes in with the workspace, the triangles' groups behind it
    bool first = false;
    if (const int rc = ensure_workspace(c, Y.pose_ws, "pose", [&](void* base) { return pt::pose_layout(T, base); },
                                        [&](const pt::PoseDev& P, Uploader& up) {
                                            stage_arrays(up, P.rest, src, num_triangles);
                                            up(P.group, T.tri_group);
                                        },
                                        &first))
        return rc;
    if (!first) {
        Uploader up{c->stream};
        stage_arrays(up, Y.pose_ws.at.rest, src, num_triangles);
        if (const int rc = check_hip(up.err, "staging the rest pose")) return rc;
    }
    // the loose triangles (the lights among them) return to these at every pose
    Y.rest_tri_verts.assign(Y.look.tri_verts.size(), 0.f);
    for (const pt::LookSlot& slot : Y.look.slots) {
        if (slot.vert < 0 || slot.index < 0 || slot.index >= num_triangles) continue;
        for (int k = 0; k < 3; k++) std::memcpy(&Y.rest_tri_verts[(size_t)slot.vert + 3 * k], src[k] + 3 * (size_t)slot.index, 3 * sizeof(float));
    }
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_pose_meshes(void* ctx, const pt_mesh_pose* u, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!u) return fail(PT_ERR_INVALID_ARG, "pose meshes: u is NULL");
    if (u->reserved[0] != 0 || u->reserved[1] != 0) return fail(PT_ERR_INVALID_ARG, "pose meshes: reserved must be 0");
    if (const int rc = check_normals_mode("pose meshes", u->normals_mode)) return rc;
    if (!u->matrices) return fail(PT_ERR_INVALID_ARG, "pose meshes: matrices is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    const pt::RefitTables& T = c->dyn.refit;
    if (u->num_meshes != T.num_groups)
        return fail(PT_ERR_INVALID_ARG, "pose meshes: num_meshes is " + std::to_string(u->num_meshes) + ", the uploaded scene has " +
                                            std::to_string(T.num_groups));
    if (!c->dyn.pose_ws.mem.ptr) return fail(PT_ERR_INVALID_ARG, "pose meshes: no rest pose (pt_set_rest_pose)");
    // the posed normals are staged unless a mode derives them; the lights return to their rest vertices
    const UpdateCall U{T.num_triangles, normals_of(u->normals_mode, true), {nullptr, nullptr, nullptr}, nullptr};
    bool launch = false;
    if (const int rc = update_prepare(c, U, true, out_kernel_ms, &launch)) return rc;
    if (!launch) return PT_OK;
    const pt::PoseDev& P = c->dyn.pose_ws.at;
    const size_t nm = (size_t)T.num_groups;
    if (nm) {
        PT_HIP(hipMemcpyAsync(P.matrices, u->matrices, nm * 16 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (u->mesh_mask) PT_HIP(hipMemcpyAsync(P.mask, u->mesh_mask, nm * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    PT_HIP(pt::launch_pose(T.num_triangles, T.num_groups, P.group, u->mesh_mask ? P.mask : nullptr, P.matrices, U.normals == Normals::Given,
                           P.rest, c->dyn.refit_ws.at.in, c->stream));
    c->dyn.pose_staged = true;
    return update_run(c, U, out_kernel_ms);
}

int pt_read_pose(void* ctx, float* v1, float* v2, float* v3, float* n1, float* n2, float* n3) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    if (!c->dyn.pose_staged || !c->dyn.refit_ws.mem.ptr)
        return fail(PT_ERR_INVALID_ARG, "read pose: the staged arrays hold no pose or skin (none made since the upload, or a later "
                                        "pt_update_* or pt_read_tri_normals reused them)");
    PT_HIP(hipSetDevice(c->device));
    const size_t arr = (size_t)c->dyn.refit.num_triangles * 3 * sizeof(float);
    float* out[6] = {v1, v2, v3, n1, n2, n3};
    for (int k = 0; k < 6; k++) PT_HIP(read_back(c, out[k], c->dyn.refit_ws.at.in[k], arr));
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}

// ---- blend skinning on the device
static_assert(pt::kSkinInfluences == PT_SKIN_INFLUENCES, "pt_skin.h and the ABI agree on the influences per corner");

int pt_set_skin(void* ctx, const pt_skin_desc* d) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!d) return fail(PT_ERR_INVALID_ARG, "set skin: desc is NULL");
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return fail(PT_ERR_INVALID_ARG, "set skin: reserved must be 0");
    const int32_t* const bones[3] = {d->bone1, d->bone2, d->bone3};
    const float* const weights[3] = {d->weight1, d->weight2, d->weight3};
    for (int k = 0; k < 3; k++)
        if (!bones[k] || !weights[k])
            return fail(PT_ERR_INVALID_ARG, "set skin: bone1, bone2, bone3, weight1, weight2 and weight3 are required");
    if (d->num_bones < 1 || d->num_bones > PT_SKIN_MAX_BONES)
        return fail(PT_ERR_INVALID_ARG, "set skin: num_bones is " + std::to_string(d->num_bones) + ", outside [1, " +
                                            std::to_string(PT_SKIN_MAX_BONES) + "]");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    SceneDyn& Y = c->dyn;
    const int32_t n = Y.refit.num_triangles;
    if (d->num_triangles != n)
        return fail(PT_ERR_INVALID_ARG, "set skin: num_triangles is " + std::to_string(d->num_triangles) + ", the uploaded scene has " +
                                            std::to_string(n));
    // every index, whatever its weight, before the first copy: the kernel's gathers stay inside the matrix array
    const size_t row = (size_t)n * PT_SKIN_INFLUENCES;
    std::vector<uint16_t> packed[3];
    for (int k = 0; k < 3; k++) {
        packed[k].resize(row);
        for (size_t i = 0; i < row; i++) {
            const int32_t b = bones[k][i];
            if (b < 0 || b >= d->num_bones)
                return fail(PT_ERR_INVALID_ARG, "set skin: bone" + std::to_string(k + 1) + "[" + std::to_string(i / PT_SKIN_INFLUENCES) + "][" +
                                                    std::to_string(i % PT_SKIN_INFLUENCES) + "] is " + std::to_string(b) +
                                                    ", outside [0, " + std::to_string(d->num_bones) + ")");
            packed[k][i] = (uint16_t)b;
        }
    }
    PT_HIP(hipSetDevice(c->device));
    // a workspace with room for the matrices: the installed one, or a new one that replaces it once it is filled
    const auto upload = [&](const pt::SkinDev& S, Uploader& up) {
        for (int k = 0; k < 3; k++) {
            up(S.bone[k], packed[k]);
            up.copy(S.weight[k], weights[k], row * sizeof(float));
        }
    };
    if (Y.skin_ws.mem.ptr && d->num_bones <= Y.skin_ws.at.bone_cap) {
        Uploader up{c->stream};
        upload(Y.skin_ws.at, up);
        if (const int rc = check_hip(up.err, "staging the skin")) return rc;
    } else {
        Workspace<pt::SkinDev> fresh;
        if (const int rc = ensure_workspace(c, fresh, "skin", [&](void* base) { return pt::skin_layout(n, d->num_bones, base); }, upload))
            return rc;
        Y.skin_ws.release();
        Y.skin_ws = fresh;
    }
    PT_HIP(hipStreamSynchronize(c->stream));
    Y.skin_bones = d->num_bones;
    return PT_OK;
}

int pt_skin_meshes(void* ctx, const pt_mesh_skin* u, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!u) return fail(PT_ERR_INVALID_ARG, "skin meshes: u is NULL");
    if (u->reserved[0] != 0 || u->reserved[1] != 0) return fail(PT_ERR_INVALID_ARG, "skin meshes: reserved must be 0");
    if (const int rc = check_normals_mode("skin meshes", u->normals_mode)) return rc;
    if (!u->matrices) return fail(PT_ERR_INVALID_ARG, "skin meshes: matrices is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    SceneDyn& Y = c->dyn;
    const pt::RefitTables& T = Y.refit;
    if (!Y.skin_ws.mem.ptr || Y.skin_bones == 0) return fail(PT_ERR_INVALID_ARG, "skin meshes: no skin (pt_set_skin)");
    if (u->num_bones != Y.skin_bones)
        return fail(PT_ERR_INVALID_ARG, "skin meshes: num_bones is " + std::to_string(u->num_bones) + ", the installed skin has " +
                                            std::to_string(Y.skin_bones));
    if (!Y.pose_ws.mem.ptr) return fail(PT_ERR_INVALID_ARG, "skin meshes: no rest pose (pt_set_rest_pose)");
    // the skinned normals are staged unless a mode derives them; the lights return to their rest vertices
    const UpdateCall U{T.num_triangles, normals_of(u->normals_mode, true), {nullptr, nullptr, nullptr}, nullptr};
    bool launch = false;
    if (const int rc = update_prepare(c, U, true, out_kernel_ms, &launch)) return rc;
    if (!launch) return PT_OK;
    const pt::PoseDev& P = Y.pose_ws.at;
    const pt::SkinDev& S = Y.skin_ws.at;
    PT_HIP(hipMemcpyAsync(S.matrices, u->matrices, (size_t)u->num_bones * 16 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    PT_HIP(pt::launch_skin(T.num_triangles, u->num_bones, P.group, S.matrices, U.normals == Normals::Given, S.bone, S.weight, P.rest,
                           Y.refit_ws.at.in, c->stream));
    Y.pose_staged = true;
    return update_run(c, U, out_kernel_ms);
}

int pt_read_skin(void* ctx, int32_t* bone1, int32_t* bone2, int32_t* bone3, float* weight1, float* weight2, float* weight3) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    SceneDyn& Y = c->dyn;
    if (!Y.skin_ws.mem.ptr || Y.skin_bones == 0) return fail(PT_ERR_INVALID_ARG, "read skin: no skin (pt_set_skin)");
    PT_HIP(hipSetDevice(c->device));
    const size_t row = (size_t)Y.refit.num_triangles * PT_SKIN_INFLUENCES;
    int32_t* const bones[3] = {bone1, bone2, bone3};
    float* const weights[3] = {weight1, weight2, weight3};
    std::vector<uint16_t> packed[3];
    for (int k = 0; k < 3; k++) {
        if (bones[k]) {
            packed[k].resize(row);
            PT_HIP(read_back(c, packed[k].data(), Y.skin_ws.at.bone[k], row * sizeof(uint16_t)));
        }
        PT_HIP(read_back(c, weights[k], Y.skin_ws.at.weight[k], row * sizeof(float)));
    }
    PT_HIP(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; k++)
        if (bones[k]) for (size_t i = 0; i < row; i++) bones[k][i] = packed[k][i];
    return PT_OK;
}

// ---- morph targets on the device
static_assert(pt::kMorphMaxTargets == PT_MORPH_MAX_TARGETS, "pt_morph.h and the ABI agree on the number of targets");

int pt_set_morph(void* ctx, const pt_morph_desc* d) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!d) return fail(PT_ERR_INVALID_ARG, "set morph: desc is NULL");
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return fail(PT_ERR_INVALID_ARG, "set morph: reserved must be 0");
    if (!d->target_first || !d->corner || !d->dpos) return fail(PT_ERR_INVALID_ARG, "set morph: target_first, corner and dpos are required");
    if (d->num_targets < 1 || d->num_targets > PT_MORPH_MAX_TARGETS)
        return fail(PT_ERR_INVALID_ARG, "set morph: num_targets is " + std::to_string(d->num_targets) + ", outside [1, " +
                                            std::to_string(PT_MORPH_MAX_TARGETS) + "]");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    SceneDyn& Y = c->dyn;
    const int32_t n = Y.refit.num_triangles;
    if (d->num_triangles != n)
        return fail(PT_ERR_INVALID_ARG, "set morph: num_triangles is " + std::to_string(d->num_triangles) + ", the uploaded scene has " +
                                            std::to_string(n));
    // every delta before the first copy: the packer and the kernel index with what this accepts
    std::string why;
    if (!pt::morph_check(n, d->num_targets, d->target_first, d->corner, &why)) return fail(PT_ERR_INVALID_ARG, "set morph: " + why);
    pt::MorphPacked P;
    pt::morph_pack(n, d->num_targets, d->target_first, d->corner, d->dpos, d->dnrm, P);
    PT_HIP(hipSetDevice(c->device));
    // the planes' sizes follow the sparsity pattern: always a new workspace, which replaces the installed one once it is filled
    Workspace<pt::MorphDev> fresh;
    if (const int rc = ensure_workspace(c, fresh, "morph",
                                        [&](void* base) { return pt::morph_layout(P.slices, P.steps, P.has_dnrm, P.num_targets, base); },
                                        [&](const pt::MorphDev& M, Uploader& up) {
                                            up(M.len, P.len);
                                            up(M.first, P.first);
                                            up(M.target, P.target);
                                            up(M.dpos, P.dpos);
                                            if (M.dnrm) up(M.dnrm, P.dnrm);
                                        }))
        return rc;
    const hipError_t e = hipStreamSynchronize(c->stream);   // P's arrays live until here
    if (e != hipSuccess) {
        fresh.release();
        return check_hip(e, "staging the morph");
    }
    Y.morph_ws.release();
    Y.morph_ws = fresh;
    Y.morph_targets = P.num_targets;
    Y.morph_deltas = P.deltas;
    Y.morph_slices = P.slices;
    Y.morph_steps = P.steps;
    return PT_OK;
}

int pt_morph_meshes(void* ctx, const pt_mesh_morph* u, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!u) return fail(PT_ERR_INVALID_ARG, "morph meshes: u is NULL");
    if (u->reserved != 0) return fail(PT_ERR_INVALID_ARG, "morph meshes: reserved must be 0");
    if (const int rc = check_normals_mode("morph meshes", u->normals_mode)) return rc;
    if (!u->weights) return fail(PT_ERR_INVALID_ARG, "morph meshes: weights is NULL");
    const bool skin = u->skin_matrices != nullptr;
    if (!skin && u->num_bones != 0) return fail(PT_ERR_INVALID_ARG, "morph meshes: num_bones is not 0 and skin_matrices is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    SceneDyn& Y = c->dyn;
    const pt::RefitTables& T = Y.refit;
    if (!Y.morph_ws.mem.ptr || Y.morph_targets == 0) return fail(PT_ERR_INVALID_ARG, "morph meshes: no morph (pt_set_morph)");
    if (u->num_targets != Y.morph_targets)
        return fail(PT_ERR_INVALID_ARG, "morph meshes: num_targets is " + std::to_string(u->num_targets) + ", the installed morph has " +
                                            std::to_string(Y.morph_targets));
    if (skin) {
        if (!Y.skin_ws.mem.ptr || Y.skin_bones == 0) return fail(PT_ERR_INVALID_ARG, "morph meshes: skin_matrices given and no skin (pt_set_skin)");
        if (u->num_bones != Y.skin_bones)
            return fail(PT_ERR_INVALID_ARG, "morph meshes: num_bones is " + std::to_string(u->num_bones) + ", the installed skin has " +
                                                std::to_string(Y.skin_bones));
    }
    if (!Y.pose_ws.mem.ptr) return fail(PT_ERR_INVALID_ARG, "morph meshes: no rest pose (pt_set_rest_pose)");
    // the morphed (and skinned) normals are staged unless a mode derives them; the lights return to their rest vertices
    const UpdateCall U{T.num_triangles, normals_of(u->normals_mode, true), {nullptr, nullptr, nullptr}, nullptr};
    bool launch = false;
    if (const int rc = update_prepare(c, U, true, out_kernel_ms, &launch)) return rc;
    if (!launch) return PT_OK;
    if (skin)
        if (const int rc = ensure_workspace(c, Y.morph_tmp_ws, "morph intermediate",
                                            [&](void* base) { return pt::morph_tmp_layout(T.num_triangles, base); },
                                            [](const pt::MorphTmpDev&, Uploader&) {}))
            return rc;
    const pt::PoseDev& P = Y.pose_ws.at;
    const pt::MorphDev& M = Y.morph_ws.at;
    PT_HIP(hipMemcpyAsync(M.weights, u->weights, (size_t)u->num_targets * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (skin)
        PT_HIP(hipMemcpyAsync(Y.skin_ws.at.matrices, u->skin_matrices, (size_t)u->num_bones * 16 * sizeof(double), hipMemcpyHostToDevice,
                              c->stream));
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    // given normals: blended with dnrm, or copied when the morph has none; derived ones: not written, or carried to the skin
    const bool given = U.normals == Normals::Given;
    const int normals = given ? (M.dnrm ? 2 : 1) : skin ? 1 : 0;
    float* const* out = skin ? Y.morph_tmp_ws.at.out : Y.refit_ws.at.in;
    PT_HIP(pt::launch_morph(T.num_triangles, u->num_targets, P.group, M.weights, normals, M.len, M.first, M.target, M.dpos, M.dnrm,
                            P.rest, out, c->stream));
    if (skin) {
        const pt::SkinDev& S = Y.skin_ws.at;
        PT_HIP(pt::launch_skin(T.num_triangles, u->num_bones, P.group, S.matrices, given, S.bone, S.weight, Y.morph_tmp_ws.at.out,
                               Y.refit_ws.at.in, c->stream));
    }
    Y.pose_staged = true;
    return update_run(c, U, out_kernel_ms);
}

int pt_read_morph(void* ctx, int64_t counts[3], int64_t* target_first, int32_t* corner, float* dpos, float* dnrm) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    SceneDyn& Y = c->dyn;
    if (!Y.morph_ws.mem.ptr || Y.morph_targets == 0) return fail(PT_ERR_INVALID_ARG, "read morph: no morph (pt_set_morph)");
    if (counts) { counts[0] = Y.morph_targets; counts[1] = Y.morph_deltas; counts[2] = Y.morph_steps * pt::kMorphSlice; }
    if (!target_first && !corner && !dpos && !dnrm) return PT_OK;
    PT_HIP(hipSetDevice(c->device));
    const pt::MorphDev& M = Y.morph_ws.at;
    pt::MorphPacked P;
    P.n = Y.refit.num_triangles;
    P.slices = Y.morph_slices;
    P.steps = Y.morph_steps;
    P.deltas = Y.morph_deltas;
    P.num_targets = Y.morph_targets;
    P.has_dnrm = M.dnrm != nullptr;
    P.len.resize((size_t)P.slices);
    P.first.resize((size_t)P.slices);
    P.target.resize((size_t)P.padded());
    P.dpos.resize((size_t)P.padded() * 3);
    if (P.has_dnrm) P.dnrm.resize((size_t)P.padded() * 3);
    PT_HIP(read_back(c, P.len.data(), M.len, P.len.size() * sizeof(int32_t)));
    PT_HIP(read_back(c, P.first.data(), M.first, P.first.size() * sizeof(int64_t)));
    PT_HIP(read_back(c, P.target.data(), M.target, P.target.size() * sizeof(uint16_t)));
    PT_HIP(read_back(c, P.dpos.data(), M.dpos, P.dpos.size() * sizeof(float)));
    if (P.has_dnrm) PT_HIP(read_back(c, P.dnrm.data(), M.dnrm, P.dnrm.size() * sizeof(float)));
    PT_HIP(hipStreamSynchronize(c->stream));
    // the device's own len and first are what the unpacker walks: checked against the sizes the planes were read with
    int64_t steps = 0;
    for (size_t s = 0; s < P.len.size(); s++) {
        if (P.len[s] < 0 || P.first[s] != steps) return fail(PT_ERR_HIP, "read morph: the device's slice table is not the installed morph's");
        steps += P.len[s];
    }
    if (steps != P.steps || !pt::morph_unpack(P, target_first, corner, dpos, dnrm))
        return fail(PT_ERR_HIP, "read morph: the device's planes are not the installed morph's");
    return PT_OK;
}

}  // extern "C"

// ---- re-sorting the triangle BVH on the device, and the BLASes (§4j)
namespace {
// The world tree's new topology, checked against what the upload allocated, and the rebuild workspace: before anything
// is staged.  `who` starts the messages.
int rebuild_world_prepare(Ctx* c, const std::string& who, RebuildRun& run) {
    SceneDyn& Y = c->dyn;
    pt::RebuildPlan& R = run.R;
    const int64_t P = (int64_t)Y.refit.src_of_pos.size();
    if (!pt::rebuild_plan(P, R) || pt::rebuild_stack_bound(R) > pt::kStackMax)
        return fail(PT_ERR_UNSUPPORTED, who + ": " + std::to_string(P) + " triangles need more than " +
                                            std::to_string(pt::kRebuildMaxLevels) + " levels");
    const int64_t node_cap = (int64_t)c->S.tri_chunk_line0 - (int64_t)c->S.tri_node_line0;
    const int64_t chunk_cap = (int64_t)c->S.lines_n - (int64_t)c->S.tri_chunk_line0;
    if (R.num_nodes + R.num_chunks > node_cap + chunk_cap)
        return fail(PT_ERR_UNSUPPORTED, who + ": the balanced tree needs " + std::to_string(R.num_nodes) + " nodes and " +
                                            std::to_string(R.num_chunks) + " chunks, the upload allocated " +
                                            std::to_string(node_cap + chunk_cap) + " lines");
    run.chunk_line0 = R.num_nodes <= node_cap && R.num_chunks <= chunk_cap ? c->S.tri_chunk_line0
                                                                            : c->S.tri_node_line0 + (uint32_t)R.num_nodes;
    RebuildDev sized{};   // pt_rebuild.hip sizes and carves this one: nothing to lay out or upload here
    if (!Y.rebuild_ws.mem.ptr) PT_HIP(pt::rebuild_workspace_bytes(P, &sized.temp_bytes, &sized.bytes));
    return ensure_workspace(c, Y.rebuild_ws, "rebuild", [&](void*) { return sized; }, [](const RebuildDev&, Uploader&) {});
}

// pt_rebuild_meshes and pt_rebuild_blas after their own argument checks: world / blas say which trees are re-sorted
int rebuild_call(Ctx* c, const std::string& who, const pt_mesh_update* u, bool world, bool blas, double* out_kernel_ms) {
    SceneDyn& Y = c->dyn;
    // u NULL: the staged pose, skin or morph with its normals, the lights at their rest vertices
    RebuildRun run{};
    UpdateCall U{Y.refit.num_triangles, Normals::Given, {nullptr, nullptr, nullptr}, nullptr};
    if (u) U = UpdateCall{u->num_triangles, normals_of(u->normals_mode, u->n1), {u->v1, u->v2, u->v3}, nullptr};
    bool launch = false;
    if (const int rc = update_prepare(c, U, true, out_kernel_ms, &launch)) return rc;
    if (!launch) return PT_OK;
    // the new topologies and the workspaces: before anything is staged
    if (world && Y.refit.num_chunks > 0) {   // a scene whose only triangles are instanced launches nothing for the world
        if (const int rc = rebuild_world_prepare(c, who, run)) return rc;
        U.rebuild = &run;
    }
    if (blas && refits_blas(c, U)) {
        if (const int rc = blas_rebuild_prepare(c)) return rc;
        U.rebuild_blas = true;
    }
    const float* const src[6] = {u ? u->v1 : nullptr, u ? u->v2 : nullptr, u ? u->v3 : nullptr, u ? u->n1 : nullptr,
                                 u ? u->n2 : nullptr, u ? u->n3 : nullptr};
    return update_stage_and_run(c, U, u ? src : nullptr, out_kernel_ms);
}
}  // namespace

extern "C" {

int pt_rebuild_meshes(void* ctx, const pt_mesh_update* u, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (u) if (const int rc = check_mesh_update("rebuild meshes", u)) return rc;
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    SceneDyn& Y = c->dyn;
    if (!u && (!Y.pose_staged || !Y.refit_ws.mem.ptr))
        return fail(PT_ERR_INVALID_ARG, "rebuild meshes: u is NULL and the staged arrays hold no pose or skin (pt_pose_meshes, pt_skin_meshes)");
    if (Y.has_blas)
        return fail(PT_ERR_UNSUPPORTED, "rebuild meshes: the scene holds an instanced mesh (a transformed shape over PT_SHAPE_MESH); "
                                        "BLASes are not rebuilt");
    return rebuild_call(c, "rebuild meshes", u, true, false, out_kernel_ms);
}

int pt_rebuild_blas(void* ctx, const pt_mesh_update* u, int32_t what, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (u) if (const int rc = check_mesh_update("rebuild blas", u)) return rc;
    if (what < 0 || what > (PT_REBUILD_WORLD | PT_REBUILD_BLAS))
        return fail(PT_ERR_INVALID_ARG, "rebuild blas: what " + std::to_string(what) + " is not 0 or PT_REBUILD_WORLD | PT_REBUILD_BLAS");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    SceneDyn& Y = c->dyn;
    if (!u && (!Y.pose_staged || !Y.refit_ws.mem.ptr))
        return fail(PT_ERR_INVALID_ARG, "rebuild blas: u is NULL and the staged arrays hold no pose or skin (pt_pose_meshes, pt_skin_meshes)");
    if (what == 0) what = PT_REBUILD_WORLD | PT_REBUILD_BLAS;
    return rebuild_call(c, "rebuild blas", u, (what & PT_REBUILD_WORLD) != 0, (what & PT_REBUILD_BLAS) != 0, out_kernel_ms);
}

int pt_blas_cost(void* ctx, int32_t num_blas, double* out) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!out && num_blas != 0) return fail(PT_ERR_INVALID_ARG, "blas cost: out is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    const pt::BlasRefitTables& T = c->dyn.blas_refit;
    const size_t nb = T.num_blas();
    if (num_blas < 0 || (size_t)num_blas != nb)
        return fail(PT_ERR_INVALID_ARG, "blas cost: num_blas is " + std::to_string(num_blas) + ", the uploaded scene has " +
                                            std::to_string(nb));
    if (nb == 0) return PT_OK;
    PT_HIP(hipSetDevice(c->device));
    // [inner | leaf | out | desc]
    const size_t arrays = pt::blas_cost_workspace_bytes(T.num_nodes), out_bytes = nb * 3 * sizeof(double);
    DeviceArray ws;
    if (hipMalloc(&ws.ptr, arrays + out_bytes + nb * 4 * sizeof(int32_t)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PT_ERR_OUT_OF_MEMORY, "blas cost workspace allocation");
    }
    double* d_out = (double*)((char*)ws.ptr + arrays);
    int32_t* d_desc = (int32_t*)((char*)ws.ptr + arrays + out_bytes);
    int64_t max_nodes = 0;
    for (size_t b = 0; b < nb; b++) max_nodes = std::max(max_nodes, (int64_t)T.desc[4 * b + 1]);
    hipError_t e = hipStreamSynchronize(c->side);   // after every pass issued before
    if (e == hipSuccess) e = hipMemcpyAsync(d_desc, T.desc.data(), nb * 4 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = pt::launch_blas_cost((int64_t)nb, T.num_nodes, max_nodes, d_desc, (const uint32_t*)c->S.blas_nodes, ws.ptr, d_out, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    ws.release();
    PT_HIP(e);
    return PT_OK;
}

int pt_tri_bvh_cost(void* ctx, double out[3]) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!out) return fail(PT_ERR_INVALID_ARG, "bvh cost: out is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    out[0] = out[1] = out[2] = 0.0;
    const int64_t nn = c->dyn.refit.num_nodes;
    if (nn <= 0 || c->dyn.refit.src_of_pos.empty()) return PT_OK;
    PT_HIP(hipSetDevice(c->device));
    size_t bytes = 0;
    PT_HIP(pt::bvh_cost_workspace_bytes(nn, &bytes));
    DeviceArray ws;
    if (hipMalloc(&ws.ptr, bytes + 2 * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PT_ERR_OUT_OF_MEMORY, "bvh cost workspace allocation");
    }
    double* d_sums = (double*)((char*)ws.ptr + bytes);
    double sums[2] = {0.0, 0.0};
    uint32_t root[pt::kNode8Words];
    hipError_t e = hipStreamSynchronize(c->side);   // after every pass issued before
    if (e == hipSuccess) e = pt::launch_bvh_cost(nn, (const uint32_t*)c->S.tri_nodes, ws.ptr, d_sums, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sums, d_sums, sizeof sums, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(root, c->S.tri_nodes, sizeof root, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    ws.release();
    PT_HIP(e);
    double ri = 0.0, rl = 0.0, area = 0.0;
    pt::rebuild_node_cost(root, &ri, &rl, &area);
    out[2] = area;
    if (area > 0.0) {
        out[0] = (area + sums[0]) / area;
        out[1] = sums[1] / area;
    }
    return PT_OK;
}

// ---- instanced meshes and moving shapes read back and moved
int pt_read_blas(void* ctx, int64_t counts[3], int32_t* blas, uint32_t* nodes, uint32_t* recs, uint32_t* shade, float* inner_boxes) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    const pt::BlasRefitTables& T = c->dyn.blas_refit;
    const size_t nb = T.num_blas();
    if (counts) { counts[0] = (int64_t)nb; counts[1] = T.num_nodes; counts[2] = T.num_tris; }
    PT_HIP(hipSetDevice(c->device));
    const size_t word = sizeof(uint32_t);
    PT_HIP(read_back(c, blas, c->S.blas, nb * sizeof(pt::DevBlas)));
    PT_HIP(read_back(c, nodes, c->S.blas_nodes, (size_t)T.num_nodes * pt::kShapeNodeWords * word));
    PT_HIP(read_back(c, recs, c->S.blas_recs, (size_t)T.num_tris * pt::kBlasRecWords * word));
    PT_HIP(read_back(c, shade, c->S.blas_shade, (size_t)T.num_tris * pt::kBlasRecWords * word));
    if (c->dyn.blas_boxes_on_device && c->dyn.blas_ws.mem.ptr) {
        PT_HIP(read_back(c, inner_boxes, c->dyn.blas_ws.at.blas_box, nb * 6 * sizeof(float)));
    } else if (inner_boxes && nb) {   // no update yet: the upload's, from the host table
        const std::vector<float>& host = c->dyn.shape_refit.xf_inner_box;
        std::memset(inner_boxes, 0, nb * 6 * sizeof(float));
        for (size_t t = 0; t < T.xf_blas.size() && 6 * t + 6 <= host.size(); t++) {
            const int64_t b = T.xf_blas[t];
            if (b >= 0 && (size_t)b < nb) std::memcpy(inner_boxes + 6 * b, &host[6 * t], 6 * sizeof(float));
        }
    }
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_update_shapes(void* ctx, const pt_shape_update* u, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!u) return fail(PT_ERR_INVALID_ARG, "update shapes: u is NULL");
    if (u->reserved != 0) return fail(PT_ERR_INVALID_ARG, "update shapes: reserved must be 0");
    if ((u->cube_min != nullptr) != (u->cube_max != nullptr))
        return fail(PT_ERR_INVALID_ARG, "update shapes: cube_min and cube_max must be both set or both NULL");
    if ((u->xform_matrix != nullptr) != (u->xform_inverse != nullptr))
        return fail(PT_ERR_INVALID_ARG, "update shapes: xform_matrix and xform_inverse must be both set or both NULL");
    if (u->sphere_radius && !u->sphere_center)
        return fail(PT_ERR_INVALID_ARG, "update shapes: sphere_radius needs sphere_center");
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    pt::ShapeRefitTables& T = c->dyn.shape_refit;
    auto count_is = [&](const char* what, int32_t given, int32_t have) -> int {
        if (given == have) return PT_OK;
        return fail(PT_ERR_INVALID_ARG, std::string("update shapes: ") + what + " is " + std::to_string(given) +
                                            ", the uploaded scene has " + std::to_string(have));
    };
    if (u->sphere_center) if (const int rc = count_is("num_spheres", u->num_spheres, T.num_spheres)) return rc;
    if (u->cube_min) if (const int rc = count_is("num_cubes", u->num_cubes, T.num_cubes)) return rc;
    if (u->xform_matrix) if (const int rc = count_is("num_transformed", u->num_transformed, T.num_transformed)) return rc;
    // (pt_upload_scene's validate_scene checks no sphere, cube or matrix value: nor does an update)
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if ((!u->sphere_center && !u->cube_min && !u->xform_matrix) || T.num_recs == 0) return PT_OK;
    PT_HIP(hipSetDevice(c->device));
    PT_HIP(hipStreamSynchronize(c->side));   // after every pass issued before, the side stream's work included
    if (const int rc = ensure_shapes_ws(c)) return rc;   // before the first change: a failed allocation leaves the scene untouched
    // the given groups into the current parameters
    if (u->sphere_center) T.sphere_center.assign(u->sphere_center, u->sphere_center + 3 * (size_t)T.num_spheres);
    if (u->sphere_radius) T.sphere_radius.assign(u->sphere_radius, u->sphere_radius + (size_t)T.num_spheres);
    if (u->cube_min) {
        T.cube_min.assign(u->cube_min, u->cube_min + 3 * (size_t)T.num_cubes);
        T.cube_max.assign(u->cube_max, u->cube_max + 3 * (size_t)T.num_cubes);
    }
    if (u->xform_matrix) {
        T.xf_matrix.assign(u->xform_matrix, u->xform_matrix + 16 * (size_t)T.num_transformed);
        T.xf_inverse.assign(u->xform_inverse, u->xform_inverse + 16 * (size_t)T.num_transformed);
    }
    if (const int rc = stage_shape_params(c)) return rc;
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    if (const int rc = launch_shapes(c)) return rc;
    PT_HIP(hipEventRecord(c->ev1, c->stream));
    // lights that are spheres, cubes or transformed shapes: their sphere from the new parameters
    if (pt::shape_refit_lights(T, c->dyn.h_lights)) if (const int rc = upload_lights(c)) return rc;
    PT_HIP(hipStreamSynchronize(c->stream));
    return kernel_ms(c, out_kernel_ms);
}

int pt_read_shape_bvh(void* ctx, int64_t counts[4], uint32_t* nodes, uint32_t* recs, uint32_t* heavy, double* lights) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    const pt::ShapeRefitTables& T = c->dyn.shape_refit;
    const size_t nl = c->dyn.h_lights.size();
    if (counts) { counts[0] = T.num_nodes; counts[1] = T.num_recs; counts[2] = T.num_heavy; counts[3] = (int64_t)nl; }
    PT_HIP(hipSetDevice(c->device));
    const size_t word = sizeof(uint32_t);
    PT_HIP(read_back(c, nodes, c->S.ana_nodes, (size_t)T.num_nodes * pt::kShapeNodeWords * word));
    PT_HIP(read_back(c, recs, c->S.ana_recs, (size_t)T.num_recs * pt::kShapeRecWords * word));
    PT_HIP(read_back(c, heavy, c->S.heavy, (size_t)T.num_heavy * pt::kShapeHeavyWords * word));
    std::vector<pt::DevLight> dl(lights ? nl : 0);   // what the device holds, not the host's copy
    PT_HIP(read_back(c, dl.data(), c->S.lights, dl.size() * sizeof(pt::DevLight)));
    PT_HIP(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < dl.size(); i++) {
        for (int k = 0; k < 3; k++) lights[4 * i + k] = (double)dl[i].center[k];
        lights[4 * i + 3] = dl[i].radius;
    }
    return PT_OK;
}

// ---- Volumes edited in place
static_assert(sizeof(pt_volume_window) == sizeof(pt::DevWindow), "pt_read_volume copies window rows as they are");

int pt_update_volumes(void* ctx, const pt_volume_update* u, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!u) return fail(PT_ERR_INVALID_ARG, "update volumes: u is NULL");
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    SceneDyn& Y = c->dyn;
    const int32_t nv = (int32_t)Y.vols.size();
    std::vector<pt::VolState> state((size_t)nv);
    for (int32_t i = 0; i < nv; i++) state[(size_t)i] = pt::VolState{Y.vols[(size_t)i], Y.vol_windows.data() + Y.vol_win_off[(size_t)i]};
    const char* why = "";
    if (const int rc = pt::vol_update_check(u, nv, state.data(), &why)) return fail(rc, std::string("update volumes: ") + why);
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if (!pt::vol_update_any(u)) return PT_OK;
    // the window rows the call would leave, and the light test with them, before anything is copied or launched
    std::vector<pt::DevWindow> rows = Y.vol_windows;
    std::vector<const pt::DevWindow*> win((size_t)nv);
    std::vector<pt::DevVolume> hdrs = Y.vols;
    for (int32_t i = 0; i < nv; i++) {
        pt::DevWindow* r = rows.data() + Y.vol_win_off[(size_t)i];
        win[(size_t)i] = r;
        if (!u->windows || !u->windows[i]) continue;
        for (int32_t k = 0; k < hdrs[(size_t)i].nwin; k++) { r[k].lo = u->windows[i][k].lo; r[k].hi = u->windows[i][k].hi; }
        pt::DevVolume view = hdrs[(size_t)i];
        view.windows = r;
        hdrs[(size_t)i].zero_sign = pt::vol_zero_sign(view);
    }
    const pt::VolumeTables& T = Y.volume_update;
    std::vector<int32_t> mats(T.slots.size());
    if (const int rc = pt::vol_update_lights(T.slots.data(), T.slots.size(), hdrs.data(), win.data(), T.emittance.data(),
                                             (int32_t)T.emittance.size(), mats.data(), &why))
        return fail(rc, std::string("update volumes: ") + why);
    PT_HIP(hipSetDevice(c->device));
    PT_HIP(hipStreamSynchronize(c->side));   // after every pass issued before, the side stream's work included
    // the copies, then the header words and the windows
    for (int32_t i = 0; i < nv; i++) {
        const pt::DevVolume& v = hdrs[(size_t)i];
        if (u->data && u->data[i])
            PT_HIP(hipMemcpyAsync(const_cast<double*>(v.data), u->data[i], (size_t)v.w * v.h * v.d * sizeof(double),
                                  hipMemcpyHostToDevice, c->stream));
    }
    for (int32_t i = 0; i < nv; i++) {
        if (!u->windows || !u->windows[i]) continue;
        const pt::DevVolume& v = hdrs[(size_t)i];
        PT_HIP(hipMemcpyAsync(const_cast<pt::DevVolume*>(c->S.volumes) + i, &v, sizeof v, hipMemcpyHostToDevice, c->stream));
        if (v.nwin > 0)
            PT_HIP(hipMemcpyAsync(const_cast<pt::DevWindow*>(v.windows), win[(size_t)i], (size_t)v.nwin * sizeof(pt::DevWindow),
                                  hipMemcpyHostToDevice, c->stream));
    }
    // one launch per changed volume
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    for (int32_t i = 0; i < nv; i++) {
        const bool new_data = u->data && u->data[i];
        if (!new_data && !(u->windows && u->windows[i])) continue;
        PT_HIP(pt::launch_vol_rebuild(hdrs[(size_t)i], new_data, c->stream));
    }
    PT_HIP(hipEventRecord(c->ev1, c->stream));
    // a light made from a Volume keeps its place and takes the material the test gives now
    bool lights_changed = false;
    for (size_t s = 0; s < T.slots.size(); s++) {
        const int32_t L = T.slots[s].light;
        if (L < 0 || Y.h_lights[(size_t)L].mat == mats[s]) continue;
        Y.h_lights[(size_t)L].mat = mats[s];
        lights_changed = true;
    }
    if (lights_changed) if (const int rc = upload_lights(c)) return rc;
    PT_HIP(hipStreamSynchronize(c->stream));
    {   // the light test's slots take the materials too: a later pt_update_materials derives the lights from them
        size_t at = 0;
        for (pt::LookSlot& slot : Y.look.slots)
            if (slot.volume >= 0 && at < mats.size()) slot.mat = mats[at++];
    }
    Y.vols = std::move(hdrs);
    Y.vol_windows = std::move(rows);
    return kernel_ms(c, out_kernel_ms);
}

int pt_read_volume(void* ctx, int32_t index, int64_t info[8], double* data, pt_volume_window* windows, int8_t* runs,
                   double* cells) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    if (index < 0 || (size_t)index >= c->dyn.vols.size()) return fail(PT_ERR_INVALID_ARG, "read volume: index outside the scene's volumes");
    PT_HIP(hipSetDevice(c->device));
    pt::DevVolume v{};   // the header the device holds, not the host's copy
    PT_HIP(hipMemcpyAsync(&v, c->S.volumes + index, sizeof v, hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    const uint64_t ncells = pt::vol_cell_count(v.w, v.h, v.d);
    if (info) {
        const int64_t o[8] = {v.w, v.h, v.d, v.nwin, v.zero_sign, v.cells ? 1 : 0, (int64_t)ncells, 0};
        std::memcpy(info, o, sizeof o);
    }
    PT_HIP(read_back(c, data, v.data, (size_t)v.w * v.h * v.d * sizeof(double)));
    PT_HIP(read_back(c, windows, v.windows, (size_t)v.nwin * sizeof(pt::DevWindow)));
    PT_HIP(read_back(c, runs, v.runs, v.runs ? (size_t)ncells : 0));
    PT_HIP(read_back(c, cells, v.cells, v.cells ? (size_t)pt::vol_cell_byte(ncells) : 0));
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}

// ---- the look edited in place
int pt_update_materials(void* ctx, const pt_material_update* u, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!u) return fail(PT_ERR_INVALID_ARG, "update materials: u is NULL");
    if (u->reserved[0] != 0 || u->reserved[1] != 0) return fail(PT_ERR_INVALID_ARG, "update materials: reserved must be 0");
    if (u->flags != 0 && u->flags != PT_LOOK_ENV) return fail(PT_ERR_INVALID_ARG, "update materials: flags must be 0 or PT_LOOK_ENV");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    SceneDyn& Y = c->dyn;
    const int32_t nm = (int32_t)Y.h_mats.size() - 1, nt = (int32_t)Y.texs.size();   // (the last row is `new Material()`)
    auto slot_ok = [&](int32_t t) { return t >= 0 && t <= nt; };
    if (u->materials) {
        if (u->num_materials != nm)
            return fail(PT_ERR_INVALID_ARG, "update materials: num_materials is " + std::to_string(u->num_materials) +
                                                ", the uploaded scene has " + std::to_string(nm));
        for (int32_t i = 0; i < nm; i++) {
            const pt_material& m = u->materials[i];
            if (!slot_ok(m.texture) || !slot_ok(m.normal_texture) || !slot_ok(m.bump_texture) || !slot_ok(m.gloss_texture))
                return fail(PT_ERR_INVALID_ARG, "update materials: material " + std::to_string(i) + ": texture reference out of range");
        }
    }
    const bool env = (u->flags & PT_LOOK_ENV) != 0;
    if (env && !slot_ok(u->env_texture)) return fail(PT_ERR_INVALID_ARG, "update materials: env_texture out of range");
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if (!u->materials && !env) return PT_OK;
    // everything the call would leave, derived on the host before the first copy: the table, the lights with their
    // side tables, the flags (the upload's own derivation, pt_scene_compile.cpp look_lights / look_flags)
    std::vector<pt::DevMaterial> mats = Y.h_mats;
    if (u->materials) for (int32_t i = 0; i < nm; i++) pt::pack_material(u->materials[i], mats[(size_t)i]);
    pt::LookLights L;
    pt::look_lights(Y.look, Y.shape_refit, mats, L);
    pt::DevScene S = c->S;
    pt::look_flags(Y.look, L.lights, mats, S.tri_num_nodes, S);
    S.num_lights = (int32_t)L.lights.size();
    if (env) {
        S.env_tex = u->env_texture - 1;
        S.env_angle = u->env_texture_angle;
        for (int k = 0; k < 3; k++) S.env[k] = u->env_color[k];
    }
    PT_HIP(hipSetDevice(c->device));
    PT_HIP(hipStreamSynchronize(c->side));   // after every pass issued before, the side stream's work included
    if (L.lights.size() > Y.lights_cap) {    // once, to the most a scene can have: one light per Scene.Shapes slot
        DeviceArray a;
        a.bytes = Y.look.slots.size() * sizeof(pt::DevLight);
        if (hipMalloc(&a.ptr, a.bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PT_ERR_OUT_OF_MEMORY, "update materials: light array allocation");
        }
        c->scene_arrays.push_back(a);   // (the upload's array goes with the scene too)
        S.lights = (const pt::DevLight*)a.ptr;
        c->S.lights = S.lights;
        Y.lights_cap = Y.look.slots.size();
        if (!Y.h_lights.empty()) if (const int rc = upload_lights(c)) return rc;   // the current lights, in the new array
    }
    // (as in the other updates, a copy or the synchronisation failing from here on is PT_ERR_HIP with the device's
    // tables part old, part new: the context needs a pt_upload_scene)
    if (u->materials)
        PT_HIP(hipMemcpyAsync(const_cast<pt::DevMaterial*>(c->S.mats), mats.data(), mats.size() * sizeof(pt::DevMaterial),
                              hipMemcpyHostToDevice, c->stream));
    if (!L.lights.empty())
        PT_HIP(hipMemcpyAsync(const_cast<pt::DevLight*>(S.lights), L.lights.data(), L.lights.size() * sizeof(pt::DevLight),
                              hipMemcpyHostToDevice, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    c->S = S;
    Y.h_mats = std::move(mats);
    Y.h_lights = std::move(L.lights);
    Y.refit.light_tri = std::move(L.light_tri);
    Y.shape_refit.light_kind = std::move(L.light_kind);
    Y.shape_refit.light_index = std::move(L.light_index);
    Y.volume_update.slots = std::move(L.vol_slots);
    Y.volume_update.emittance = std::move(L.emittance);
    Y.look.light_slot = std::move(L.light_slot);
    return PT_OK;
}

int pt_read_materials(void* ctx, pt_look_info* info, pt_material* materials, int32_t* light_rows, double* light_spheres) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    const pt::DevScene& S = c->S;
    const size_t nm = (size_t)S.default_mat, nl = (size_t)S.num_lights;
    if (info) {
        std::memset(info, 0, sizeof *info);
        info->num_materials = (int32_t)nm;
        info->num_textures = (int32_t)c->dyn.texs.size();
        info->num_lights = S.num_lights;
        info->lights_lean = S.lights_lean; info->route = S.route; info->shade_route = S.shade_route;
        info->env_texture = S.env_tex + 1;
        for (int k = 0; k < 3; k++) info->env_color[k] = S.env[k];
        info->env_texture_angle = S.env_angle;
    }
    PT_HIP(hipSetDevice(c->device));
    std::vector<pt::DevMaterial> dm(materials ? nm : 0);   // what the device holds, not the host's copies
    std::vector<pt::DevLight> dl(light_rows || light_spheres ? nl : 0);
    PT_HIP(read_back(c, dm.data(), S.mats, dm.size() * sizeof(pt::DevMaterial)));
    PT_HIP(read_back(c, dl.data(), S.lights, dl.size() * sizeof(pt::DevLight)));
    PT_HIP(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < dm.size(); i++) {
        const pt::DevMaterial& m = dm[i];
        pt_material& o = materials[i];
        std::memset(&o, 0, sizeof o);
        for (int k = 0; k < 3; k++) o.color[k] = m.color[k];
        o.emittance = m.emittance; o.index = m.index; o.gloss = m.gloss; o.tint = m.tint; o.reflectivity = m.reflectivity;
        o.transparent = m.transparent;
        o.texture = m.tex + 1; o.normal_texture = m.ntex + 1; o.bump_texture = m.btex + 1; o.gloss_texture = m.gtex + 1;
        o.bump_multiplier = m.bump_multiplier;
    }
    for (size_t i = 0; i < dl.size(); i++) {
        if (light_rows) { light_rows[4 * i] = dl[i].kind; light_rows[4 * i + 1] = dl[i].index; light_rows[4 * i + 2] = dl[i].mat; light_rows[4 * i + 3] = dl[i].phantom; }
        if (light_spheres) {
            for (int k = 0; k < 3; k++) light_spheres[4 * i + k] = (double)dl[i].center[k];
            light_spheres[4 * i + 3] = dl[i].radius;
        }
    }
    return PT_OK;
}

int pt_update_textures(void* ctx, const pt_texture_update* u, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!u) return fail(PT_ERR_INVALID_ARG, "update textures: u is NULL");
    if (u->reserved[0] != 0 || u->reserved[1] != 0 || u->reserved[2] != 0) return fail(PT_ERR_INVALID_ARG, "update textures: reserved must be 0");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    SceneDyn& Y = c->dyn;
    const int32_t nt = (int32_t)Y.texs.size();
    if (u->num_textures != nt)
        return fail(PT_ERR_INVALID_ARG, "update textures: num_textures is " + std::to_string(u->num_textures) +
                                            ", the uploaded scene has " + std::to_string(nt));
    bool any = false, any8 = false;
    for (int32_t i = 0; u->images && i < nt; i++) {
        const pt_texture_image* im = u->images[i];
        if (!im) continue;
        const std::string who = "update textures: image " + std::to_string(i);
        if (im->reserved != 0) return fail(PT_ERR_INVALID_ARG, who + ": reserved must be 0");
        if (im->width != Y.texs[(size_t)i].w || im->height != Y.texs[(size_t)i].h)
            return fail(PT_ERR_INVALID_ARG, who + ": width and height differ from the uploaded texture's");
        if (im->format != PT_TEXELS_F64 && im->format != PT_TEXELS_RGB8 && im->format != PT_TEXELS_RGBA8)
            return fail(PT_ERR_INVALID_ARG, who + ": format is not a pt_texel_format");
        if (!im->data) return fail(PT_ERR_INVALID_ARG, who + ": data is NULL");
        if (im->format != PT_TEXELS_F64 && !im->lut) return fail(PT_ERR_INVALID_ARG, who + ": an 8-bit format needs lut");
        any = true;
        any8 = any8 || im->format != PT_TEXELS_F64;
    }
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if (!any) return PT_OK;
    PT_HIP(hipSetDevice(c->device));
    // the byte staging: every texture's table (2 KiB each), then room for every texture as RGBA8; before the first copy
    const size_t luts = (size_t)nt * pt::kTexLut * sizeof(double);
    if (any8 && !Y.tex_stage.ptr) {
        size_t bytes = luts;
        for (const pt::DevTexture& t : Y.texs) bytes += (size_t)pt::tex_pixels(t.w, t.h) * 4;
        if (hipMalloc(&Y.tex_stage.ptr, bytes) != hipSuccess) {
            Y.tex_stage.ptr = nullptr;
            (void)hipGetLastError();
            return fail(PT_ERR_OUT_OF_MEMORY, "update textures: byte staging allocation");
        }
        Y.tex_stage.bytes = bytes;
    }
    PT_HIP(hipStreamSynchronize(c->side));   // after every pass issued before, the side stream's work included
    uint8_t* stage = (uint8_t*)Y.tex_stage.ptr;
    std::vector<uint64_t> src_off((size_t)nt, 0);
    uint64_t at = luts;   // the images packed one after another, in the formats this call gives
    for (int32_t i = 0; i < nt; i++) {
        const pt_texture_image* im = u->images[i];
        if (!im) continue;
        const pt::DevTexture& t = Y.texs[(size_t)i];
        const uint64_t pixels = pt::tex_pixels(t.w, t.h);
        if (im->format == PT_TEXELS_F64) {
            PT_HIP(hipMemcpyAsync(const_cast<double*>(t.data), im->data, (size_t)pixels * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
            continue;
        }
        const size_t bytes = (size_t)pixels * (size_t)pt::tex_bpp(im->format);
        src_off[(size_t)i] = at;
        PT_HIP(hipMemcpyAsync(stage + (size_t)i * pt::kTexLut * sizeof(double), im->lut, pt::kTexLut * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PT_HIP(hipMemcpyAsync(stage + at, im->data, bytes, hipMemcpyHostToDevice, c->stream));
        at += bytes;
    }
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    for (int32_t i = 0; i < nt && any8; i++) {
        const pt_texture_image* im = u->images[i];
        if (!im || im->format == PT_TEXELS_F64) continue;
        const pt::DevTexture& t = Y.texs[(size_t)i];
        PT_HIP(pt::launch_tex_decode(stage, src_off[(size_t)i], im->format, pt::tex_pixels(t.w, t.h),
                                     (const double*)(stage + (size_t)i * pt::kTexLut * sizeof(double)), const_cast<double*>(t.data), c->stream));
    }
    PT_HIP(hipEventRecord(c->ev1, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    return any8 ? kernel_ms(c, out_kernel_ms) : PT_OK;
}

int pt_read_texture(void* ctx, int32_t index, int32_t info[4], double* data) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    if (index < 0 || (size_t)index >= c->dyn.texs.size()) return fail(PT_ERR_INVALID_ARG, "read texture: index outside the scene's textures");
    PT_HIP(hipSetDevice(c->device));
    pt::DevTexture t{};   // the header the device holds, not the host's copy
    PT_HIP(hipMemcpyAsync(&t, c->S.texs + index, sizeof t, hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    if (info) { info[0] = t.w; info[1] = t.h; info[2] = 0; info[3] = 0; }
    PT_HIP(read_back(c, data, t.data, (size_t)pt::tex_pixels(t.w, t.h) * 3 * sizeof(double)));
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}

}  // extern "C"

// ---- pt_intersect_hits
namespace {
// The identity tables on the device: uploaded by the scene's first query, gone with the scene.  The query keeps its own
// copy of position -> source triangle (the refit workspace's exists only after an update), and takes
// RefitTables::src_of_pos again after a pt_rebuild_meshes permuted it.
int ensure_query_ws(Ctx* c) {
    SceneDyn& Y = c->dyn;
    bool first = false;
    if (const int rc = ensure_workspace(c, Y.query_ws, "query", [&](void* base) { return pt::query_layout(Y.refit, Y.blas_refit, Y.query, base); },
                                        [&](const pt::QueryDev& D, Uploader& up) {
                                            up(D.tri_src, Y.refit.src_of_pos);
                                            up(D.blas_src, Y.blas_refit.src_of_pos);
                                            up(D.tri_slot, Y.query.tri_slot);
                                            up(D.ana_slot, Y.query.ana_slot);
                                            up(D.plane_slot, Y.query.plane_slot);
                                        },
                                        &first))
        return rc;
    if (!first && Y.query_src_stale) {
        Uploader up{c->stream};
        up(Y.query_ws.at.tri_src, Y.refit.src_of_pos);
        if (const int rc = check_hip(up.err, "query: the rebuilt triangle order")) return rc;
    }
    if (!first && Y.query_blas_src_stale) {
        Uploader up{c->stream};
        up(Y.query_ws.at.blas_src, Y.blas_refit.src_of_pos);
        if (const int rc = check_hip(up.err, "query: the rebuilt BLAS order")) return rc;
    }
    Y.query_src_stale = false;
    Y.query_blas_src_stale = false;
    return PT_OK;
}

// The kernels' view of the identity tables, after ensure_query_ws
pt::QueryDevTables query_dev_tables(const Ctx* c) {
    const SceneDyn& Y = c->dyn;
    const pt::QueryDev& D = Y.query_ws.at;
    pt::QueryDevTables T{};
    T.tri_src = D.tri_src; T.tri_src_n = (int64_t)Y.refit.src_of_pos.size();
    T.blas_src = D.blas_src; T.blas_src_n = (int64_t)Y.blas_refit.src_of_pos.size();
    T.tri_slot = D.tri_slot; T.tri_slot_n = (int64_t)Y.query.tri_slot.size();
    T.ana_slot = D.ana_slot; T.ana_slot_n = (int64_t)Y.query.ana_slot.size();
    T.plane_slot = D.plane_slot; T.plane_slot_n = (int64_t)Y.query.plane_slot.size();
    std::memcpy(T.ana_off, Y.query.ana_off, sizeof T.ana_off);
    std::memcpy(T.ana_cnt, Y.query.ana_cnt, sizeof T.ana_cnt);
    T.num_blas = (int32_t)Y.blas_refit.num_blas();
    return T;
}

// PT_QUERY_CHUNK, read at each call (tests set it): rays staged at a time
int64_t query_chunk() {
    const char* e = std::getenv("PT_QUERY_CHUNK");
    if (!e || !*e) return pt::kQueryChunkMax;
    return std::min(std::max((int64_t)std::atoll(e), pt::kQueryChunkMin), pt::kQueryChunkMax);
}

// One output of pt_hit_arrays: the host's array (NULL: not wanted), its staged chunk on the device, bytes per ray
struct QueryPart {
    void* host;
    void** dev;
    size_t stride;
};
}  // namespace

extern "C" {

int pt_intersect_hits(void* ctx, int64_t n, const float* origins, const float* dirs, int32_t flags, const pt_hit_arrays* out) {
    Ctx* c = (Ctx*)ctx;
    const std::string who = "pt_intersect_hits";
    if (!c || !out) return fail(PT_ERR_INVALID_ARG, who + ": ctx or out is NULL");
    if (out->reserved[0] != 0 || out->reserved[1] != 0) return fail(PT_ERR_INVALID_ARG, who + ": reserved must be 0");
    if (n < 0 || n > (int64_t)1 << 30) return fail(PT_ERR_INVALID_ARG, who + ": n out of range [0, 2^30]");
    if (n > 0 && (!origins || !dirs)) return fail(PT_ERR_INVALID_ARG, who + ": origins or dirs is NULL");
    if (flags & ~(PT_MARCH_LANE | PT_MARCH_WAVE) || (flags & PT_MARCH_LANE && flags & PT_MARCH_WAVE))
        return fail(PT_ERR_INVALID_ARG, who + ": flags: PT_MARCH_LANE or PT_MARCH_WAVE, not both");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    pt::QueryOut O{};
    const QueryPart parts[] = {
        {out->t, (void**)&O.t, sizeof(double)},           {out->kind, (void**)&O.kind, sizeof(int32_t)},
        {out->index, (void**)&O.index, sizeof(int32_t)},  {out->prim, (void**)&O.prim, sizeof(int32_t)},
        {out->shape, (void**)&O.shape, sizeof(int32_t)},  {out->position, (void**)&O.position, 3 * sizeof(float)},
        {out->normal, (void**)&O.normal, 3 * sizeof(float)}, {out->inside, (void**)&O.inside, sizeof(int32_t)},
        {out->material, (void**)&O.material, sizeof(int32_t)}, {out->albedo, (void**)&O.albedo, 3 * sizeof(double)},
        {out->gloss, (void**)&O.gloss, sizeof(double)}};
    bool wanted = false;
    for (const QueryPart& p : parts) wanted = wanted || p.host;
    c->query_kernel_ms = 0.0;
    if (n == 0 || !wanted) return PT_OK;
    PT_HIP(hipSetDevice(c->device));
    if (const int rc = ensure_query_ws(c)) return rc;
    // the staging of one chunk: [origins | dirs | every wanted output], parts 256-B aligned
    const int64_t chunk = std::min(query_chunk(), n);
    float *d_o = nullptr, *d_d = nullptr;
    auto carve = [&](void* base) {
        pt::Carver cv(base);
        d_o = cv.take<float>((size_t)chunk * 3);
        d_d = cv.take<float>((size_t)chunk * 3);
        for (const QueryPart& p : parts) if (p.host) *p.dev = cv.take<char>((size_t)chunk * p.stride);
        return cv.bytes();
    };
    void* staging = nullptr;
    if (hipMalloc(&staging, carve(nullptr)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PT_ERR_OUT_OF_MEMORY, who + ": staging allocation");
    }
    carve(staging);
    const pt::QueryDevTables T = query_dev_tables(c);
    pt::DevScene S = c->S;
    S.march = nullptr;
    if (flags & PT_MARCH_LANE) S.coop_min_lanes = 65;   // as pt_intersect sets them
    if (flags & PT_MARCH_WAVE) S.coop_min_lanes = 1;
    int rc = PT_OK;
    auto step = [&](hipError_t err, const char* what) {
        if (rc == PT_OK && err != hipSuccess) rc = fail(PT_ERR_HIP, who + ": " + what + ": " + hipGetErrorString(err));
    };
    for (int64_t at = 0; at < n && rc == PT_OK; at += chunk) {
        const size_t m = (size_t)std::min(chunk, n - at);
        step(hipMemcpyAsync(d_o, origins + 3 * at, m * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream), "origins");
        step(hipMemcpyAsync(d_d, dirs + 3 * at, m * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream), "dirs");
        step(hipEventRecord(c->ev0, c->stream), "hipEventRecord");
        if (rc == PT_OK) step(pt::launch_intersect_hits(S, T, (int64_t)m, d_o, d_d, O, c->stream), "k_intersect_hits");
        step(hipEventRecord(c->ev1, c->stream), "hipEventRecord");
        for (const QueryPart& p : parts)
            if (p.host && rc == PT_OK)
                step(hipMemcpyAsync((char*)p.host + (size_t)at * p.stride, *p.dev, m * p.stride, hipMemcpyDeviceToHost, c->stream), "answers");
        step(hipStreamSynchronize(c->stream), "hipStreamSynchronize");   // the next chunk reuses the staging
        float ms = 0.f;
        if (rc == PT_OK) step(hipEventElapsedTime(&ms, c->ev0, c->ev1), "hipEventElapsedTime");
        c->query_kernel_ms += ms;
    }
    if (rc != PT_OK) (void)hipStreamSynchronize(c->stream);
    (void)hipFree(staging);
    return rc;
}

int pt_query_kernel_ms(void* ctx, double* out_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !out_ms) return fail(PT_ERR_INVALID_ARG, "NULL argument");
    *out_ms = c->query_kernel_ms;
    return PT_OK;
}

}  // extern "C"

// ---- motion vectors and temporal accumulation
namespace {
// pt_motion_snapshot's storage: [world records by source | BLAS records by source | analytic records | xforms | ext_recs]
struct MotionSnapDev {
    float4 *tris, *blas, *ana, *ext;
    pt::DevXform* xforms;
    size_t bytes;
};
MotionSnapDev motion_snap_layout(const Ctx* c, void* base) {
    const SceneDyn& Y = c->dyn;
    const size_t num_src = (size_t)std::max(Y.refit.num_triangles, 0);
    pt::Carver cv(base);
    MotionSnapDev r{};
    r.tris = cv.take<float4>(Y.refit.src_of_pos.empty() ? 0 : 3 * num_src);
    r.blas = cv.take<float4>(Y.blas_refit.src_of_pos.empty() ? 0 : 3 * num_src);
    r.ana = cv.take<float4>(3 * (size_t)std::max(c->S.ana_count, 0));
    r.xforms = cv.take<pt::DevXform>((size_t)Y.num_xforms);
    r.ext = cv.take<float4>(3 * (size_t)Y.num_ext_recs);
    r.bytes = cv.bytes();
    return r;
}

int device_storage(DeviceArray& a, size_t bytes, const char* name) {
    if (a.ptr) return PT_OK;
    if (hipMalloc(&a.ptr, bytes) != hipSuccess) {
        a.ptr = nullptr;
        (void)hipGetLastError();
        return fail(PT_ERR_OUT_OF_MEMORY, std::string(name) + " allocation");
    }
    a.bytes = bytes;
    return PT_OK;
}

pt::DevCamera features_camera(const pt_camera* camera) {
    pt::DevCamera cam;
    std::memcpy(cam.p, camera->p, sizeof cam.p); std::memcpy(cam.u, camera->u, sizeof cam.u);
    std::memcpy(cam.v, camera->v, sizeof cam.v); std::memcpy(cam.w, camera->w, sizeof cam.w);
    cam.m = camera->m; cam.focal_distance = camera->focal_distance;
    cam.aperture_radius = 0.0;   // the lens is ignored: one deterministic ray through the pixel
    return cam;
}

// The two history sets, then the merge's status
size_t temporal_bytes(const Ctx* c) {
    return 2 * pt::temporal_set_bytes(c->width, c->height) + (size_t)c->width * (size_t)c->height * sizeof(int32_t);
}
pt::TemporalSet temporal_set(const Ctx* c, int which) {
    return pt::temporal_set_of((char*)c->dyn.temporal.ptr + (size_t)which * pt::temporal_set_bytes(c->width, c->height), c->width, c->height);
}
int32_t* temporal_status_array(const Ctx* c) {
    return (int32_t*)((char*)c->dyn.temporal.ptr + 2 * pt::temporal_set_bytes(c->width, c->height));
}
}  // namespace

extern "C" {

int pt_motion_snapshot(void* ctx, const pt_camera* camera) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !camera) return fail(PT_ERR_INVALID_ARG, "pt_motion_snapshot: ctx or camera is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    PT_HIP(hipSetDevice(c->device));
    if (const int rc = ensure_query_ws(c)) return rc;
    SceneDyn& Y = c->dyn;
    const bool first = !Y.motion_snap.ptr;
    if (const int rc = device_storage(Y.motion_snap, motion_snap_layout(c, nullptr).bytes, "motion snapshot")) return rc;
    const MotionSnapDev D = motion_snap_layout(c, Y.motion_snap.ptr);
    if (first) PT_HIP(hipMemsetAsync(Y.motion_snap.ptr, 0, Y.motion_snap.bytes, c->stream));
    const pt::DevScene& S = c->S;
    const pt::QueryDev& Q = Y.query_ws.at;
    const int64_t num_src = (int64_t)std::max(Y.refit.num_triangles, 0);
    const int64_t world_pos = (int64_t)Y.refit.src_of_pos.size(), blas_pos = (int64_t)Y.blas_refit.src_of_pos.size();
    if (world_pos > 0 && S.tri_recs)
        PT_HIP(pt::launch_motion_snapshot_tris(world_pos, S.tri_recs, S.tri_rstride, Q.tri_src, num_src, D.tris, c->stream));
    if (blas_pos > 0 && S.blas_recs)
        PT_HIP(pt::launch_motion_snapshot_tris(blas_pos, S.blas_recs, 3, Q.blas_src, num_src, D.blas, c->stream));
    const size_t ana_bytes = 3 * (size_t)std::max(S.ana_count, 0) * sizeof(float4);
    if (ana_bytes && S.ana_recs) PT_HIP(hipMemcpyAsync(D.ana, S.ana_recs, ana_bytes, hipMemcpyDeviceToDevice, c->stream));
    if (Y.num_xforms && S.xforms)
        PT_HIP(hipMemcpyAsync(D.xforms, S.xforms, (size_t)Y.num_xforms * sizeof(pt::DevXform), hipMemcpyDeviceToDevice, c->stream));
    if (Y.num_ext_recs && S.ext_recs)
        PT_HIP(hipMemcpyAsync(D.ext, S.ext_recs, 3 * (size_t)Y.num_ext_recs * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    pt::MotionSnap N{};
    N.tris = world_pos > 0 && S.tri_recs ? D.tris : nullptr;
    N.blas = blas_pos > 0 && S.blas_recs ? D.blas : nullptr;
    N.ana = ana_bytes && S.ana_recs ? D.ana : nullptr;
    N.xforms = Y.num_xforms && S.xforms ? D.xforms : nullptr;
    N.ext = Y.num_ext_recs && S.ext_recs ? D.ext : nullptr;
    N.num_src = num_src;
    N.num_ana = (int64_t)std::max(S.ana_count, 0);
    N.num_xforms = Y.num_xforms;
    N.num_ext = Y.num_ext_recs;
    for (int k = 0; k < 3; k++) {
        N.cam.p[k] = camera->p[k]; N.cam.u[k] = camera->u[k];
        N.cam.v[k] = camera->v[k]; N.cam.w[k] = camera->w[k];
    }
    N.cam.m = camera->m;
    N.have = 1;
    Y.snap = N;
    return PT_OK;
}

int pt_render_motion(void* ctx, const pt_camera* camera, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !camera) return fail(PT_ERR_INVALID_ARG, "pt_render_motion: ctx or camera is NULL");
    if (!c->has_scene) return fail(PT_ERR_NO_SCENE, "no scene uploaded");
    PT_HIP(hipSetDevice(c->device));
    if (const int rc = ensure_query_ws(c)) return rc;
    SceneDyn& Y = c->dyn;
    if (const int rc = device_storage(Y.motion_out, pt::motion_bytes(c->width, c->height), "motion result")) return rc;
    const pt::QueryDevTables T = query_dev_tables(c);
    pt::DevScene S = c->S;
    S.march = nullptr;
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    PT_HIP(pt::launch_motion(S, T, Y.snap, features_camera(camera), pt::motion_of(Y.motion_out.ptr, c->width, c->height), c->width,
                             c->height, c->stream));
    PT_HIP(hipEventRecord(c->ev1, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    Y.have_motion = true;
    Y.motion_fresh = true;
    return kernel_ms(c, out_kernel_ms);
}

int pt_read_motion(void* ctx, int32_t what, void* out) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !out) return fail(PT_ERR_INVALID_ARG, "pt_read_motion: ctx or out is NULL");
    if (what < PT_MOTION_SHAPE_I32 || what > PT_MOTION_STATUS_I32) return fail(PT_ERR_INVALID_ARG, "pt_read_motion: what is not a pt_motion_array");
    if (!c->dyn.have_motion) return fail(PT_ERR_INVALID_ARG, "pt_read_motion before any pt_render_motion on this scene");
    PT_HIP(hipSetDevice(c->device));
    const size_t P = (size_t)c->width * (size_t)c->height;
    const pt::MotionOut M = pt::motion_of(c->dyn.motion_out.ptr, c->width, c->height);
    const void* src = nullptr;
    size_t bytes = P * sizeof(int32_t);
    switch (what) {
        case PT_MOTION_SHAPE_I32: src = M.shape; break;
        case PT_MOTION_PRIM_I32: src = M.prim; break;
        case PT_MOTION_DEPTH_F64: src = M.depth; bytes = P * sizeof(double); break;
        case PT_MOTION_PREV_XY_F64: src = M.prev_xy; bytes = 2 * P * sizeof(double); break;
        case PT_MOTION_PREV_DEPTH_F64: src = M.prev_depth; bytes = P * sizeof(double); break;
        case PT_MOTION_PREV_PIXEL_I32: src = M.prev_pixel; break;
        default: src = M.status; break;
    }
    PT_HIP(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_accumulate_temporal(void* ctx, const pt_temporal_params* params, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    const int32_t max_history = params ? params->max_history : 32;
    const double sigma_depth = params ? params->sigma_depth : 0.1;
    if (max_history < 0 || max_history > (1 << 20)) return fail(PT_ERR_INVALID_ARG, "accumulate_temporal: max_history must be 0..2^20");
    if (params && params->reserved != 0) return fail(PT_ERR_INVALID_ARG, "accumulate_temporal: reserved must be 0");
    if (!(sigma_depth >= 0.0) || !std::isfinite(sigma_depth))
        return fail(PT_ERR_INVALID_ARG, "accumulate_temporal: sigma_depth must be finite and >= 0");
    SceneDyn& Y = c->dyn;
    if (!Y.motion_fresh)
        return fail(PT_ERR_INVALID_ARG, "pt_accumulate_temporal needs a pt_render_motion since the last accumulate or reset");
    PT_HIP(hipSetDevice(c->device));
    if (const int rc = device_storage(Y.temporal, temporal_bytes(c), "temporal history")) return rc;
    const int next = 1 - Y.temporal_cur;
    PT_HIP(hipEventRecord(c->ev0, c->stream));
    PT_HIP(pt::launch_temporal_merge(c->width, c->height, c->d_m, c->d_v, c->d_n, pt::motion_of(Y.motion_out.ptr, c->width, c->height),
                                     temporal_set(c, Y.temporal_cur), Y.have_history, max_history, sigma_depth, temporal_set(c, next),
                                     temporal_status_array(c), c->stream));
    PT_HIP(hipEventRecord(c->ev1, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    Y.temporal_cur = next;
    Y.have_history = true;
    Y.have_temporal = true;
    Y.motion_fresh = false;
    return kernel_ms(c, out_kernel_ms);
}

int pt_read_temporal(void* ctx, double* m, double* v, int32_t* n, int32_t* status) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->dyn.have_temporal) return fail(PT_ERR_INVALID_ARG, "pt_read_temporal before any pt_accumulate_temporal on this scene");
    PT_HIP(hipSetDevice(c->device));
    const size_t P = (size_t)c->width * (size_t)c->height;
    const pt::TemporalSet R = temporal_set(c, c->dyn.temporal_cur);
    if (m) PT_HIP(hipMemcpyAsync(m, R.m, 3 * P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (v) PT_HIP(hipMemcpyAsync(v, R.v, 3 * P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (n) PT_HIP(hipMemcpyAsync(n, R.n, P * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (status) PT_HIP(hipMemcpyAsync(status, temporal_status_array(c), P * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_denoise_temporal(void* ctx, const pt_denoise_params* plain, const pt_denoise_guided_params* guided, double* out_kernel_ms) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (plain && guided) return fail(PT_ERR_INVALID_ARG, "pt_denoise_temporal: plain or guided, not both");
    if (!c->dyn.have_temporal) return fail(PT_ERR_INVALID_ARG, "pt_denoise_temporal before any pt_accumulate_temporal on this scene");
    const pt::TemporalSet R = temporal_set(c, c->dyn.temporal_cur);
    if (guided) return denoise_guided_on(c, guided, R.m, R.v, R.n, out_kernel_ms);
    return denoise_on(c, plain, R.m, R.v, R.n, out_kernel_ms);
}

int pt_reset_temporal(void* ctx) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    SceneDyn& Y = c->dyn;
    Y.have_history = Y.have_temporal = Y.have_motion = Y.motion_fresh = false;
    return PT_OK;
}

int pt_scene_bvh_digest(const pt_scene_desc* d, uint64_t out[4]) {
    if (!out) return fail(PT_ERR_INVALID_ARG, "out is NULL");
    std::string err;
    const int rc = pt::validate_scene(d, err);
    if (rc != PT_OK) return fail(rc, err);
    const std::shared_ptr<const pt::TriBvhBuild> b = pt::tri_bvh_shared(d, pt::gather_tri_src(d));   // pt_upload_scene's triangle order
    if (b->rc != PT_OK) return fail(b->rc, b->err);
    uint64_t h = 0xCBF29CE484222325ull;
    auto eat = [&](const void* p, size_t n) {
        const unsigned char* q = (const unsigned char*)p;
        for (size_t i = 0; i < n; i++) h = (h ^ q[i]) * 0x100000001B3ull;
    };
    eat(b->order.data(), b->order.size() * sizeof(uint32_t));
    eat(b->nodes.data(), b->nodes.size() * sizeof(float4));
    eat(b->chunks.data(), b->chunks.size() * sizeof(float4));
    out[0] = h;
    out[1] = (uint64_t)(b->nodes.size() + b->chunks.size()) * sizeof(float4);
    const pt::TriBvhStats cs = pt::tri_bvh_stats();
    out[2] = (uint64_t)cs.builds;
    out[3] = (uint64_t)cs.hits;
    return PT_OK;
}

int pt_stats_get(void* ctx, pt_stats* out) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !out) return fail(PT_ERR_INVALID_ARG, "NULL argument");
    *out = c->stats;
    return PT_OK;
}

void pt_destroy(void* ctx) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) { ncclCommDestroy(c->comm); c->comm = nullptr; }
    pt::tri_bvh_release(c->tri_build);
    free_scene(c);
    free_wavefront(c);
    if (c->d_m) (void)hipFree(c->d_m);
    if (c->d_v) (void)hipFree(c->d_v);
    if (c->d_n) (void)hipFree(c->d_n);
    if (c->d_counters) (void)hipFree(c->d_counters);
    if (c->h_counters) (void)hipHostFree(c->h_counters);
    if (c->d_tiles) (void)hipFree(c->d_tiles);
    if (c->d_image) (void)hipFree(c->d_image);
    if (c->d_denoise) (void)hipFree(c->d_denoise);
    if (c->d_features) (void)hipFree(c->d_features);
    if (c->d_own) (void)hipFree(c->d_own);
    for (void* p : {(void*)c->g_ids, (void*)c->g_m, (void*)c->g_v, (void*)c->g_n, (void*)c->g_cnts, (void*)c->g_all})
        if (p) (void)hipFree(p);
    c->timer.destroy();
    if (c->ev_main) (void)hipEventDestroy(c->ev_main);
    for (hipEvent_t e : c->ev_side) if (e) (void)hipEventDestroy(e);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// ------------------------------------------------------------------ RCCL
int pt_comm_unique_id(uint8_t out_id[128]) {
    if (!out_id) return fail(PT_ERR_INVALID_ARG, "out_id is NULL");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(PT_ERR_RCCL, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    std::memcpy(out_id, &id, 128);
    return PT_OK;
}

int pt_comm_init(void* ctx, int32_t nranks, int32_t rank, const uint8_t id[128]) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return fail(PT_ERR_INVALID_ARG, "bad comm arguments");
    PT_HIP(hipSetDevice(c->device));
    if (c->comm) { ncclCommDestroy(c->comm); c->comm = nullptr; }
    ncclUniqueId uid;
    std::memcpy(&uid, id, 128);
    ncclResult_t r = ncclCommInitRank(&c->comm, nranks, uid, rank);
    if (r != ncclSuccess) return fail(PT_ERR_RCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    c->nranks = nranks;
    c->rank = rank;
    return PT_OK;
}

// ---- the gather's host-side arithmetic (pure functions, exported: hosts and CPU tests check them)
// Where each rank's packed tiles land in the root's receive buffers: rank p (not the root, with
// tiles) at tile offset out_offsets[p] (entries × 1024 pixels; M/V × 3072 doubles), in rank order;
// −1 for the root and for ranks with no tiles.  The counts are one pass' tile lists, which the
// ranks keep disjoint, so they cannot sum past the image's tiles.
int pt_gather_layout(int32_t nranks, int32_t root, const int32_t* counts, int32_t image_tiles,
                     int64_t* out_offsets, int64_t* out_total) {
    if (nranks < 1 || !counts || !out_offsets || !out_total || image_tiles < 0)
        return fail(PT_ERR_INVALID_ARG, "gather layout: bad arguments");
    if (root < 0 || root >= nranks) return fail(PT_ERR_INVALID_ARG, "gather layout: root out of range");
    int64_t sum = 0;
    for (int32_t p = 0; p < nranks; p++) {
        if (counts[p] < 0 || counts[p] > image_tiles)
            return fail(PT_ERR_INVALID_ARG, "gather layout: rank " + std::to_string(p) + " reports " +
                                                std::to_string(counts[p]) + " tiles of " + std::to_string(image_tiles));
        sum += counts[p];
    }
    if (sum > image_tiles)   // disjoint lists never hold more tiles than the image
        return fail(PT_ERR_INVALID_ARG, "gather: the ranks' tile lists overlap (more tiles than the image has)");
    int64_t off = 0;
    for (int32_t p = 0; p < nranks; p++) {
        if (p == root || counts[p] == 0) { out_offsets[p] = -1; continue; }
        out_offsets[p] = off;
        off += counts[p];
    }
    *out_total = off;
    return PT_OK;
}

// Every id in [0, image_tiles) and none twice (a tile on two ranks would be written twice, the
// last sender's copy replacing the others).
int pt_tile_lists_check(const int32_t* ids, int64_t n, int32_t image_tiles) {
    if (n < 0 || (n > 0 && !ids) || image_tiles < 0) return fail(PT_ERR_INVALID_ARG, "tile list: bad arguments");
    std::vector<uint8_t> seen((size_t)image_tiles, 0);
    for (int64_t i = 0; i < n; i++) {
        const int32_t t = ids[i];
        if (t < 0 || t >= image_tiles)
            return fail(PT_ERR_INVALID_ARG, "tile id " + std::to_string(t) + " out of range [0, " +
                                                std::to_string(image_tiles) + ")");
        if (seen[(size_t)t]) return fail(PT_ERR_INVALID_ARG, "tile " + std::to_string(t) + " listed twice");
        seen[(size_t)t] = 1;
    }
    return PT_OK;
}

// Every rank rendered a disjoint tile set into a zero-initialised full-frame
// buffer, so a sum-reduce onto `root` is the gather.
// Tile-compacted gather: every rank but the root packs the {M, V, N} of its
// tiles (the last pass' list) and sends them with the tile ids; the root writes them into
// its Buffer.  The ranks' tiles are disjoint, so this equals a sum-reduce of the full frames
// at ≈1/N of their bytes per rank (1080p, 8 ranks: 13.6 MB instead of 108 MB).  Two steps:
// the tile counts (one all-gather), then the grouped sends and receives.
static int tile_workspace(Ctx* c) {
    const int32_t tiles = ((c->width + 31) / 32) * ((c->height + 31) / 32);
    const size_t slots = (size_t)tiles * 1024u;
    if (!c->g_ids) {
        PT_HIP(hipMalloc(&c->g_ids, (size_t)tiles * sizeof(int32_t)));
        PT_HIP(hipMalloc(&c->g_m, slots * 3 * sizeof(double)));
        PT_HIP(hipMalloc(&c->g_v, slots * 3 * sizeof(double)));
        PT_HIP(hipMalloc(&c->g_n, slots * sizeof(int32_t)));
        PT_HIP(hipMalloc(&c->g_all, (size_t)tiles * sizeof(int32_t)));
        hipLaunchKernelGGL(pt::k_iota, dim3(64), dim3(256), 0, c->stream, c->g_all, tiles);
        PT_HIP(hipGetLastError());
    }
    return PT_OK;
}
static int gather_prepare(Ctx* c) {
    const int32_t tiles = ((c->width + 31) / 32) * ((c->height + 31) / 32);
    int rc = tile_workspace(c);
    if (rc) return rc;
    if (!c->g_cnts) PT_HIP(hipMalloc(&c->g_cnts, (size_t)(c->nranks + 1) * sizeof(int32_t)));
    const int32_t mine = c->pass_tiles > 0 ? c->pass_tiles : tiles;
    PT_HIP(hipMemcpyAsync(c->g_cnts + c->nranks, &mine, sizeof mine, hipMemcpyHostToDevice, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));   // `mine` is a host temporary
    return PT_OK;
}
static const int32_t* own_ids(Ctx* c) { return c->pass_tiles > 0 ? c->d_tiles : c->g_all; }
static int32_t own_count(Ctx* c) {
    return c->pass_tiles > 0 ? c->pass_tiles : ((c->width + 31) / 32) * ((c->height + 31) / 32);
}
// The rank's sends (not root) or receives (root) of step 2; inside a group.  Non-root ranks
// pack first (same stream, so the sends follow the packing).
static ncclResult_t gather_issue(Ctx* c, int32_t root, const std::vector<int32_t>& cnts,
                                 const std::vector<int64_t>& offs) {
    const int tiles_x = (c->width + 31) / 32;
    if (c->rank != root) {
        const int32_t nt = own_count(c);
        if (nt == 0) return ncclSuccess;
        pt::DevBuffer B{c->d_m, c->d_v, c->d_n, c->d_counters};
        hipLaunchKernelGGL(pt::k_tiles_pack, dim3(2048), dim3(256), 0, c->stream, B, c->width, c->height, tiles_x,
                           own_ids(c), (uint32_t)nt, c->g_m, c->g_v, c->g_n, 0);
        if (hipGetLastError() != hipSuccess) return ncclUnhandledCudaError;
        const size_t s = (size_t)nt * 1024u;
        ncclResult_t r = ncclSend(own_ids(c), (size_t)nt, ncclInt32, root, c->comm, c->stream);
        if (r == ncclSuccess) r = ncclSend(c->g_m, s * 3, ncclFloat64, root, c->comm, c->stream);
        if (r == ncclSuccess) r = ncclSend(c->g_v, s * 3, ncclFloat64, root, c->comm, c->stream);
        if (r == ncclSuccess) r = ncclSend(c->g_n, s, ncclInt32, root, c->comm, c->stream);
        return r;
    }
    for (int p = 0; p < c->nranks; p++) {
        if (offs[(size_t)p] < 0) continue;   // the root, or a rank without tiles (pt_gather_layout)
        const size_t off = (size_t)offs[(size_t)p], nt = (size_t)cnts[(size_t)p], s = nt * 1024u;
        ncclResult_t r = ncclRecv(c->g_ids + off, nt, ncclInt32, p, c->comm, c->stream);
        if (r == ncclSuccess) r = ncclRecv(c->g_m + off * 3072u, s * 3, ncclFloat64, p, c->comm, c->stream);
        if (r == ncclSuccess) r = ncclRecv(c->g_v + off * 3072u, s * 3, ncclFloat64, p, c->comm, c->stream);
        if (r == ncclSuccess) r = ncclRecv(c->g_n + off * 1024u, s, ncclInt32, p, c->comm, c->stream);
        if (r != ncclSuccess) return r;
    }
    return ncclSuccess;
}
// The root checks the received tile ids against each other and its own list (a duplicate means
// two ranks rendered one tile: refused before anything is written), then writes them into its Buffer.
static int gather_finish(Ctx* c, int32_t root, int64_t total) {
    if (c->rank == root) {
        if (total > 0) {
            std::vector<int32_t> ids((size_t)total);
            PT_HIP(hipMemcpyAsync(ids.data(), c->g_ids, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            PT_HIP(hipStreamSynchronize(c->stream));
            const int32_t image = ((c->width + 31) / 32) * ((c->height + 31) / 32);
            if (c->pass_tiles > 0) ids.insert(ids.end(), c->h_tiles.begin(), c->h_tiles.end());
            else for (int32_t t = 0; t < image; t++) ids.push_back(t);   // the root rendered the whole image
            if (pt_tile_lists_check(ids.data(), (int64_t)ids.size(), image))
                return fail(PT_ERR_INVALID_ARG, std::string("gather: the ranks' tile lists overlap (") + g_last_error + ")");
            pt::DevBuffer B{c->d_m, c->d_v, c->d_n, c->d_counters};
            hipLaunchKernelGGL(pt::k_tiles_pack, dim3(2048), dim3(256), 0, c->stream, B, c->width, c->height,
                               (c->width + 31) / 32, c->g_ids, (uint32_t)total, c->g_m, c->g_v, c->g_n, 1);
            PT_HIP(hipGetLastError());
        }
        c->gathered = true;
    }
    PT_HIP(hipStreamSynchronize(c->stream));
    return PT_OK;
}
static int gather_counts(Ctx* c, int32_t root, std::vector<int32_t>& cnts, std::vector<int64_t>& offs, int64_t& total) {
    cnts.assign((size_t)c->nranks, 0);
    offs.assign((size_t)c->nranks, -1);
    PT_HIP(hipMemcpy(cnts.data(), c->g_cnts, (size_t)c->nranks * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int32_t tiles = ((c->width + 31) / 32) * ((c->height + 31) / 32);
    return pt_gather_layout(c->nranks, root, cnts.data(), tiles, offs.data(), &total);
}

int pt_comm_gather(void* ctx, int32_t root) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->comm) return fail(PT_ERR_RCCL, "pt_comm_init not called");
    if (root < 0 || root >= c->nranks) return fail(PT_ERR_INVALID_ARG, "root out of range");
    PT_HIP(hipSetDevice(c->device));
    int rc = gather_prepare(c);
    if (rc) return rc;
    ncclResult_t r = ncclAllGather(c->g_cnts + c->nranks, c->g_cnts, 1, ncclInt32, c->comm, c->stream);
    if (r != ncclSuccess) return fail(PT_ERR_RCCL, std::string("ncclAllGather: ") + ncclGetErrorString(r));
    PT_HIP(hipStreamSynchronize(c->stream));
    std::vector<int32_t> cnts;
    std::vector<int64_t> offs;
    int64_t total = 0;
    if ((rc = gather_counts(c, root, cnts, offs, total))) return rc;   // every rank sees the same counts
    r = ncclGroupStart();
    if (r == ncclSuccess) r = gather_issue(c, root, cnts, offs);
    ncclResult_t r2 = ncclGroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess)
        return fail(PT_ERR_RCCL, std::string("gather send/recv: ") + ncclGetErrorString(r != ncclSuccess ? r : r2));
    return gather_finish(c, root, total);
}

// One communicator over G contexts of this process (one per device), formed by one call:
// the single-process multi-GPU form a .NET host uses.
int pt_comm_init_all(void* const* ctxs, int32_t n) {
    if (!ctxs || n < 1) return fail(PT_ERR_INVALID_ARG, "bad context list");
    std::vector<int> devs((size_t)n);
    for (int i = 0; i < n; i++) {
        Ctx* c = (Ctx*)ctxs[i];
        if (!c) return fail(PT_ERR_INVALID_ARG, "NULL context in the list");
        for (int j = 0; j < i; j++)
            if (((Ctx*)ctxs[j])->device == c->device) return fail(PT_ERR_INVALID_ARG, "two contexts on one device");
        devs[(size_t)i] = c->device;
    }
    for (int i = 0; i < n; i++) {
        Ctx* c = (Ctx*)ctxs[i];
        if (c->comm) { ncclCommDestroy(c->comm); c->comm = nullptr; }
    }
    std::vector<ncclComm_t> comms((size_t)n, nullptr);
    ncclResult_t r = ncclCommInitAll(comms.data(), n, devs.data());
    if (r != ncclSuccess) return fail(PT_ERR_RCCL, std::string("ncclCommInitAll: ") + ncclGetErrorString(r));
    for (int i = 0; i < n; i++) {
        Ctx* c = (Ctx*)ctxs[i];
        c->comm = comms[(size_t)i];
        c->nranks = n;
        c->rank = i;
    }
    return PT_OK;
}

// The group's gathers issued from one thread inside one RCCL group (each context's
// reduce on its own stream), then every stream synchronised.
int pt_comm_gather_all(void* const* ctxs, int32_t n, int32_t root) {
    if (!ctxs || n < 1) return fail(PT_ERR_INVALID_ARG, "bad context list");
    if (root < 0 || root >= n) return fail(PT_ERR_INVALID_ARG, "root out of range");
    for (int i = 0; i < n; i++) {
        Ctx* c = (Ctx*)ctxs[i];
        if (!c || !c->comm || c->nranks != n || c->rank != i)
            return fail(PT_ERR_RCCL, "contexts are not the group pt_comm_init_all formed (in that order)");
    }
    int rc;
    for (int i = 0; i < n; i++) {
        Ctx* c = (Ctx*)ctxs[i];
        PT_HIP(hipSetDevice(c->device));
        if ((rc = gather_prepare(c))) return rc;
    }
    ncclResult_t r = ncclGroupStart();   // step 1: the tile counts, every context in one group
    for (int i = 0; i < n && r == ncclSuccess; i++) {
        Ctx* c = (Ctx*)ctxs[i];
        if (hipSetDevice(c->device) != hipSuccess) { r = ncclInvalidUsage; break; }
        r = ncclAllGather(c->g_cnts + c->nranks, c->g_cnts, 1, ncclInt32, c->comm, c->stream);
    }
    ncclResult_t r2 = ncclGroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess)
        return fail(PT_ERR_RCCL, std::string("ncclAllGather (group): ") + ncclGetErrorString(r != ncclSuccess ? r : r2));
    std::vector<std::vector<int32_t>> cnts((size_t)n);
    std::vector<std::vector<int64_t>> offs((size_t)n);
    std::vector<int64_t> total((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        Ctx* c = (Ctx*)ctxs[i];
        PT_HIP(hipSetDevice(c->device));
        PT_HIP(hipStreamSynchronize(c->stream));
        if ((rc = gather_counts(c, root, cnts[(size_t)i], offs[(size_t)i], total[(size_t)i]))) return rc;
    }
    r = ncclGroupStart();   // step 2: the sends and receives
    for (int i = 0; i < n && r == ncclSuccess; i++) {
        Ctx* c = (Ctx*)ctxs[i];
        if (hipSetDevice(c->device) != hipSuccess) { r = ncclInvalidUsage; break; }
        r = gather_issue(c, root, cnts[(size_t)i], offs[(size_t)i]);
    }
    r2 = ncclGroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess)
        return fail(PT_ERR_RCCL, std::string("gather send/recv (group): ") + ncclGetErrorString(r != ncclSuccess ? r : r2));
    for (int i = 0; i < n; i++) {
        Ctx* c = (Ctx*)ctxs[i];
        PT_HIP(hipSetDevice(c->device));
        if ((rc = gather_finish(c, root, total[(size_t)i]))) return rc;
    }
    return PT_OK;
}

int pt_comm_destroy(void* ctx) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx is NULL");
    if (c->comm) { ncclCommDestroy(c->comm); c->comm = nullptr; }
    c->nranks = 1; c->rank = 0;
    return PT_OK;
}

}  // extern "C"
