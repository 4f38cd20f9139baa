// pt_scene_compile.h — host-only scene compilation: a pt_scene_desc turned into the bytes pt_upload_scene
// copies to the device (replacing Scene.Compile / Tree.NewTree, Scene.cs:48-68).  Nothing here touches the
// GPU: pt_scene_compile.cpp is built by the host compiler, pt_api.hip uploads a HostScene's arrays and
// derives the DevScene's pointer fields from their device addresses.
#pragma once
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/ptsharp_hip.h"
#include "pt_scene.h"

namespace pt {

// What pt_upload_scene reads from the environment at each upload (tests flip them between uploads);
// the compile itself reads no environment.
struct CompileOptions {
    bool vol_cells = true;   // PT_VOL_CELLS=0: no cell-major Volume corners, the march reads the grid
    bool vol_lds = true;     // PT_VOL_LDS=0: the scene's one Volume is not staged in LDS
    bool route = true;       // PT_ROUTE=0: every ray through the FULL analytic half
    int pop_cull_bits = 15;  // PT_POP_CULL=0: 0 (bare stack entries); PT_POP_CULL_BITS=n: at most n key bits
};

// The triangle BVH of one geometry, shared by every context of the process that uploads it (tri_bvh_shared).
struct TriBvhBuild {
    std::vector<uint32_t> order;      // BVH position -> index into tri_src
    std::vector<float4> nodes, chunks;
    int32_t num_nodes = 0;
    float box[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int rc = PT_OK;
    std::string err;
};

struct HostTexture {
    size_t off;   // first texel component in tex_data
    int32_t w, h;
};
struct HostVolume {
    DevVolume v;   // every field but the pointers (data, windows, runs, cells), which are the offsets below
    size_t vox_off, win_off, runs_off;   // into vox, windows, vol_runs
    int64_t cells_off;                   // into vol_cells; -1: the march reads the grid
};

// What pt_update_triangles needs beside the device arrays: small host tables kept from the upload.
struct RefitTables {
    int32_t num_triangles = 0;          // pt_scene_desc::num_triangles: the length of the arrays an update takes
    std::vector<int32_t> src_of_pos;    // source triangle of BVH position i: tri_src[order[i]]
    std::vector<uint32_t> level_nodes;  // the triangle BVH's node indices grouped by depth, the root's level first
    std::vector<uint32_t> level_off;    // level l is level_nodes[level_off[l] .. level_off[l + 1])
    std::vector<int32_t> light_tri;     // per HostScene::lights entry: its source triangle, or -1 (not a loose triangle)
    int64_t num_nodes = 0, num_chunks = 0;
    // pt_update_triangles_normals: the mesh (index into mesh_first / mesh_count) of every source triangle, -1 for
    // one outside every mesh (a loose triangle); a triangle inside several ranges takes the last of them
    std::vector<int32_t> tri_group;
    int32_t num_groups = 0;             // pt_scene_desc::num_meshes
};
// The nodes of an 8-wide BVH (kNode8Words words each) grouped by depth.  A child's index is greater than its
// parent's (pt_bvh.cpp Wide8::emit allocates children after their parent), so one forward sweep gives the depths.
void refit_levels(const uint32_t* nodes, int64_t num_nodes, std::vector<uint32_t>& level_nodes, std::vector<uint32_t>& level_off);
// The box of the triangle BVH from its root node's 32 words, as the compile computes DevScene::tri_box.
void tri_root_box(const uint32_t* root, float box[6]);
// Centre and radius of a loose emissive triangle's light, as the compile's light stage computes them.
void tri_light_sphere(const float* p1, const float* p2, const float* p3, DevLight& L);

// What pt_update_shapes needs beside the device arrays: host tables kept from the upload, and the
// parameters the device holds now (a group an update does not give is refitted from these).
struct ShapeRefitTables {
    int32_t num_spheres = 0, num_cubes = 0, num_transformed = 0;   // pt_scene_desc's counts: the lengths an update takes
    int64_t num_nodes = 0, num_recs = 0, num_heavy = 0;            // analytic BVH4 nodes, analytic records, heavy records
    std::vector<uint32_t> level_nodes;   // the BVH4's node indices grouped by depth, the root's level first
    std::vector<uint32_t> level_off;     // level l is level_nodes[level_off[l] .. level_off[l + 1])
    std::vector<int32_t> xf_kind, xf_index;   // per transformed shape: its inner shape (kind as DevXform::kind)
    std::vector<float> xf_inner_box;     // per transformed shape: 6 floats, the inner box before march_pad of the kinds
                                         // that never move (SDF, Volume, Mesh, Plane); zeros for a sphere or cube
    std::vector<float> rec_box;          // per analytic record: 6 floats, its BVH box at the upload
    std::vector<int32_t> light_kind, light_index;   // per HostScene::lights entry: its source (PT_SHAPE_SPHERE, _CUBE or
                                                    // _TRANSFORMED and the scene index), or -1 (a light no update moves)
    std::vector<float> sphere_center, cube_min, cube_max;   // the current parameters, in pt_scene_desc order
    std::vector<double> sphere_radius, xf_matrix, xf_inverse;   // matrices [num_transformed][16] row-major
};
// The nodes of a BVH4 (kNode4Words words each) grouped by depth: a breadth-first walk from node 0 over words 24-27.
void shape_levels(const uint32_t* nodes, int64_t num_nodes, std::vector<uint32_t>& level_nodes, std::vector<uint32_t>& level_off);
// Centre and radius of a sphere light (Sampler.cs:218-223) and of a light with a bounding box (Box.Center,
// Box.OuterRadius), as the compile's light stage computes them.
void sphere_light_sphere(const float* center, double radius, DevLight& L);
void box_light_sphere(const float* mn, const float* mx, DevLight& L);
// The lights that follow T's current parameters, recomputed in place (lights: HostScene::lights' order); true
// when the scene has one.
bool shape_refit_lights(const ShapeRefitTables& T, std::vector<DevLight>& lights);

// What pt_update_meshes needs beside the device arrays to refit the BLASes of instanced meshes: host
// tables kept from the upload.
struct BlasRefitTables {
    int64_t num_nodes = 0, num_tris = 0;   // BLAS nodes and BLAS triangle positions in total
    std::vector<int32_t> desc;          // per BLAS four int32 (pt_blas_refit.h BlasDesc): node_off, num_nodes, rec_off, num_tris
    std::vector<int32_t> src_of_pos;    // source triangle of BLAS triangle position i: mesh_first + order[i - rec_off]
    std::vector<uint32_t> level_nodes;  // every BLAS's node indices (relative to its node_off) grouped by depth over all
    std::vector<int32_t> level_blas;    // BLASes, the roots' level first; per entry its BLAS
    std::vector<uint32_t> level_off;    // level l is entries [level_off[l], level_off[l + 1])
    std::vector<int32_t> xf_blas;       // per transformed shape: the BLAS of its mesh, or -1
    size_t num_blas() const { return desc.size() / 4; }
};
// Fills T.level_* from the BLASes' nodes (kNode4Words words each, all BLASes back to back) and T.desc: shape_levels'
// breadth-first walk from each BLAS's node 0.
void blas_levels(const uint32_t* nodes, BlasRefitTables& T);

// What pt_intersect_hits needs beside the device arrays to say which Scene.Shapes slot a hit belongs to (DESIGN.md
// §4h): -1 for a shape in no slot; where several slots name one shape, the first.
struct QueryTables {
    // per source triangle (pt_scene_desc order): the first PT_SHAPE_TRIANGLE slot that names it; else the first slot
    // of the mesh tri_group assigns it to; else the first PT_SHAPE_MESH slot whose range holds it
    std::vector<int32_t> tri_slot;
    // per analytic shape, the kinds one after another in pt_shape_kind order: entry ana_off[k] + j is shape j of kind k
    // (ana_cnt[k] of them; planes, triangles and meshes have none here)
    std::vector<int32_t> ana_slot;
    int32_t ana_off[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ana_cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<int32_t> plane_slot;   // per plane (pt_scene_desc order)
};
// tri_group: RefitTables::tri_group of the same scene.  Indices out of range are skipped (the compile validated the
// shapes it uses; this reads nothing else).
void query_tables(const pt_scene_desc* d, const std::vector<int32_t>& tri_group, QueryTables& Q);

// What pt_update_volumes needs beside the device arrays: the light test's inputs.  (The volumes'
// headers and window rows are HostScene::volumes and ::windows; the context keeps copies of those, never the grid.)
struct VolumeTables {
    std::vector<VolLightSlot> slots;   // every Scene.Shapes slot that is a Volume or a TransformedShape over one, and the
                                       // HostScene::lights entry it registered (-1: none)
    std::vector<double> emittance;     // per material of the scene (pt_scene_desc order)
};

// What pt_update_materials needs beside the device arrays: Scene.Add's light test (Scene.cs:29-38)
// over tables instead of a pt_scene_desc, so that the upload and a later material edit run one derivation.
struct LookSlot {
    int32_t kind, index;   // Scene.Shapes slot: pt_shape_kind and the index of that kind
    int32_t mat;           // MaterialAt(new Vector()) as an index (a Mesh: -1, `default`; a Volume's follows its windows)
    int32_t pos;           // DevLight::index if the slot is a light: its position in ana_recs or planes; else -1
    int32_t vert;          // a loose triangle: its first float in LookTables::tri_verts; else -1
    int32_t volume;        // a Volume, or a TransformedShape over one: that volume; else -1
};
struct LookTables {
    std::vector<LookSlot> slots;    // Scene.Shapes order
    std::vector<float> fixed_box;   // per slot 6 floats: BoundingBox of an SDF shape or a Volume (no update moves it)
    std::vector<float> tri_verts;   // 9 floats per PT_SHAPE_TRIANGLE slot: v1, v2, v3 as the device holds them now
    std::vector<int32_t> light_slot;   // per entry of the current lights: its slot (LookLights::light_slot, kept here)
    // the parts of DevScene::route and ::shade_route that no material decides (pt_scene_compile.cpp look_flags)
    bool route_geom = false, shade_full = false;
};
void pack_material(const pt_material& m, DevMaterial& o);
// The lights of the scene whose materials are `mats` (the scene's own, then `new Material()`), in Scene.Shapes order,
// with the tables that name each light's source: RefitTables::light_tri, ShapeRefitTables::light_kind and
// ::light_index, VolumeTables::slots and ::emittance.  A light's sphere comes from where its shape is now: T's current
// parameters, K.tri_verts, K.fixed_box.
struct LookLights {
    std::vector<DevLight> lights;
    std::vector<int32_t> light_tri, light_kind, light_index;
    std::vector<int32_t> light_slot;   // per light: the Scene.Shapes slot that registered it
    std::vector<VolLightSlot> vol_slots;
    std::vector<double> emittance;
};
void look_lights(const LookTables& K, const ShapeRefitTables& T, const std::vector<DevMaterial>& mats, LookLights& out);
// DevScene::lights_lean, ::route and ::shade_route from those lights and materials; tri_num_nodes: the triangle
// BVH's node count now.
void look_flags(const LookTables& K, const std::vector<DevLight>& lights, const std::vector<DevMaterial>& mats,
                int32_t tri_num_nodes, DevScene& S);

// A compiled scene on the host: every array pt_upload_scene uploads, and the DevScene with every
// non-pointer field filled.
struct HostScene {
    std::vector<float4> lines;   // [ana nodes | tri nodes | tri chunks], 8 float4 per line (S.tri_node_line0, S.tri_chunk_line0)
    std::vector<float4> tri_sh;  // one 128-B shading record per triangle: recs at +0, shade at +3, uv at +6
    bool tri_uv = false;         // tri_sh carries texture coordinates (a scene with textures and triangles)
    std::vector<float4> ana_recs, planes, heavy;
    std::vector<DevMaterial> mats;   // the scene's, then `new Material()` (S.default_mat)
    std::vector<DevLight> lights;
    std::vector<double> tex_data;
    std::vector<HostTexture> texs;
    std::vector<DevSdfIns> sdf_prog;
    std::vector<double> sdf_params;
    std::vector<DevSdfShape> sdf_shapes;
    std::vector<double> vox;
    std::vector<DevWindow> windows;
    std::vector<int8_t> vol_runs;
    std::vector<double> vol_cells;
    std::vector<HostVolume> volumes;
    std::vector<DevXform> xforms;
    std::vector<float4> ext_recs;
    std::vector<DevBlas> blas;
    std::vector<float4> blas_nodes, blas_recs, blas_shade, blas_uv;
    DevScene S{};
    uint64_t bvh_nodes = 0, traversal_bytes = 0, bvh_bytes = 0;   // pt_stats
    std::shared_ptr<const TriBvhBuild> tri_build;   // the shared triangle build `lines` was filled from
    double tri_build_ms = 0;                        // host time to build (or wait for, or find) it
    RefitTables refit;
    ShapeRefitTables shape_refit;
    BlasRefitTables blas_refit;
    QueryTables query;
    VolumeTables volume_update;
    LookTables look;
};

// Validates and compiles.  PT_OK, or an error code with its message in err (H is then partly filled; its
// tri_build is set once the triangle BVH was found or built).
int compile_scene(const pt_scene_desc* d, const CompileOptions& opt, HostScene& H, std::string& err);

int validate_scene(const pt_scene_desc* d, std::string& err);
// Source triangle of every triangle of the world BVH, in Scene.Shapes order (loose triangles and top-level meshes).
std::vector<int32_t> gather_tri_src(const pt_scene_desc* d);

// The build for this geometry: the cached one, one in progress on another thread (waited for), or a new one.
std::shared_ptr<const TriBvhBuild> tri_bvh_shared(const pt_scene_desc* d, const std::vector<int32_t>& tri_src);
// A holder lets go of its build (next upload, pt_destroy): the last holder of a geometry takes its cache entry
// along, so the host memory (tens of MB at 1M triangles) lives as long as a context uses it.
void tri_bvh_release(std::shared_ptr<const TriBvhBuild>& build);
struct TriBvhStats {
    int64_t builds, hits;   // since the process started
    size_t entries;         // builds the cache holds now
};
TriBvhStats tri_bvh_stats();

}  // namespace pt
