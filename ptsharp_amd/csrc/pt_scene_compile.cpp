// pt_scene_compile.cpp — scene flattening and BVH builds on the host (pt_scene_compile.h): validation,
// materials and textures, SDF programs, Volume tables, instanced-mesh BLASes, the process-wide triangle
// BVH, the analytic BVH, planes, lights and the routing flags.  Host compiler only; no HIP call.
#include "pt_scene_compile.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <future>
#include <mutex>

#include "pt_bvh.h"
#include "pt_ext.h"
#include "pt_math.h"
#include "pt_shape_refit.h"
#include "pt_stack_key.h"

static_assert(sizeof(float4) == 16, "float4 rows are 16 bytes in host and device objects alike");

#ifndef PT_SDF_LDS_MAX
#define PT_SDF_LDS_MAX 16384   // LDS bytes k_wf_sdf_* may stage the SDF programs in; 0: never
#endif
#ifndef PT_VOL_LDS_MAX
#define PT_VOL_LDS_MAX 40960   // LDS bytes k_wf_vol_* may stage the scene's one Volume in (its uniform-cell table); 0: never
#endif
#ifndef PT_VOL_CELLS_MAX
#define PT_VOL_CELLS_MAX (1ull << 30)   // bytes of cell-major Volume corners (8 per cell) a scene may hold; 0: none
#endif
// Analytic shapes tested linearly by the refill traversal kernels when there are at most this many
// (pt_scene.h ana_linear); 0: always through the analytic BVH.
#ifndef PT_ANA_LINEAR
#define PT_ANA_LINEAR 8
#endif
#ifndef PT_SHADE_ROUTE
#define PT_SHADE_ROUTE 1   // the routed shade (pt_scene.h shade_route); 0: every vertex of a FULL scene through the FULL shade
#endif
#ifndef PT_ROUTE
#define PT_ROUTE 1   // the routed split traversal (pt_scene.h route); 0: every ray through the FULL analytic half
#endif

namespace pt {
namespace {

int fail(std::string& err, int code, const std::string& msg) {
    err = msg;
    return code;
}

inline float4 f4(float x, float y, float z, float w) { return make_float4(x, y, z, w); }
inline float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
inline v3 ld3(const float* p) { return v3{p[0], p[1], p[2]}; }

// Conservative AABB padding for the fp32 slab test (see k_render_pass).
inline void pad_box(float* lo, float* hi) {
    for (int k = 0; k < 3; k++) {
        float m = std::max(std::fabs(lo[k]), std::fabs(hi[k]));
        float e = m * 2.0e-6f + 1e-30f;
        lo[k] = lo[k] - e;
        hi[k] = hi[k] + e;
    }
}

// ---- One source triangle `s` of the scene as device records (pt_scene.h tri_recs / tri_shade / tri_uv) and
// as a padded box: the world BVH's chunks and shading records and the BLASes' arrays all come from these.
inline void pack_tri_geom(const pt_scene_desc* d, int s, float4* r) {
    v3 v1 = ld3(d->tri_v1 + 3 * (size_t)s), v2 = ld3(d->tri_v2 + 3 * (size_t)s), v3_ = ld3(d->tri_v3 + 3 * (size_t)s);
    v3 e1 = sub(v2, v1), e2 = sub(v3_, v1);  // Triangle.cs:97-98
    r[0] = f4(v1.x, v1.y, v1.z, e1.x);
    r[1] = f4(e1.y, e1.z, e2.x, e2.y);
    r[2] = f4(e2.z, 0.f, 0.f, 0.f);
}
inline void pack_tri_shade(const pt_scene_desc* d, int s, float4* r) {
    const float* n1 = d->tri_n1 + 3 * (size_t)s; const float* n2 = d->tri_n2 + 3 * (size_t)s; const float* n3 = d->tri_n3 + 3 * (size_t)s;
    r[0] = f4(n1[0], n1[1], n1[2], n2[0]);
    r[1] = f4(n2[1], n2[2], n3[0], n3[1]);
    r[2] = f4(n3[2], u2f((uint32_t)d->tri_material[s]), 0.f, 0.f);
}
inline void pack_tri_uv(const pt_scene_desc* d, int s, float4* r) {
    const float zero[3] = {0.f, 0.f, 0.f};
    const float* t1 = d->tri_t1 ? d->tri_t1 + 3 * (size_t)s : zero;
    const float* t2 = d->tri_t2 ? d->tri_t2 + 3 * (size_t)s : zero;
    const float* t3 = d->tri_t3 ? d->tri_t3 + 3 * (size_t)s : zero;
    r[0] = f4(t1[0], t1[1], t2[0], t2[1]);
    r[1] = f4(t3[0], t3[1], 0.f, 0.f);
}
inline void tri_padded_box(const pt_scene_desc* d, int s, float* lo, float* hi) {
    for (int k = 0; k < 3; k++) {
        float a = d->tri_v1[3 * (size_t)s + k], b = d->tri_v2[3 * (size_t)s + k], cc = d->tri_v3[3 * (size_t)s + k];
        lo[k] = std::fmin(std::fmin(a, b), cc);
        hi[k] = std::fmax(std::fmax(a, b), cc);
    }
    pad_box(lo, hi);
}

// BVH2 → 4-wide nodes (pt_bvh.h collapse_bvh4) as device float4 rows.  The
// collapse keeps every path's pushes within the kStackMax-entry traversal stack.
// The triangle BVH: a binned-SAH BVH2 with kTriBins bins per axis and leaves of at most 3 triangles
// (one leaf chunk), collapsed to 4-wide nodes by the SAH-optimal dynamic program (pt_bvh.h
// collapse_bvh4_sah, a triangle test priced at kTriCost traversal steps).  Against 32 bins and the
// greedy collapse: C4 nodes per closest-hit ray 8.51 → 8.27, 6025 → 6065 Mrays/s (profiles/r04ab1_*).
// Making SAH's leaf decision always take a full chunk (3 triangles) measured slower.
constexpr int kTriBins = 128;
constexpr double kTriCost = 0.5;
int pack_nodes(const BvhResult& b, std::vector<float4>& out, int32_t& num_nodes, std::string& err, bool sah = false) {
    Bvh4Result r;
    if (sah) collapse_bvh4_sah(b, kStack4Budget, r, 1.0, kTriCost, 3);
    else collapse_bvh4(b, kStack4Budget, r);
    if (r.stack_need > kStack4Budget) return fail(err, PT_ERR_UNSUPPORTED, "BVH4 traversal stack bound exceeded");
    out.resize(r.words.size() / 4);
    if (!r.words.empty()) std::memcpy(out.data(), r.words.data(), r.words.size() * sizeof(uint32_t));
    num_nodes = (int32_t)r.nodes();
    return PT_OK;
}

// ---- The triangle BVH, built once per process for identical geometry (Scene.Compile compiles a scene
// once, Scene.cs:48-68; the reference has one Tree per Scene).  N contexts of one process (the .NET group
// host, bench.py --gpus N) upload the same scene: the first pt_upload_scene builds the BVH (1.1 s at 1M
// triangles on the host), the others wait for that build and upload its bytes.  The key is the triangle
// count, the build parameters and two independent 64-bit hashes of the triangles' vertices in the
// upload's order; the last two builds are kept.
using TriBvhFuture = std::shared_future<std::shared_ptr<const TriBvhBuild>>;
struct TriBvhKey {
    uint64_t n = 0, h1 = 0, h2 = 0;
    bool operator==(const TriBvhKey& o) const { return n == o.n && h1 == o.h1 && h2 == o.h2; }
};
struct TriBvhCache {
    std::mutex mu;
    std::vector<std::pair<TriBvhKey, TriBvhFuture>> entries;
    int64_t builds = 0, hits = 0;
};
TriBvhCache& tri_bvh_cache() {
    static TriBvhCache c;
    return c;
}
// A finished build that no context holds (only the cache's own reference): evictable.  Builds held by live
// contexts and builds in progress are never evicted, so neither a host-only pt_scene_bvh_digest nor another
// scene's upload can push out the build a context of this process would reuse.
bool tri_bvh_evictable(const TriBvhFuture& f) {
    if (f.wait_for(std::chrono::seconds(0)) != std::future_status::ready) return false;
    return f.get().use_count() <= 1;
}
constexpr size_t kTriBvhSpare = 2;   // unreferenced finished builds kept for a later upload of the same geometry
TriBvhKey tri_bvh_key(const pt_scene_desc* d, const std::vector<int32_t>& tri_src) {
    TriBvhKey k;
    k.n = (uint64_t)tri_src.size() ^ ((uint64_t)kTriBins << 40) ^ ((uint64_t)(kTriCost * 1024) << 52);
    uint64_t a = 0x243F6A8885A308D3ull, b = 0x13198A2E03707344ull;
    auto mix = [](uint64_t x) {
        x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
        return x;
    };
    for (int32_t s : tri_src) {
        uint32_t w[9];
        std::memcpy(w, d->tri_v1 + 3 * (size_t)s, 12);
        std::memcpy(w + 3, d->tri_v2 + 3 * (size_t)s, 12);
        std::memcpy(w + 6, d->tri_v3 + 3 * (size_t)s, 12);
        for (int j = 0; j < 9; j++) {
            a = (a ^ w[j]) * 0x100000001B3ull;          // FNV-1a over 32-bit words
            b = mix(b + w[j] + 0x9E3779B97F4A7C15ull);  // a splitmix chain
        }
    }
    k.h1 = a;
    k.h2 = b;
    return k;
}
// Root box = union of the root node's children (their quantized boxes)
void bvh8_root_box(const Bvh8Result& b8, float* box) { tri_root_box(b8.words.data(), box); }
void root_box_of(const uint32_t* w, float* box) {
    for (int ax = 0; ax < 3; ax++) { box[ax] = INFINITY; box[3 + ax] = -INFINITY; }
    for (int k = 0; k < (int)(w[3] >> 28); k++) {
        float lo[3], hi[3];
        bvh8_child_box(w, k, lo, hi);
        for (int ax = 0; ax < 3; ax++) {
            box[ax] = std::min(box[ax], lo[ax]);
            box[3 + ax] = std::max(box[3 + ax], hi[ax]);
        }
    }
}
std::shared_ptr<const TriBvhBuild> build_tri_bvh(const pt_scene_desc* d, const std::vector<int32_t>& tri_src) {
    auto out = std::make_shared<TriBvhBuild>();
    const size_t nt = tri_src.size();
    std::vector<float> bmin(nt * 3), bmax(nt * 3);
    for (size_t i = 0; i < nt; i++) tri_padded_box(d, tri_src[i], &bmin[3 * i], &bmax[3 * i]);
    BvhResult tb;
    build_bvh(bmin.data(), bmax.data(), (int64_t)nt, 0, tb, 3, false, kTriBins);   // leaves fit one chunk
    // 8-wide nodes with quantized child boxes (pt_bvh.h collapse_bvh8q), leaf chunks (one
    // 128-B line per leaf: the first record in word 0, up to three {v1, e1, e2})
    Bvh8Result b8;
    collapse_bvh8q(tb, kStackMax, b8, 1.0, kTriCost, 3);
    if (b8.stack_need > kStackMax) {
        out->rc = fail(out->err, PT_ERR_UNSUPPORTED, "BVH8 traversal stack bound exceeded");
        return out;
    }
    if (b8.chunk_first.size() > 0x1FFFFFFFu) {
        out->rc = fail(out->err, PT_ERR_UNSUPPORTED, "too many triangle leaves");
        return out;
    }
    out->nodes.resize(b8.words.size() / 4);
    if (!b8.words.empty()) std::memcpy(out->nodes.data(), b8.words.data(), b8.words.size() * sizeof(uint32_t));
    out->num_nodes = (int32_t)b8.nodes();
    out->chunks.resize(8 * b8.chunk_first.size());
    for (size_t ci = 0; ci < b8.chunk_first.size(); ci++) {
        float w[32] = {0.f};
        const uint32_t first = b8.chunk_first[ci], cnt = b8.chunk_count[ci];
        const uint32_t w0 = first | ((cnt - 1u) << 29);   // the first record, the count - 1 in bits 29-30
        std::memcpy(&w[0], &w0, 4);
        for (uint32_t t = 0; t < cnt; t++) {
            float4 rec[3];
            pack_tri_geom(d, tri_src[tb.order[first + t]], rec);
            std::memcpy(&w[1 + 9 * t], rec, 9 * sizeof(float));
        }
        std::memcpy(&out->chunks[8 * ci], w, sizeof w);
    }
    if (!out->nodes.empty()) bvh8_root_box(b8, out->box);
    out->order = std::move(tb.order);
    return out;
}

// Box of a light shape as Box.Center / Box.OuterRadius compute it (Box.cs:316-324).
void light_sphere_of_box(v3 mn, v3 mx, DevLight& L) {
    v3 center = add(mn, mul(sub(mx, mn), mk(0.5, 0.5, 0.5)));
    L.center[0] = center.x; L.center[1] = center.y; L.center[2] = center.z;
    L.radius = (double)lengthf(sub(mn, center));
}

// ---- §8f row 4 host side: SDF tree → postfix program, boxes (IShape.BoundingBox)
struct HostBox { v3 mn, mx; };
inline HostBox box_extend(const HostBox& a, const HostBox& b) { return HostBox{vmin(a.mn, b.mn), vmax(a.mx, b.mx)}; }
inline HostBox box_mul(const double* m, const HostBox& b) { HostBox r; mat_box(m, b.mn, b.mx, r.mn, r.mx); return r; }
inline void rows12(const double* m16, double* out) { for (int k = 0; k < 12; k++) out[k] = m16[k]; }

// SDF.BoundingBox per node (SDF.cs:136-139, 191-195, 214-219, 280-284, 313-318, 344-353, 374-382, 413-434, 470-476, 509-530, 555-558)
HostBox sdf_box(const pt_scene_desc* d, int ni) {
    const pt_sdf_node& n = d->sdf_nodes[ni];
    const double* P = n.params;
    switch (n.op) {
        case PT_SDF_SPHERE: { double r = P[0]; return HostBox{mk(-r, -r, -r), mk(r, r, r)}; }
        case PT_SDF_CUBE: {
            double x = (double)(float)P[0] / 2, y = (double)(float)P[1] / 2, z = (double)(float)P[2] / 2;
            return HostBox{mk(-x, -y, -z), mk(x, y, z)};
        }
        case PT_SDF_CYLINDER: { double r = P[0], h = P[1] / 2; return HostBox{mk(-r, -h, -r), mk(r, h, r)}; }
        case PT_SDF_CAPSULE: {
            v3 A = mk(P[0], P[1], P[2]), B = mk(P[3], P[4], P[5]);
            v3 a = vmin(A, B), b = vmax(A, B);
            double r = P[6];   // SubScalar / AddScalar
            return HostBox{mk((double)a.x - r, (double)a.y - r, (double)a.z - r),
                           mk((double)b.x + r, (double)b.y + r, (double)b.z + r)};
        }
        case PT_SDF_TORUS: { double a = P[1], b = P[1] + P[0]; return HostBox{mk(-b, -b, a), mk(b, b, a)}; }
        case PT_SDF_TRANSFORM: return box_mul(n.matrix, sdf_box(d, d->sdf_children[n.first_child]));
        case PT_SDF_SCALE: {
            double f = (double)(float)P[0];   // new Matrix().Scale(new Vector(f, f, f))
            const double m[16] = {f, 0, 0, 0, 0, f, 0, 0, 0, 0, f, 0, 0, 0, 0, 1};
            return box_mul(m, sdf_box(d, d->sdf_children[n.first_child]));
        }
        case PT_SDF_UNION:
        case PT_SDF_INTERSECTION: {
            HostBox r{zero3(), zero3()};
            for (int i = 0; i < n.num_children; i++) {
                HostBox b = sdf_box(d, d->sdf_children[n.first_child + i]);
                r = i == 0 ? b : box_extend(r, b);
            }
            return r;
        }
        case PT_SDF_DIFFERENCE:
            return n.num_children > 0 ? sdf_box(d, d->sdf_children[n.first_child]) : HostBox{zero3(), zero3()};
        default: return HostBox{zero3(), zero3()};   // RepeatSDF: new Box()
    }
}

// Postfix program of an SDF tree (pt_ext.h SdfOp): SDF.Evaluate's recursion unrolled.
struct SdfCompiler {
    const pt_scene_desc* d;
    std::vector<DevSdfIns>& prog;
    std::vector<double>& params;
    int ps = 0, vs = 0, max_ps = 0, max_vs = 0;
    void emit(int op, const double* P, int np) {
        prog.push_back(DevSdfIns{op, (int32_t)params.size()});
        for (int k = 0; k < np; k++) params.push_back(P[k]);
        if (np == 0) params.push_back(0.0);
    }
    void value() { vs++; max_vs = std::max(max_vs, vs); }
    void node(int ni) {
        const pt_sdf_node& n = d->sdf_nodes[ni];
        const double* P = n.params;
        auto child = [&](int k) { return d->sdf_children[n.first_child + k]; };
        switch (n.op) {
            case PT_SDF_SPHERE: emit(SDF_LEAF_SPHERE, P, 2); value(); return;
            case PT_SDF_CUBE: {   // Size is a Vector: its halves are taken from the fp32 values
                const double q[3] = {(double)(float)P[0], (double)(float)P[1], (double)(float)P[2]};
                emit(SDF_LEAF_CUBE, q, 3); value(); return;
            }
            case PT_SDF_CYLINDER: emit(SDF_LEAF_CYLINDER, P, 2); value(); return;
            case PT_SDF_CAPSULE: emit(SDF_LEAF_CAPSULE, P, 8); value(); return;
            case PT_SDF_TORUS: emit(SDF_LEAF_TORUS, P, 4); value(); return;
            case PT_SDF_TRANSFORM:
            case PT_SDF_SCALE:
            case PT_SDF_REPEAT: {
                if (n.op == PT_SDF_TRANSFORM) {
                    double inv[12];
                    rows12(n.inverse, inv);
                    emit(SDF_PUSH_TRANSFORM, inv, 12);
                } else if (n.op == PT_SDF_SCALE) {
                    emit(SDF_PUSH_SCALE, P, 1);
                } else {
                    const double st[3] = {(double)(float)P[0], (double)(float)P[1], (double)(float)P[2]};
                    emit(SDF_PUSH_REPEAT, st, 3);
                }
                ps++;
                max_ps = std::max(max_ps, ps);
                node(child(0));
                emit(SDF_POP_POINT, nullptr, 0);
                ps--;
                if (n.op == PT_SDF_SCALE) emit(SDF_MUL, P, 1);
                return;
            }
            default: {   // Union / Difference / Intersection: fold over the children in order
                const int fold = n.op == PT_SDF_UNION ? SDF_UNION : n.op == PT_SDF_DIFFERENCE ? SDF_DIFFERENCE
                                                                                             : SDF_INTERSECTION;
                if (n.num_children == 0) { emit(SDF_CONST0, nullptr, 0); value(); return; }
                node(child(0));
                for (int k = 1; k < n.num_children; k++) {
                    node(child(k));
                    emit(fold, nullptr, 0);
                    vs--;
                }
            }
        }
    }
};

// A volume view over host data (validation / light registration); the uploader puts device addresses in.
DevVolume dev_volume(const pt_volume& v, const double* data, const DevWindow* windows) {
    DevVolume o{};
    o.data = data; o.windows = windows;
    o.w = v.w; o.h = v.h; o.d = v.d; o.nwin = v.num_windows; o.zscale = v.zscale; o.zinv = vol_zinv(v.zscale);
    for (int k = 0; k < 3; k++) { o.bmin[k] = v.box_min[k]; o.bmax[k] = v.box_max[k]; }
    return o;
}

// Hits of marched shapes can sit just outside their box (SDF: start 1e-4 and a 1e-3 jump back;
// Volume: one step of 1/512 before the box): the BVH boxes are widened by that much.
inline double march_pad(int k) { return k == PT_SHAPE_SDF ? 2e-3 : k == PT_SHAPE_VOLUME ? 4.0 / 512 : 0.0; }

// The state of one compile: the scene, the output, and what one stage leaves for the next.
struct Compiler {
    const pt_scene_desc* d;
    const CompileOptions& opt;
    HostScene& H;
    std::string& err;
    std::vector<int32_t> ana_kind, ana_scene;   // analytic prims (sphere, cube, SDF, volume, transformed)
    std::vector<int32_t> tri_src;               // source triangle index per BVH triangle
    std::vector<int32_t> plane_scene;
    std::vector<HostBox> sdf_boxes, xform_boxes, xform_bvh_boxes;
    std::vector<int32_t> blas_of_mesh;
    std::vector<float> amin, amax;              // the analytic prims' BVH boxes, in gather order
    BvhResult ab;
    std::vector<float4> ana_nodes;
    std::vector<std::vector<int32_t>> ana_pos;  // position in ana_recs of each shape (first occurrence), per kind
    std::vector<int32_t> plane_pos;             // likewise in planes
    const v3 origin = zero3();

    int run();
    void materials_and_textures();
    int gather();
    int sdf_tables();
    void volume_tables();
    int blases();
    void transformed();
    int triangles();
    void ana_boxes();
    int ana_bvh();
    void planes();
    void lights();
    int lines();
    void flags();

    DevVolume host_volume(int i) const {   // Scene.Add's MaterialAt(new Vector()) for light registration
        const HostVolume& v = H.volumes[(size_t)i];
        return dev_volume(d->volumes[i], H.vox.data() + v.vox_off, H.windows.data() + v.win_off);
    }
    HostBox shape_box(int k, int j) const;
    int32_t shape_mat(int k, int j, v3 p) const;
    int32_t shape_mat_any(int k, int j, v3 p) const {   // including TransformedShape.MaterialAt
        if (k == PT_SHAPE_TRANSFORMED) return shape_mat(d->transformed[j].shape_kind, d->transformed[j].shape_index, p);
        return shape_mat(k, j, p);
    }
    void make_rec(int k, int j, int32_t ext_mat, float4* r) const;
};

void Compiler::materials_and_textures() {
    H.mats.resize((size_t)d->num_materials);
    for (int i = 0; i < d->num_materials; i++) {
        pack_material(d->materials[i], H.mats[(size_t)i]);
    }
    H.mats.push_back(DevMaterial{});   // `new Material()` (Volume.MaterialAt's fallback), after the scene's own
    for (auto& m : H.mats.back().color) m = 0.0;
    H.mats.back().tex = H.mats.back().ntex = H.mats.back().btex = H.mats.back().gtex = -1;
    H.S.default_mat = d->num_materials;
    // textures: one fp64 texel array in HBM, DevTexture views into it
    size_t texels = 0;
    for (int i = 0; i < d->num_textures; i++) {
        H.texs.push_back(HostTexture{texels, d->textures[i].width, d->textures[i].height});
        texels += 3 * (size_t)d->textures[i].width * (size_t)d->textures[i].height;
    }
    H.tex_data.resize(texels);
    for (int i = 0; i < d->num_textures; i++)
        std::memcpy(H.tex_data.data() + H.texs[(size_t)i].off, d->textures[i].data,
                    3 * (size_t)d->textures[i].width * (size_t)d->textures[i].height * sizeof(double));
}

// Primitives in Scene.Shapes order
int Compiler::gather() {
    for (int i = 0; i < d->num_shapes; i++) {
        int k = d->shape_kind[i], j = d->shape_index[i];
        if (k == PT_SHAPE_PLANE) plane_scene.push_back(j);
        else if (k != PT_SHAPE_TRIANGLE && k != PT_SHAPE_MESH) { ana_kind.push_back(k); ana_scene.push_back(j); }
    }
    tri_src = gather_tri_src(d);
    if ((int64_t)tri_src.size() >= (int64_t)(1u << 29) || ana_kind.size() >= (1u << 29))
        return fail(err, PT_ERR_UNSUPPORTED, "more than 2^29 primitives");
    return PT_OK;
}

int Compiler::sdf_tables() {
    SdfCompiler sdfc{d, H.sdf_prog, H.sdf_params};
    H.sdf_shapes.resize((size_t)std::max(d->num_sdf_shapes, 0));
    sdf_boxes.resize(H.sdf_shapes.size());
    for (size_t i = 0; i < H.sdf_shapes.size(); i++) {
        DevSdfShape& o = H.sdf_shapes[i];
        o.begin = (int32_t)sdfc.prog.size();
        sdfc.ps = sdfc.vs = 0;
        sdfc.node(d->sdf_shapes[i].root);
        o.len = (int32_t)sdfc.prog.size() - o.begin;
        o.mat = d->sdf_shapes[i].material;
        int leaves = 0, folds = 0;   // a chain: one leaf, no fold (pt_ext.h sdf_eval_chain)
        for (int k = o.begin; k < o.begin + o.len; k++) {
            const int op = sdfc.prog[(size_t)k].op;
            if (op <= SDF_LEAF_TORUS) leaves++;
            if (op == SDF_UNION || op == SDF_DIFFERENCE || op == SDF_INTERSECTION || op == SDF_CONST0) folds++;
        }
        o.chain = (leaves == 1 && folds == 0) ? 1 : 0;
        sdf_boxes[i] = sdf_box(d, d->sdf_shapes[i].root);   // SDFShape.BoundingBox (SDF.cs:100-103)
        o.bmin[0] = sdf_boxes[i].mn.x; o.bmin[1] = sdf_boxes[i].mn.y; o.bmin[2] = sdf_boxes[i].mn.z;
        o.bmax[0] = sdf_boxes[i].mx.x; o.bmax[1] = sdf_boxes[i].mx.y; o.bmax[2] = sdf_boxes[i].mx.z;
    }
    if (sdfc.max_ps + 1 > kSdfStack || sdfc.max_vs > kSdfStack)
        return fail(err, PT_ERR_UNSUPPORTED, "SDF tree nested deeper than the device evaluator's stacks");
    // the SDF programs, staged in LDS by the SDF queue kernels when small (pt_wavefront.hip stage_sdf)
    const size_t need = H.sdf_prog.size() * sizeof(DevSdfIns) + H.sdf_params.size() * sizeof(double);
    H.S.sdf_prog_n = (int32_t)H.sdf_prog.size();
    H.S.sdf_lds = (!H.sdf_prog.empty() && need <= (size_t)PT_SDF_LDS_MAX) ? (int32_t)need : 0;
    return PT_OK;
}

void Compiler::volume_tables() {
    size_t voxels = 0;
    for (int i = 0; i < d->num_volumes; i++) {
        const pt_volume& v = d->volumes[i];
        H.volumes.push_back(HostVolume{dev_volume(v, nullptr, nullptr), voxels, H.windows.size(), 0, -1});
        voxels += (size_t)v.w * v.h * v.d;
        for (int k = 0; k < v.num_windows; k++)
            H.windows.push_back(DevWindow{v.windows[k].lo, v.windows[k].hi, v.windows[k].material, 0});
    }
    H.vox.resize(voxels);
    for (int i = 0; i < d->num_volumes; i++)
        std::memcpy(H.vox.data() + H.volumes[(size_t)i].vox_off, d->volumes[i].data,
                    (size_t)d->volumes[i].w * d->volumes[i].h * d->volumes[i].d * sizeof(double));
    // uniform-cell tables of the march skip (pt_ext.h vol_build_runs), one per volume
    for (int i = 0; i < d->num_volumes; i++) {
        const pt_volume& v = d->volumes[i];
        HostVolume& o = H.volumes[(size_t)i];
        o.runs_off = H.vol_runs.size();
        H.vol_runs.resize(H.vol_runs.size() + (size_t)(v.w + 1) * (v.h + 1) * (v.d + 1));
        vol_build_runs(host_volume(i), H.vol_runs.data() + o.runs_off, o.v.zero_sign);
    }
    // cell-major corners of the march (pt_ext.h vol_build_cells), per volume while they stay within
    // PT_VOL_CELLS_MAX bytes in all; cells_off = -1: the march reads the grid
    for (int i = 0; i < d->num_volumes && opt.vol_cells; i++) {
        const pt_volume& v = d->volumes[i];
        const size_t n = 8 * (size_t)(v.w + 1) * (v.h + 1) * (v.d + 1);
        if ((H.vol_cells.size() + n) * sizeof(double) > (size_t)PT_VOL_CELLS_MAX) continue;
        H.volumes[(size_t)i].cells_off = (int64_t)H.vol_cells.size();
        H.vol_cells.resize(H.vol_cells.size() + n);
        vol_build_cells(host_volume(i), H.vol_cells.data() + H.volumes[(size_t)i].cells_off);
    }
    H.S.vol_lds = 0;
    if (d->num_volumes == 1 && !H.vol_runs.empty() && opt.vol_lds) {   // k_wf_vol_* stage it in LDS (pt_wavefront.hip stage_vol)
        const size_t need = kVolLdsHeader + (((size_t)d->volumes[0].num_windows * sizeof(DevWindow) + 15) & ~(size_t)15) +
                            ((H.vol_runs.size() + 15) & ~(size_t)15);
        if (need <= (size_t)PT_VOL_LDS_MAX) H.S.vol_lds = (int32_t)need;
    }
}

// IShape.BoundingBox of a shape that can be analytic or inner (exact, as the reference computes it)
HostBox Compiler::shape_box(int k, int j) const {
    switch (k) {
        case PT_SHAPE_SPHERE: {
            const float* cc = d->sphere_center + 3 * j;
            double r = d->sphere_radius[j];
            return HostBox{mk((double)cc[0] - r, (double)cc[1] - r, (double)cc[2] - r),
                           mk((double)cc[0] + r, (double)cc[1] + r, (double)cc[2] + r)};
        }
        case PT_SHAPE_CUBE: return HostBox{ld3(d->cube_min + 3 * j), ld3(d->cube_max + 3 * j)};
        case PT_SHAPE_PLANE: return HostBox{mk(-1e9, -1e9, -1e9), mk(1e9, 1e9, 1e9)};
        case PT_SHAPE_SDF: return sdf_boxes[(size_t)j];
        case PT_SHAPE_VOLUME: return HostBox{ld3(d->volumes[j].box_min), ld3(d->volumes[j].box_max)};
        case PT_SHAPE_MESH: {   // Mesh.BoundingBox (Mesh.cs:88-120)
            const int f = d->mesh_first[j], n = d->mesh_count[j];
            if (n <= 0) return HostBox{zero3(), zero3()};
            HostBox b{ld3(d->tri_v1 + 3 * f), ld3(d->tri_v1 + 3 * f)};
            for (int t = f; t < f + n; t++) {
                b.mn = vmin(vmin(vmin(b.mn, ld3(d->tri_v1 + 3 * t)), ld3(d->tri_v2 + 3 * t)), ld3(d->tri_v3 + 3 * t));
                b.mx = vmax(vmax(vmax(b.mx, ld3(d->tri_v1 + 3 * t)), ld3(d->tri_v2 + 3 * t)), ld3(d->tri_v3 + 3 * t));
            }
            return b;
        }
    }
    return HostBox{zero3(), zero3()};
}

// IShape.MaterialAt(p) of an analytic / inner shape
int32_t Compiler::shape_mat(int k, int j, v3 p) const {
    switch (k) {
        case PT_SHAPE_SPHERE: return d->sphere_material[j];
        case PT_SHAPE_CUBE: return d->cube_material[j];
        case PT_SHAPE_PLANE: return d->plane_material[j];
        case PT_SHAPE_SDF: return d->sdf_shapes[j].material;
        case PT_SHAPE_VOLUME: { DevVolume v = host_volume(j); return vol_material(v, p, H.S.default_mat); }
    }
    return H.S.default_mat;
}

// analytic-format record of a shape (top level: ana_recs; inner of a transformed shape: ext_recs)
void Compiler::make_rec(int k, int j, int32_t ext_mat, float4* r) const {
    if (k == PT_SHAPE_SPHERE) {
        const float* cc = d->sphere_center + 3 * j;
        uint64_t rb; double rad = d->sphere_radius[j]; std::memcpy(&rb, &rad, 8);
        r[0] = f4(cc[0], cc[1], cc[2], u2f(KIND_SPHERE));
        r[1] = f4(0.f, 0.f, 0.f, u2f((uint32_t)j));
        r[2] = f4(u2f((uint32_t)d->sphere_material[j]), u2f((uint32_t)(rb & 0xFFFFFFFFu)), u2f((uint32_t)(rb >> 32)), 0.f);
    } else if (k == PT_SHAPE_CUBE) {
        const float* mn = d->cube_min + 3 * j; const float* mx = d->cube_max + 3 * j;
        r[0] = f4(mn[0], mn[1], mn[2], u2f(KIND_CUBE));
        r[1] = f4(mx[0], mx[1], mx[2], u2f((uint32_t)j));
        r[2] = f4(u2f((uint32_t)d->cube_material[j]), 0.f, 0.f, 0.f);
    } else if (k == PT_SHAPE_PLANE) {
        const float* pp = d->plane_point + 3 * j; const float* nn = d->plane_normal + 3 * j;
        r[0] = f4(pp[0], pp[1], pp[2], u2f(KIND_PLANE));
        r[1] = f4(nn[0], nn[1], nn[2], u2f((uint32_t)j));
        r[2] = f4(u2f((uint32_t)d->plane_material[j]), 0.f, 0.f, 0.f);
    } else {   // SDF / volume / transformed: the shape lives in its table, `ext_mat` = MaterialAt(origin)
        const int32_t kind = k == PT_SHAPE_SDF ? KIND_SDF : k == PT_SHAPE_VOLUME ? KIND_VOLUME : KIND_XFORM;
        r[0] = f4(0.f, 0.f, 0.f, u2f((uint32_t)kind));
        r[1] = f4(0.f, 0.f, 0.f, u2f((uint32_t)j));
        r[2] = f4(u2f((uint32_t)ext_mat), u2f((uint32_t)j), 0.f, 0.f);
    }
}

// instanced meshes: one object-space BVH4 per distinct inner mesh (BLAS), records in their own arrays
int Compiler::blases() {
    blas_of_mesh.assign((size_t)std::max(d->num_meshes, 0), -1);
    for (int i = 0; i < d->num_transformed; i++) {
        const pt_transformed_shape& x = d->transformed[i];
        if (x.shape_kind != PT_SHAPE_MESH || blas_of_mesh[(size_t)x.shape_index] >= 0) continue;
        const int f = d->mesh_first[x.shape_index], n = d->mesh_count[x.shape_index];
        std::vector<float> lo((size_t)n * 3), hi((size_t)n * 3);
        for (int t = 0; t < n; t++) tri_padded_box(d, f + t, &lo[3 * (size_t)t], &hi[3 * (size_t)t]);
        BvhResult bb;
        build_bvh(lo.data(), hi.data(), (int64_t)n, 0, bb);
        std::vector<float4> nodes;
        int32_t nn = 0;
        if (int rc = pack_nodes(bb, nodes, nn, err)) return rc;
        DevBlas B{(int32_t)(H.blas_nodes.size() / 8), nn, (int32_t)(H.blas_recs.size() / 3), 0};
        H.blas_nodes.insert(H.blas_nodes.end(), nodes.begin(), nodes.end());
        const size_t r0 = H.blas_recs.size() / 3;
        H.blas_recs.resize(3 * (r0 + (size_t)n));
        H.blas_shade.resize(3 * (r0 + (size_t)n));
        H.blas_uv.resize(2 * (r0 + (size_t)n));
        for (int t = 0; t < n; t++) {
            const int src = f + (int)bb.order[(size_t)t];
            pack_tri_geom(d, src, &H.blas_recs[3 * (r0 + (size_t)t)]);
            pack_tri_shade(d, src, &H.blas_shade[3 * (r0 + (size_t)t)]);
            pack_tri_uv(d, src, &H.blas_uv[2 * (r0 + (size_t)t)]);
            H.blas_refit.src_of_pos.push_back(src);
        }
        const int32_t desc[4] = {B.node_off, B.num_nodes, B.rec_off, n};
        H.blas_refit.desc.insert(H.blas_refit.desc.end(), desc, desc + 4);
        blas_of_mesh[(size_t)x.shape_index] = (int32_t)H.blas.size();
        H.blas.push_back(B);
    }
    // what a later pt_update_meshes needs (BlasRefitTables)
    BlasRefitTables& T = H.blas_refit;
    T.num_nodes = (int64_t)(H.blas_nodes.size() / 8);
    T.num_tris = (int64_t)(H.blas_recs.size() / 3);
    blas_levels((const uint32_t*)H.blas_nodes.data(), T);
    T.xf_blas.assign((size_t)std::max(d->num_transformed, 0), -1);
    for (int i = 0; i < d->num_transformed; i++)
        if (d->transformed[i].shape_kind == PT_SHAPE_MESH) T.xf_blas[(size_t)i] = blas_of_mesh[(size_t)d->transformed[i].shape_index];
    return PT_OK;
}

void Compiler::transformed() {
    H.xforms.resize((size_t)std::max(d->num_transformed, 0));
    H.ext_recs.resize(H.xforms.size() * 3);
    xform_boxes.resize(H.xforms.size());
    xform_bvh_boxes.resize(H.xforms.size());
    for (size_t i = 0; i < H.xforms.size(); i++) {
        const pt_transformed_shape& x = d->transformed[i];
        DevXform& o = H.xforms[i];
        rows12(x.matrix, o.m);
        rows12(x.inverse, o.inv);
        o.kind = x.shape_kind == PT_SHAPE_SDF ? KIND_SDF : x.shape_kind == PT_SHAPE_VOLUME ? KIND_VOLUME
               : x.shape_kind == PT_SHAPE_MESH ? KIND_MESH : x.shape_kind;
        o.rec = x.shape_kind == PT_SHAPE_MESH ? blas_of_mesh[(size_t)x.shape_index] : (int32_t)i;
        if (x.shape_kind != PT_SHAPE_MESH)
            make_rec(x.shape_kind, x.shape_index, shape_mat(x.shape_kind, x.shape_index, origin), &H.ext_recs[3 * i]);
        HostBox ib = shape_box(x.shape_kind, x.shape_index);
        xform_boxes[i] = box_mul(x.matrix, ib);   // TransformedShape.BoundingBox (TransformedShape.cs:36-39)
        const double mp = march_pad(x.shape_kind);
        HostBox pb{mk((double)ib.mn.x - mp, (double)ib.mn.y - mp, (double)ib.mn.z - mp),
                   mk((double)ib.mx.x + mp, (double)ib.mx.y + mp, (double)ib.mx.z + mp)};
        xform_bvh_boxes[i] = box_mul(x.matrix, pb);
    }
    // what a later pt_update_shapes needs (ShapeRefitTables): the inner shapes, and the boxes of those that never move
    ShapeRefitTables& T = H.shape_refit;
    T.num_spheres = std::max(d->num_spheres, 0);
    T.num_cubes = std::max(d->num_cubes, 0);
    T.num_transformed = (int32_t)H.xforms.size();
    T.xf_kind.resize(H.xforms.size());
    T.xf_index.resize(H.xforms.size());
    T.xf_inner_box.assign(H.xforms.size() * 6, 0.f);
    T.xf_matrix.resize(H.xforms.size() * 16);
    T.xf_inverse.resize(H.xforms.size() * 16);
    for (size_t i = 0; i < H.xforms.size(); i++) {
        const pt_transformed_shape& x = d->transformed[i];
        T.xf_kind[i] = H.xforms[i].kind;
        T.xf_index[i] = x.shape_index;
        if (x.shape_kind != PT_SHAPE_SPHERE && x.shape_kind != PT_SHAPE_CUBE) {
            const HostBox ib = shape_box(x.shape_kind, x.shape_index);
            const float b[6] = {ib.mn.x, ib.mn.y, ib.mn.z, ib.mx.x, ib.mx.y, ib.mx.z};
            std::memcpy(&T.xf_inner_box[6 * i], b, sizeof b);
        }
        std::memcpy(&T.xf_matrix[16 * i], x.matrix, 16 * sizeof(double));
        std::memcpy(&T.xf_inverse[16 * i], x.inverse, 16 * sizeof(double));
    }
    if (T.num_spheres > 0) {
        T.sphere_center.assign(d->sphere_center, d->sphere_center + 3 * (size_t)T.num_spheres);
        T.sphere_radius.assign(d->sphere_radius, d->sphere_radius + (size_t)T.num_spheres);
    }
    if (T.num_cubes > 0) {
        T.cube_min.assign(d->cube_min, d->cube_min + 3 * (size_t)T.num_cubes);
        T.cube_max.assign(d->cube_max, d->cube_max + 3 * (size_t)T.num_cubes);
    }
}

// The triangle BVH (built once per process for the same geometry: tri_bvh_shared) and one 128-B shading
// record per triangle (pt_scene.h tri_rstride): what k_wf_shade reads for a triangle hit is one line
// instead of two or three
int Compiler::triangles() {
    const size_t nt = tri_src.size();
    const auto t0 = std::chrono::steady_clock::now();
    const std::shared_ptr<const TriBvhBuild> tbv = tri_bvh_shared(d, tri_src);
    H.tri_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (tbv->rc != PT_OK) return fail(err, tbv->rc, tbv->err);
    H.tri_build = tbv;
    H.tri_uv = d->num_textures > 0 && nt > 0;   // texture coordinates only matter with textures
    H.tri_sh.assign(nt * 8, f4(0.f, 0.f, 0.f, 0.f));
    for (size_t i = 0; i < nt; i++) {
        const int s = tri_src[tbv->order[i]];
        pack_tri_geom(d, s, &H.tri_sh[8 * i]);
        pack_tri_shade(d, s, &H.tri_sh[8 * i + 3]);
        if (H.tri_uv) pack_tri_uv(d, s, &H.tri_sh[8 * i + 6]);
    }
    H.S.tri_rstride = 8;
    H.S.tri_ustride = 8;
    H.S.tri_num_nodes = tbv->num_nodes;
    std::memcpy(H.S.tri_box, tbv->box, sizeof H.S.tri_box);
    // what a later pt_update_triangles needs (RefitTables)
    H.refit.num_triangles = d->num_triangles;
    H.refit.src_of_pos.resize(nt);
    for (size_t i = 0; i < nt; i++) H.refit.src_of_pos[i] = tri_src[tbv->order[i]];
    H.refit.num_nodes = tbv->num_nodes;
    H.refit.num_chunks = (int64_t)(tbv->chunks.size() / 8);
    refit_levels((const uint32_t*)tbv->nodes.data(), tbv->num_nodes, H.refit.level_nodes, H.refit.level_off);
    H.refit.tri_group.assign((size_t)std::max(d->num_triangles, 0), -1);
    H.refit.num_groups = std::max(d->num_meshes, 0);
    for (int j = 0; j < d->num_meshes; j++) {   // only the ranges of meshes in Scene.Shapes were validated: clamp
        const int64_t f = std::max<int64_t>(d->mesh_first[j], 0);
        const int64_t e = std::min<int64_t>((int64_t)d->mesh_first[j] + d->mesh_count[j], (int64_t)H.refit.tri_group.size());
        for (int64_t t = f; t < e; t++) H.refit.tri_group[(size_t)t] = j;
    }
    return PT_OK;
}

// BVH boxes of the analytic prims (spheres, cubes, SDF shapes, volumes, transformed shapes)
void Compiler::ana_boxes() {
    const size_t na = ana_kind.size();
    amin.resize(na * 3);
    amax.resize(na * 3);
    for (size_t i = 0; i < na; i++) {
        int k = ana_kind[i], j = ana_scene[i];
        if (k == PT_SHAPE_SPHERE) {
            double r = d->sphere_radius[j];
            for (int q = 0; q < 3; q++) {
                double cc = d->sphere_center[3 * j + q];
                amin[3 * i + q] = std::nextafter((float)(cc - r), -INFINITY);
                amax[3 * i + q] = std::nextafter((float)(cc + r), INFINITY);
            }
        } else {
            HostBox b = k == PT_SHAPE_TRANSFORMED ? xform_bvh_boxes[(size_t)j] : shape_box(k, j);
            const double mp = k == PT_SHAPE_TRANSFORMED ? 0.0 : march_pad(k);
            const float lo[3] = {b.mn.x, b.mn.y, b.mn.z}, hi[3] = {b.mx.x, b.mx.y, b.mx.z};
            for (int q = 0; q < 3; q++) {
                amin[3 * i + q] = (float)((double)lo[q] - mp);
                amax[3 * i + q] = (float)((double)hi[q] + mp);
            }
        }
        pad_box(&amin[3 * i], &amax[3 * i]);
    }
}

int Compiler::ana_bvh() {
    const size_t na = ana_kind.size();
    ana_boxes();
    build_bvh(amin.data(), amax.data(), (int64_t)na, 0, ab);
    H.ana_recs.resize(na * 3);
    // position in ana_recs of each shape (first occurrence), per kind: Sampler's identity test
    ana_pos.resize(8);
    const int32_t counts[8] = {d->num_spheres, d->num_cubes, 0, 0, 0, d->num_sdf_shapes, d->num_volumes, d->num_transformed};
    for (int k = 0; k < 8; k++) ana_pos[(size_t)k].assign((size_t)std::max(counts[k], 0), -1);
    for (size_t i = 0; i < na; i++) {
        size_t src = ab.order[i];
        int k = ana_kind[src], j = ana_scene[src];
        make_rec(k, j, shape_mat_any(k, j, origin), &H.ana_recs[3 * i]);
        if (ana_pos[(size_t)k][(size_t)j] < 0) ana_pos[(size_t)k][(size_t)j] = (int32_t)i;
    }
    // the row-4 records (SDF shapes, volumes, transformed shapes) with their BVH boxes, in record order:
    // what the routed split's refill kernels test against a ray's segment (pt_scene.h route)
    for (size_t i = 0; i < na; i++) {
        const size_t src = ab.order[i];
        const int k = ana_kind[src];
        if (k != PT_SHAPE_SDF && k != PT_SHAPE_VOLUME && k != PT_SHAPE_TRANSFORMED) continue;
        H.heavy.push_back(f4(amin[3 * src], amin[3 * src + 1], amin[3 * src + 2], u2f((uint32_t)i)));
        H.heavy.push_back(f4(amax[3 * src], amax[3 * src + 1], amax[3 * src + 2], 0.f));
    }
    H.S.ana_count = (int32_t)na;
    H.S.heavy_count = (int32_t)(H.heavy.size() / 2);
    if (int rc = pack_nodes(ab, ana_nodes, H.S.ana_num_nodes, err)) return rc;
    // what a later pt_update_shapes needs (ShapeRefitTables): the records' boxes in record order, the nodes by depth
    ShapeRefitTables& T = H.shape_refit;
    T.num_recs = (int64_t)na;
    T.num_heavy = H.S.heavy_count;
    T.num_nodes = H.S.ana_num_nodes;
    T.rec_box.resize(na * 6);
    for (size_t i = 0; i < na; i++) {
        const size_t src = ab.order[i];
        for (int q = 0; q < 3; q++) { T.rec_box[6 * i + q] = amin[3 * src + q]; T.rec_box[6 * i + 3 + q] = amax[3 * src + q]; }
    }
    shape_levels((const uint32_t*)ana_nodes.data(), T.num_nodes, T.level_nodes, T.level_off);
    return PT_OK;
}

void Compiler::planes() {
    H.planes.resize(plane_scene.size() * 2);
    plane_pos.assign(d->num_planes > 0 ? d->num_planes : 0, -1);
    for (size_t i = 0; i < plane_scene.size(); i++) {
        int j = plane_scene[i];
        const float* p = d->plane_point + 3 * j; const float* n = d->plane_normal + 3 * j;
        H.planes[2 * i] = f4(p[0], p[1], p[2], u2f((uint32_t)d->plane_material[j]));
        H.planes[2 * i + 1] = f4(n[0], n[1], n[2], u2f((uint32_t)j));
        if (plane_pos[(size_t)j] < 0) plane_pos[(size_t)j] = (int32_t)i;
    }
    H.S.num_planes = (int32_t)plane_scene.size();
}

// Scene.Add's light test (Scene.cs:29-38) is look_lights below; this stage states the scene's slots as its tables
void Compiler::lights() {
    LookTables& K = H.look;
    K.slots.reserve((size_t)std::max(d->num_shapes, 0));
    K.fixed_box.assign(6 * (size_t)std::max(d->num_shapes, 0), 0.f);
    for (int i = 0; i < d->num_shapes; i++) {
        const int k = d->shape_kind[i], j = d->shape_index[i];
        LookSlot s{k, j, -1, -1, -1, -1};
        s.mat = k == PT_SHAPE_TRIANGLE ? d->tri_material[j] : k == PT_SHAPE_MESH ? -1 : shape_mat_any(k, j, origin);   // Mesh: `default`
        s.volume = k == PT_SHAPE_VOLUME ? j
                 : (k == PT_SHAPE_TRANSFORMED && d->transformed[j].shape_kind == PT_SHAPE_VOLUME) ? d->transformed[j].shape_index : -1;
        if (k == PT_SHAPE_PLANE) s.pos = plane_pos[(size_t)j];
        else if (k == PT_SHAPE_TRIANGLE) {
            s.vert = (int32_t)K.tri_verts.size();
            for (const float* v : {d->tri_v1, d->tri_v2, d->tri_v3}) K.tri_verts.insert(K.tri_verts.end(), v + 3 * (size_t)j, v + 3 * (size_t)j + 3);
        } else if (k != PT_SHAPE_MESH) s.pos = ana_pos[(size_t)k][(size_t)j];
        if (k == PT_SHAPE_SDF || k == PT_SHAPE_VOLUME) {
            const HostBox b = shape_box(k, j);   // light.BoundingBox()
            const float f[6] = {b.mn.x, b.mn.y, b.mn.z, b.mx.x, b.mx.y, b.mx.z};
            std::memcpy(&K.fixed_box[6 * (size_t)i], f, sizeof f);
        }
        K.slots.push_back(s);
    }
    LookLights L;
    look_lights(K, H.shape_refit, H.mats, L);
    H.lights = std::move(L.lights);
    H.refit.light_tri = std::move(L.light_tri);
    H.shape_refit.light_kind = std::move(L.light_kind);
    H.shape_refit.light_index = std::move(L.light_index);
    H.volume_update.slots = std::move(L.vol_slots);
    H.volume_update.emittance = std::move(L.emittance);
    K.light_slot = std::move(L.light_slot);
    H.S.num_lights = (int32_t)H.lights.size();
}

// the traversal lines: [ana_nodes | tri_nodes | tri_chunks], 8 float4 per node / chunk; the statistics
int Compiler::lines() {
    const std::vector<float4>& tri_nodes = H.tri_build->nodes;
    const std::vector<float4>& tri_chunks = H.tri_build->chunks;
    H.lines.reserve(ana_nodes.size() + tri_nodes.size() + tri_chunks.size());
    H.lines.insert(H.lines.end(), ana_nodes.begin(), ana_nodes.end());
    H.lines.insert(H.lines.end(), tri_nodes.begin(), tri_nodes.end());
    H.lines.insert(H.lines.end(), tri_chunks.begin(), tri_chunks.end());
    if (H.lines.size() >= 0xFFFFFFFFull) return fail(err, PT_ERR_UNSUPPORTED, "more than 2^29 BVH lines");   // 32-bit piece offsets
    H.S.lines_n = (uint32_t)(H.lines.size() / 8);
    H.S.tri_node_line0 = (uint32_t)(ana_nodes.size() / 8);
    H.S.tri_chunk_line0 = (uint32_t)((ana_nodes.size() + tri_nodes.size()) / 8);
    // the stack entries' key field: what the widest triangle-phase index leaves of the 31 bits below the leaf flag
    H.S.stack_key_mask = stack_key_mask(stack_key_choose(tri_nodes.size() / 8, tri_chunks.size() / 8, opt.pop_cull_bits));
    H.bvh_nodes = (uint64_t)H.S.tri_num_nodes + (uint64_t)H.S.ana_num_nodes;
    H.traversal_bytes = (H.lines.size() + H.ana_recs.size()) * sizeof(float4);
    H.bvh_bytes = H.lines.size() * sizeof(float4) + (H.tri_sh.size() + H.ana_recs.size()) * sizeof(float4);
    return PT_OK;
}

void Compiler::flags() {
    DevScene& S = H.S;
    const size_t na = ana_kind.size();
    S.env_tex = d->env_texture - 1;
    S.env_angle = d->env_texture_angle;
    for (int k = 0; k < 3; k++) S.env[k] = d->env_color[k];
    S.num_mats = (int32_t)H.mats.size();
    S.num_sdf = d->num_sdf_shapes;
    S.num_vol = d->num_volumes;
    S.full_geom = (d->num_sdf_shapes > 0 || d->num_volumes > 0 || d->num_transformed > 0) ? 1 : 0;
    S.full = (d->num_textures > 0 || S.full_geom) ? 1 : 0;
    // C4's floor cube and two light spheres: a linear test of 3 records at refill costs less than a BVH
    // node step (seven loads through the texture path) and leaf record loads per ray
    S.ana_linear = (na > 0 && na <= (size_t)PT_ANA_LINEAR && !S.full_geom) ? 1 : 0;
    // Routed split (C5's kind of scene: the 1M-triangle mesh, a floor cube, light spheres, one SDF shape and
    // one transformed Volume): only the rays whose segment reaches a row-4 box take the FULL kernels
    // (CompileOptions::route off: every ray through the FULL analytic half, as a -DPT_ROUTE=0 build;
    // tests compare the two, whose only possible difference is the exact-t tie order of DESIGN.md §5)
    const bool route_on = PT_ROUTE && opt.route;
    H.look.route_geom = route_on && S.full_geom && na <= (size_t)PT_ANA_LINEAR && !H.heavy.empty();
    H.look.shade_full = PT_SHADE_ROUTE && S.full;
    look_flags(H.look, H.lights, H.mats, S.tri_num_nodes, S);
}

// The order of the stages shows in the error a bad scene reports first; each stage's output order
// (Scene.Shapes order, BVH order, first occurrence) shows in the bytes.
int Compiler::run() {
    int rc;
    materials_and_textures();
    if ((rc = gather())) return rc;
    if ((rc = sdf_tables())) return rc;
    volume_tables();
    if ((rc = blases())) return rc;
    transformed();
    if ((rc = triangles())) return rc;
    if ((rc = ana_bvh())) return rc;
    planes();
    lights();
    if ((rc = lines())) return rc;
    flags();
    query_tables(d, H.refit.tri_group, H.query);
    return PT_OK;
}

// The last part of validate_scene: Scene.Shapes itself
int validate_shape_list(const pt_scene_desc* d, std::string& err) {
    for (int i = 0; i < d->num_shapes; i++) {
        int k = d->shape_kind[i], j = d->shape_index[i];
        int lim = k == PT_SHAPE_SPHERE ? d->num_spheres : k == PT_SHAPE_CUBE ? d->num_cubes
                : k == PT_SHAPE_PLANE ? d->num_planes : k == PT_SHAPE_TRIANGLE ? d->num_triangles
                : k == PT_SHAPE_MESH ? d->num_meshes : k == PT_SHAPE_SDF ? d->num_sdf_shapes
                : k == PT_SHAPE_VOLUME ? d->num_volumes : k == PT_SHAPE_TRANSFORMED ? d->num_transformed : -1;
        if (lim < 0) return fail(err, PT_ERR_UNSUPPORTED, "unsupported shape kind " + std::to_string(k));
        if (j < 0 || j >= lim) return fail(err, PT_ERR_INVALID_ARG, "shape index out of range at shape " + std::to_string(i));
        if (k == PT_SHAPE_MESH) {
            int64_t f = d->mesh_first[j], n = d->mesh_count[j];
            if (f < 0 || n < 0 || f + n > d->num_triangles) return fail(err, PT_ERR_INVALID_ARG, "mesh range out of bounds");
        }
    }
    return PT_OK;
}

}  // namespace

void tri_root_box(const uint32_t* root, float box[6]) { root_box_of(root, box); }

void tri_light_sphere(const float* p1, const float* p2, const float* p3, DevLight& L) {
    v3 a = ld3(p1), b = ld3(p2), cc = ld3(p3);
    light_sphere_of_box(vmin(vmin(a, b), cc), vmax(vmax(a, b), cc), L);
}

void sphere_light_sphere(const float* center, double radius, DevLight& L) {
    L.center[0] = center[0]; L.center[1] = center[1]; L.center[2] = center[2];
    L.radius = radius;
}

void box_light_sphere(const float* mn, const float* mx, DevLight& L) { light_sphere_of_box(ld3(mn), ld3(mx), L); }

// The sphere of a light that is sphere j, cube j or transformed shape j of T's current parameters; false for an
// index outside them
static bool shape_light_sphere(const ShapeRefitTables& T, int k, int64_t j, DevLight& L) {
    if (k == PT_SHAPE_SPHERE && j >= 0 && j < T.num_spheres) {
        sphere_light_sphere(&T.sphere_center[3 * (size_t)j], T.sphere_radius[(size_t)j], L);
    } else if (k == PT_SHAPE_CUBE && j >= 0 && j < T.num_cubes) {
        box_light_sphere(&T.cube_min[3 * (size_t)j], &T.cube_max[3 * (size_t)j], L);
    } else if (k == PT_SHAPE_TRANSFORMED && j >= 0 && j < T.num_transformed) {   // light.BoundingBox(): the unpadded box
        const int32_t ik = T.xf_kind[(size_t)j];
        const int64_t ij = T.xf_index[(size_t)j];
        const float* ib = &T.xf_inner_box[6 * (size_t)j];
        v3 imn = ld3(ib), imx = ld3(ib + 3), bmn, bmx;
        if (ik == kShapeSphere && ij >= 0 && ij < T.num_spheres)
            shape_sphere_bounds(&T.sphere_center[3 * (size_t)ij], T.sphere_radius[(size_t)ij], imn, imx);
        else if (ik == kShapeCube && ij >= 0 && ij < T.num_cubes) {
            imn = ld3(&T.cube_min[3 * (size_t)ij]);
            imx = ld3(&T.cube_max[3 * (size_t)ij]);
        }
        float lo[3], hi[3];
        shape_xform_boxes(&T.xf_matrix[16 * (size_t)j], ik, imn, imx, lo, hi, bmn, bmx);
        const float mn[3] = {bmn.x, bmn.y, bmn.z}, mx[3] = {bmx.x, bmx.y, bmx.z};
        box_light_sphere(mn, mx, L);
    } else {
        return false;
    }
    return true;
}

bool shape_refit_lights(const ShapeRefitTables& T, std::vector<DevLight>& lights) {
    bool any = false;
    for (size_t i = 0; i < lights.size() && i < T.light_kind.size(); i++)
        any = shape_light_sphere(T, T.light_kind[i], T.light_index[i], lights[i]) || any;
    return any;
}

void pack_material(const pt_material& m, DevMaterial& o) {
    for (int k = 0; k < 3; k++) o.color[k] = m.color[k];
    o.emittance = m.emittance;
    o.tint = m.tint;
    o.transparent = m.transparent;
    o.index = m.index;
    o.gloss = m.gloss;
    o.reflectivity = m.reflectivity;
    o.tex = m.texture - 1; o.ntex = m.normal_texture - 1; o.btex = m.bump_texture - 1; o.gtex = m.gloss_texture - 1;
    o.bump_multiplier = m.bump_multiplier;
}

// Scene.Add order (Scene.cs:29-38): MaterialAt(new Vector()).Emittance > 0
void look_lights(const LookTables& K, const ShapeRefitTables& T, const std::vector<DevMaterial>& mats, LookLights& out) {
    out = LookLights{};
    const int32_t num_materials = mats.empty() ? 0 : (int32_t)mats.size() - 1;   // the last is `new Material()`
    for (size_t i = 0; i < K.slots.size(); i++) {
        const LookSlot& s = K.slots[i];
        const int k = s.kind, j = s.index, mat = s.mat;
        const bool lit = !(mat < 0 || mat >= num_materials || !(mats[(size_t)mat].emittance > 0));
        // what a later pt_update_volumes tests again with its new windows (VolumeTables)
        if (s.volume >= 0) out.vol_slots.push_back(VolLightSlot{s.volume, lit ? (int32_t)out.lights.size() : -1});
        if (!lit) continue;
        DevLight L{};
        L.kind = k; L.mat = mat; L.phantom = 0; L.index = s.pos;
        if (k == PT_SHAPE_SPHERE) {   // Sampler.cs:218-223
            shape_light_sphere(T, k, j, L);
        } else if (k == PT_SHAPE_PLANE) {
            light_sphere_of_box(mk(-1e9, -1e9, -1e9), mk(1e9, 1e9, 1e9), L);  // Plane.BoundingBox
        } else if (k == PT_SHAPE_TRIANGLE) {  // a directly-added struct Triangle: never passes the identity test
            L.index = -1; L.phantom = 1;
            const float* v = &K.tri_verts[(size_t)s.vert];
            tri_light_sphere(v, v + 3, v + 6, L);
        } else {   // Cube, SDFShape, Volume: class shapes; TransformedShape: a struct, never identical
            L.kind = k == PT_SHAPE_CUBE ? KIND_CUBE : k == PT_SHAPE_SDF ? KIND_SDF : k == PT_SHAPE_VOLUME ? KIND_VOLUME : KIND_XFORM;
            L.phantom = k == PT_SHAPE_TRANSFORMED;
            if (k == PT_SHAPE_SDF || k == PT_SHAPE_VOLUME) box_light_sphere(&K.fixed_box[6 * i], &K.fixed_box[6 * i + 3], L);   // light.BoundingBox()
            else shape_light_sphere(T, k, j, L);
        }
        out.lights.push_back(L);
        out.light_slot.push_back((int32_t)i);
        out.light_tri.push_back(k == PT_SHAPE_TRIANGLE ? j : -1);
        const bool moves = k == PT_SHAPE_SPHERE || k == PT_SHAPE_CUBE || k == PT_SHAPE_TRANSFORMED;
        out.light_kind.push_back(moves ? k : -1);
        out.light_index.push_back(moves ? j : -1);
    }
    out.emittance.resize((size_t)num_materials);
    for (size_t i = 0; i < out.emittance.size(); i++) out.emittance[i] = mats[i].emittance;
}

void look_flags(const LookTables& K, const std::vector<DevLight>& lights, const std::vector<DevMaterial>& mats,
                int32_t tri_num_nodes, DevScene& S) {
    S.lights_lean = 1;
    for (const DevLight& L : lights)
        if (!L.phantom && (L.kind == KIND_SDF || L.kind == KIND_VOLUME || L.kind == KIND_XFORM)) S.lights_lean = 0;
    S.route = (K.route_geom && S.lights_lean && tri_num_nodes > 64) ? 1 : 0;
    bool mat_tex = false;
    for (const auto& m : mats) mat_tex = mat_tex || m.tex >= 0 || m.ntex >= 0 || m.btex >= 0 || m.gtex >= 0;
    S.shade_route = (K.shade_full && !mat_tex && S.lights_lean) ? 1 : 0;   // (a Volume light's colour is FULL work)
}

void shape_levels(const uint32_t* nodes, int64_t num_nodes, std::vector<uint32_t>& level_nodes, std::vector<uint32_t>& level_off) {
    level_nodes.clear();
    level_off.assign(1, 0u);
    if (num_nodes <= 0) return;
    std::vector<uint8_t> seen((size_t)num_nodes, 0);
    level_nodes.push_back(0u);
    seen[0] = 1;
    size_t begin = 0;
    while (begin < level_nodes.size()) {   // one level per round: the children of [begin, end)
        const size_t end = level_nodes.size();
        level_off.push_back((uint32_t)end);
        for (size_t q = begin; q < end; q++) {
            const uint32_t* w = nodes + (size_t)level_nodes[q] * kNode4Words;
            for (int k = 0; k < 4; k++) {
                const uint32_t ref = w[24 + k];
                if (ref == kEmpty4 || (ref & 0x80000000u) || (int64_t)ref >= num_nodes || seen[ref]) continue;
                seen[ref] = 1;
                level_nodes.push_back(ref);
            }
        }
        begin = end;
    }
}

void blas_levels(const uint32_t* nodes, BlasRefitTables& T) {
    T.level_nodes.clear();
    T.level_blas.clear();
    T.level_off.assign(1, 0u);
    std::vector<std::vector<uint32_t>> ln(T.num_blas()), lo(T.num_blas());
    size_t depth = 0;
    for (size_t b = 0; b < T.num_blas(); b++) {
        const int64_t n0 = T.desc[4 * b], nn = T.desc[4 * b + 1];
        if (n0 < 0 || nn < 0 || n0 + nn > T.num_nodes) { lo[b].assign(1, 0u); continue; }
        shape_levels(nodes + (size_t)n0 * kNode4Words, nn, ln[b], lo[b]);
        depth = std::max(depth, lo[b].size() - 1);
    }
    for (size_t l = 0; l < depth; l++) {
        for (size_t b = 0; b < T.num_blas(); b++) {
            if (l + 1 >= lo[b].size()) continue;
            for (uint32_t q = lo[b][l]; q < lo[b][l + 1]; q++) {
                T.level_nodes.push_back(ln[b][q]);
                T.level_blas.push_back((int32_t)b);
            }
        }
        T.level_off.push_back((uint32_t)T.level_nodes.size());
    }
}

void refit_levels(const uint32_t* nodes, int64_t num_nodes, std::vector<uint32_t>& level_nodes, std::vector<uint32_t>& level_off) {
    level_nodes.clear();
    level_off.assign(1, 0u);
    if (num_nodes <= 0) return;
    std::vector<uint32_t> depth((size_t)num_nodes, 0u);
    uint32_t deepest = 0;
    for (int64_t i = 0; i < num_nodes; i++) {
        const uint32_t* w = nodes + i * kNode8Words;
        const uint32_t nin = (w[3] >> 24) & 15u;
        for (uint32_t k = 0; k < nin; k++) {
            const int64_t c = (int64_t)w[4] + k;
            if (c <= i || c >= num_nodes) continue;   // not a tree of this builder: left at depth 0
            depth[(size_t)c] = depth[(size_t)i] + 1;
            deepest = std::max(deepest, depth[(size_t)c]);
        }
    }
    level_off.assign((size_t)deepest + 2, 0u);
    for (int64_t i = 0; i < num_nodes; i++) level_off[depth[(size_t)i] + 1]++;
    for (size_t l = 1; l < level_off.size(); l++) level_off[l] += level_off[l - 1];
    level_nodes.resize((size_t)num_nodes);
    std::vector<uint32_t> at(level_off.begin(), level_off.end() - 1);
    for (int64_t i = 0; i < num_nodes; i++) level_nodes[at[depth[(size_t)i]]++] = (uint32_t)i;
}

// The slot tables of pt_intersect_hits (pt_scene_compile.h QueryTables): one pass over Scene.Shapes for the first slot
// of every shape, then the triangles from the loose slots and the meshes' slots
void query_tables(const pt_scene_desc* d, const std::vector<int32_t>& tri_group, QueryTables& Q) {
    const int32_t counts[8] = {d->num_spheres, d->num_cubes, 0, 0, 0, d->num_sdf_shapes, d->num_volumes, d->num_transformed};
    int32_t at = 0;
    for (int k = 0; k < 8; k++) {
        Q.ana_off[k] = at;
        Q.ana_cnt[k] = std::max(counts[k], 0);
        at += Q.ana_cnt[k];
    }
    Q.ana_slot.assign((size_t)at, -1);
    Q.plane_slot.assign((size_t)std::max(d->num_planes, 0), -1);
    const size_t nt = (size_t)std::max(d->num_triangles, 0), nm = (size_t)std::max(d->num_meshes, 0);
    std::vector<int32_t> loose_slot(nt, -1), mesh_slot(nm, -1);
    for (int i = 0; i < d->num_shapes; i++) {
        const int k = d->shape_kind[i], j = d->shape_index[i];
        int32_t* first = nullptr;
        if (j < 0 || k < 0 || k > 7) continue;
        if (k == PT_SHAPE_PLANE) { if ((size_t)j < Q.plane_slot.size()) first = &Q.plane_slot[(size_t)j]; }
        else if (k == PT_SHAPE_TRIANGLE) { if ((size_t)j < nt) first = &loose_slot[(size_t)j]; }
        else if (k == PT_SHAPE_MESH) { if ((size_t)j < nm) first = &mesh_slot[(size_t)j]; }
        else if (j < Q.ana_cnt[k]) first = &Q.ana_slot[(size_t)(Q.ana_off[k] + j)];
        if (first && *first < 0) *first = i;
    }
    Q.tri_slot = loose_slot;
    std::vector<size_t> slotted;   // the meshes that are top-level shapes
    for (size_t m = 0; m < nm; m++) if (mesh_slot[m] >= 0) slotted.push_back(m);
    for (size_t t = 0; t < nt; t++) {
        if (Q.tri_slot[t] >= 0) continue;
        const int64_t g = t < tri_group.size() ? tri_group[t] : -1;
        if (g >= 0 && (size_t)g < nm && mesh_slot[(size_t)g] >= 0) { Q.tri_slot[t] = mesh_slot[(size_t)g]; continue; }
        int32_t best = -1;   // the mesh tri_group names is in no slot: the first slot of a mesh that holds the triangle
        for (const size_t m : slotted) {
            const int64_t f = d->mesh_first[m], n = d->mesh_count[m];
            if ((int64_t)t >= f && (int64_t)t < f + n && (best < 0 || mesh_slot[m] < best)) best = mesh_slot[m];
        }
        Q.tri_slot[t] = best;
    }
}

std::vector<int32_t> gather_tri_src(const pt_scene_desc* d) {
    std::vector<int32_t> tri_src;
    for (int i = 0; i < d->num_shapes; i++) {
        const int k = d->shape_kind[i], j = d->shape_index[i];
        if (k == PT_SHAPE_TRIANGLE) tri_src.push_back(j);
        else if (k == PT_SHAPE_MESH) for (int t = 0; t < d->mesh_count[j]; t++) tri_src.push_back(d->mesh_first[j] + t);
    }
    return tri_src;
}

std::shared_ptr<const TriBvhBuild> tri_bvh_shared(const pt_scene_desc* d, const std::vector<int32_t>& tri_src) {
    const TriBvhKey key = tri_bvh_key(d, tri_src);
    TriBvhCache& C = tri_bvh_cache();
    std::promise<std::shared_ptr<const TriBvhBuild>> mine;
    TriBvhFuture theirs;
    {
        std::lock_guard<std::mutex> lk(C.mu);
        for (auto& e : C.entries)
            if (e.first == key) { theirs = e.second; break; }
        if (theirs.valid()) {
            C.hits++;
        } else {
            C.builds++;
            C.entries.emplace_back(key, mine.get_future().share());
            // oldest first, only the evictable ones, down to kTriBvhSpare of them
            size_t spare = 0;
            for (auto& e : C.entries) spare += tri_bvh_evictable(e.second) ? 1 : 0;
            for (size_t i = 0; i < C.entries.size() && spare > kTriBvhSpare;) {
                if (tri_bvh_evictable(C.entries[i].second)) {
                    C.entries.erase(C.entries.begin() + (long)i);
                    spare--;
                } else {
                    i++;
                }
            }
        }
    }
    if (theirs.valid()) {
        std::shared_ptr<const TriBvhBuild> r = theirs.get();   // waits while another thread builds it
        if (r->rc == PT_OK) return r;
        return build_tri_bvh(d, tri_src);                        // that build failed: this thread's own error
    }
    std::shared_ptr<const TriBvhBuild> r = build_tri_bvh(d, tri_src);
    mine.set_value(r);
    if (r->rc != PT_OK) {   // a failed build is not kept
        std::lock_guard<std::mutex> lk(C.mu);
        for (size_t i = 0; i < C.entries.size(); i++)
            if (C.entries[i].first == key) { C.entries.erase(C.entries.begin() + (long)i); break; }
    }
    return r;
}

void tri_bvh_release(std::shared_ptr<const TriBvhBuild>& build) {
    if (!build) return;
    TriBvhCache& C = tri_bvh_cache();
    std::lock_guard<std::mutex> lk(C.mu);
    for (size_t i = 0; i < C.entries.size(); i++) {
        auto& f = C.entries[i].second;
        if (f.wait_for(std::chrono::seconds(0)) == std::future_status::ready && f.get() == build &&
            f.get().use_count() <= 2) {   // the cache's reference and this holder's
            C.entries.erase(C.entries.begin() + (long)i);
            break;
        }
    }
    build.reset();
}

TriBvhStats tri_bvh_stats() {
    TriBvhCache& C = tri_bvh_cache();
    std::lock_guard<std::mutex> lk(C.mu);
    return TriBvhStats{C.builds, C.hits, C.entries.size()};
}

int validate_scene(const pt_scene_desc* d, std::string& err) {
    auto bad = [&](int code, const std::string& msg) { return fail(err, code, msg); };
    if (!d) return bad(PT_ERR_INVALID_ARG, "scene is NULL");
    if (d->num_materials <= 0 || !d->materials) return bad(PT_ERR_INVALID_ARG, "scene has no materials");
    if (d->num_shapes < 0 || (d->num_shapes > 0 && (!d->shape_kind || !d->shape_index)))
        return bad(PT_ERR_INVALID_ARG, "shape arrays missing");
    auto chk_mat = [&](const int32_t* m, int n) {
        for (int i = 0; i < n; i++) if (m[i] < 0 || m[i] >= d->num_materials) return false;
        return true;
    };
    if (d->num_spheres > 0 && (!d->sphere_center || !d->sphere_radius || !d->sphere_material ||
                               !chk_mat(d->sphere_material, d->num_spheres)))
        return bad(PT_ERR_INVALID_ARG, "bad sphere arrays");
    if (d->num_cubes > 0 && (!d->cube_min || !d->cube_max || !d->cube_material || !chk_mat(d->cube_material, d->num_cubes)))
        return bad(PT_ERR_INVALID_ARG, "bad cube arrays");
    if (d->num_planes > 0 && (!d->plane_point || !d->plane_normal || !d->plane_material ||
                              !chk_mat(d->plane_material, d->num_planes)))
        return bad(PT_ERR_INVALID_ARG, "bad plane arrays");
    if (d->num_triangles > 0 && (!d->tri_v1 || !d->tri_v2 || !d->tri_v3 || !d->tri_n1 || !d->tri_n2 || !d->tri_n3 ||
                                 !d->tri_material || !chk_mat(d->tri_material, d->num_triangles)))
        return bad(PT_ERR_INVALID_ARG, "bad triangle arrays");
    if (d->num_meshes > 0 && (!d->mesh_first || !d->mesh_count)) return bad(PT_ERR_INVALID_ARG, "bad mesh arrays");
    if (d->num_textures < 0 || (d->num_textures > 0 && !d->textures)) return bad(PT_ERR_INVALID_ARG, "bad texture arrays");
    for (int i = 0; i < d->num_textures; i++) {
        const pt_texture& t = d->textures[i];
        if (t.width < 2 || t.height < 2 || !t.data)   // BilinearSample reads x0 + 1 / y0 + 1 (Texture.cs:198-206)
            return bad(PT_ERR_INVALID_ARG, "texture " + std::to_string(i) + ": needs data and width, height >= 2");
    }
    auto chk_tex = [&](int32_t t) { return t >= 0 && t <= d->num_textures; };
    for (int i = 0; i < d->num_materials; i++) {
        const pt_material& m = d->materials[i];
        if (!chk_tex(m.texture) || !chk_tex(m.normal_texture) || !chk_tex(m.bump_texture) || !chk_tex(m.gloss_texture))
            return bad(PT_ERR_INVALID_ARG, "material " + std::to_string(i) + ": texture reference out of range");
    }
    if (!chk_tex(d->env_texture)) return bad(PT_ERR_INVALID_ARG, "env_texture out of range");
    // §8f row 4
    if (d->num_sdf_nodes < 0 || (d->num_sdf_nodes > 0 && (!d->sdf_nodes || !d->sdf_children)))
        return bad(PT_ERR_INVALID_ARG, "bad SDF node arrays");
    for (int i = 0; i < d->num_sdf_nodes; i++) {
        const pt_sdf_node& n = d->sdf_nodes[i];
        if (n.op < PT_SDF_SPHERE || n.op > PT_SDF_REPEAT) return bad(PT_ERR_INVALID_ARG, "SDF node " + std::to_string(i) + ": bad op");
        const bool one = n.op == PT_SDF_TRANSFORM || n.op == PT_SDF_SCALE || n.op == PT_SDF_REPEAT;
        const bool many = n.op >= PT_SDF_UNION && n.op <= PT_SDF_INTERSECTION;
        if ((one && n.num_children != 1) || (!one && !many && n.num_children != 0) || n.num_children < 0)
            return bad(PT_ERR_INVALID_ARG, "SDF node " + std::to_string(i) + ": wrong number of children");
        for (int k = 0; k < n.num_children; k++) {
            int c = d->sdf_children[n.first_child + k];
            if (c < 0 || c >= i) return bad(PT_ERR_INVALID_ARG, "SDF node " + std::to_string(i) + ": children must precede their parent");
        }
    }
    if (d->num_sdf_shapes < 0 || (d->num_sdf_shapes > 0 && !d->sdf_shapes)) return bad(PT_ERR_INVALID_ARG, "bad SDF shapes");
    for (int i = 0; i < d->num_sdf_shapes; i++)
        if (d->sdf_shapes[i].root < 0 || d->sdf_shapes[i].root >= d->num_sdf_nodes ||
            d->sdf_shapes[i].material < 0 || d->sdf_shapes[i].material >= d->num_materials)
            return bad(PT_ERR_INVALID_ARG, "SDF shape " + std::to_string(i) + ": bad root or material");
    if (d->num_volumes < 0 || (d->num_volumes > 0 && !d->volumes)) return bad(PT_ERR_INVALID_ARG, "bad volumes");
    for (int i = 0; i < d->num_volumes; i++) {
        const pt_volume& v = d->volumes[i];
        if (v.w < 1 || v.h < 1 || v.d < 1 || !v.data || v.num_windows < 0 || (v.num_windows > 0 && !v.windows))
            return bad(PT_ERR_INVALID_ARG, "volume " + std::to_string(i) + ": bad grid or windows");
        for (int k = 0; k < v.num_windows; k++)
            if (v.windows[k].material < 0 || v.windows[k].material >= d->num_materials)
                return bad(PT_ERR_INVALID_ARG, "volume " + std::to_string(i) + ": window material out of range");
    }
    if (d->num_transformed < 0 || (d->num_transformed > 0 && !d->transformed)) return bad(PT_ERR_INVALID_ARG, "bad transformed shapes");
    for (int i = 0; i < d->num_transformed; i++) {
        const pt_transformed_shape& x = d->transformed[i];
        int lim = x.shape_kind == PT_SHAPE_SPHERE ? d->num_spheres : x.shape_kind == PT_SHAPE_CUBE ? d->num_cubes
                : x.shape_kind == PT_SHAPE_PLANE ? d->num_planes : x.shape_kind == PT_SHAPE_SDF ? d->num_sdf_shapes
                : x.shape_kind == PT_SHAPE_VOLUME ? d->num_volumes : x.shape_kind == PT_SHAPE_MESH ? d->num_meshes : -1;
        if (lim < 0) return bad(PT_ERR_UNSUPPORTED, "transformed shape " + std::to_string(i) + ": inner kind not on the GPU path");
        if (x.shape_index < 0 || x.shape_index >= lim) return bad(PT_ERR_INVALID_ARG, "transformed shape " + std::to_string(i) + ": inner index out of range");
    }
    if (d->num_triangles > 0 && ((d->tri_t1 != nullptr) != (d->tri_t2 != nullptr) || (d->tri_t1 != nullptr) != (d->tri_t3 != nullptr)))
        return bad(PT_ERR_INVALID_ARG, "tri_t1/t2/t3 must be all set or all NULL");
    return validate_shape_list(d, err);
}

int compile_scene(const pt_scene_desc* d, const CompileOptions& opt, HostScene& H, std::string& err) {
    if (int rc = validate_scene(d, err)) return rc;
    H = HostScene{};
    return Compiler{d, opt, H, err}.run();
}

}  // namespace pt
