// scene_compile_check.cpp — the host-only scene compile (ptsharp_amd/csrc/pt_scene_compile.cpp) on scenes built
// in C++ (scene_fixture.h), checked from first principles: the layout of the traversal lines, every triangle once
// in the BVH order and once in the leaf chunks, record kinds and indices, the shared BLAS, the light list, the
// heavy records, every routing flag against its defining expression, the three CompileOptions, the error cases
// with their codes, and determinism.  `--digest [fixed|fixed1|big] [cells0|lds0|route0]` prints a 64-bit FNV-1a
// per array and the scalar DevScene fields instead (for comparing two builds of the library's compile).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ptsharp_amd/csrc/pt_bvh.h"
#include "../../ptsharp_amd/csrc/pt_scene_compile.h"
#include "scene_fixture.h"

static int failures = 0;
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
            failures++;                                                           \
        }                                                                         \
    } while (0)

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// ---- digests: every array as bytes; textures and volumes as their offsets and scalar fields
struct TexRow { int64_t off; int32_t w, h; };
struct VolRow {
    int64_t vox_off, win_off, runs_off, cells_off;
    int32_t w, h, d, nwin;
    double zscale, zinv;
    float bmin[3], bmax[3];
    int32_t zero_sign, pad;
};
static uint64_t fnv(const void* p, size_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    const unsigned char* q = (const unsigned char*)p;
    for (size_t i = 0; i < n; i++) h = (h ^ q[i]) * 0x100000001B3ull;
    return h;
}
template <class T>
static void row(std::vector<std::string>& out, const char* name, const std::vector<T>& v) {
    char b[128];
    std::snprintf(b, sizeof b, "%-12s %016llx %zu", name, (unsigned long long)fnv(v.data(), v.size() * sizeof(T)), v.size() * sizeof(T));
    out.push_back(b);
}
static std::vector<std::string> digest(const pt::HostScene& H) {
    std::vector<std::string> o;
    std::vector<TexRow> texs;
    for (const pt::HostTexture& t : H.texs) texs.push_back(TexRow{(int64_t)t.off, t.w, t.h});
    std::vector<VolRow> vols;
    for (const pt::HostVolume& v : H.volumes) {
        VolRow r;
        std::memset(&r, 0, sizeof r);
        r.vox_off = (int64_t)v.vox_off; r.win_off = (int64_t)v.win_off; r.runs_off = (int64_t)v.runs_off; r.cells_off = v.cells_off;
        r.w = v.v.w; r.h = v.v.h; r.d = v.v.d; r.nwin = v.v.nwin; r.zscale = v.v.zscale; r.zinv = v.v.zinv;
        for (int k = 0; k < 3; k++) { r.bmin[k] = v.v.bmin[k]; r.bmax[k] = v.v.bmax[k]; }
        r.zero_sign = v.v.zero_sign;
        vols.push_back(r);
    }
    row(o, "lines", H.lines); row(o, "tri_sh", H.tri_sh); row(o, "ana_recs", H.ana_recs); row(o, "planes", H.planes);
    row(o, "mats", H.mats); row(o, "lights", H.lights); row(o, "tex_data", H.tex_data); row(o, "texs", texs);
    row(o, "sdf_prog", H.sdf_prog); row(o, "sdf_params", H.sdf_params); row(o, "sdf_shapes", H.sdf_shapes);
    row(o, "vox", H.vox); row(o, "windows", H.windows); row(o, "vol_runs", H.vol_runs); row(o, "vol_cells", H.vol_cells);
    row(o, "volumes", vols); row(o, "xforms", H.xforms); row(o, "ext_recs", H.ext_recs); row(o, "blas", H.blas);
    row(o, "blas_nodes", H.blas_nodes); row(o, "blas_recs", H.blas_recs); row(o, "blas_shade", H.blas_shade);
    row(o, "blas_uv", H.blas_uv); row(o, "heavy", H.heavy);
    const pt::DevScene& S = H.S;
    char b[512];
    std::snprintf(b, sizeof b, "nodes tri %d ana %d lines %u %u %u tri_box %08x %08x %08x %08x %08x %08x", S.tri_num_nodes,
                  S.ana_num_nodes, S.tri_node_line0, S.tri_chunk_line0, S.lines_n, bits(S.tri_box[0]), bits(S.tri_box[1]),
                  bits(S.tri_box[2]), bits(S.tri_box[3]), bits(S.tri_box[4]), bits(S.tri_box[5]));
    o.push_back(b);
    std::snprintf(b, sizeof b, "counts planes %d lights %d mats %d ana %d sdf %d vol %d heavy %d sdf_prog %d uv %d strides %d %d",
                  S.num_planes, S.num_lights, S.num_mats, S.ana_count, S.num_sdf, S.num_vol, S.heavy_count, S.sdf_prog_n,
                  (int)H.tri_uv, S.tri_rstride, S.tri_ustride);
    o.push_back(b);
    std::snprintf(b, sizeof b, "flags full %d full_geom %d ana_linear %d lights_lean %d route %d shade_route %d sdf_lds %d vol_lds %d default_mat %d",
                  S.full, S.full_geom, S.ana_linear, S.lights_lean, S.route, S.shade_route, S.sdf_lds, S.vol_lds, S.default_mat);
    o.push_back(b);
    std::snprintf(b, sizeof b, "env %a %a %a tex %d angle %a", S.env[0], S.env[1], S.env[2], S.env_tex, S.env_angle);
    o.push_back(b);
    std::snprintf(b, sizeof b, "stats bvh_nodes %llu traversal_bytes %llu bvh_bytes %llu", (unsigned long long)H.bvh_nodes,
                  (unsigned long long)H.traversal_bytes, (unsigned long long)H.bvh_bytes);
    o.push_back(b);
    return o;
}

static int compile(const FixScene& s, pt::HostScene& H, const pt::CompileOptions& opt = pt::CompileOptions{}) {
    std::string err;
    const int rc = pt::compile_scene(&s.d, opt, H, err);
    if (rc != PT_OK) std::fprintf(stderr, "compile_scene: %d %s\n", rc, err.c_str());
    return rc;
}

// ---- the traversal lines and the triangle records
static void check_lines_and_triangles(const FixScene& s, const pt::HostScene& H) {
    const pt::DevScene& S = H.S;
    const std::vector<int32_t> src = pt::gather_tri_src(&s.d);
    const size_t nt = src.size();
    CHECK(H.lines.size() == 8 * (size_t)S.lines_n);
    CHECK(S.tri_node_line0 == (uint32_t)S.ana_num_nodes);
    CHECK(S.tri_chunk_line0 == S.tri_node_line0 + (uint32_t)S.tri_num_nodes);
    CHECK(S.tri_chunk_line0 <= S.lines_n);
    CHECK(H.tri_build && H.tri_build->nodes.size() == 8 * (size_t)S.tri_num_nodes);
    CHECK(H.tri_build->chunks.size() == 8 * (size_t)(S.lines_n - S.tri_chunk_line0));
    CHECK(!std::memcmp(H.lines.data() + 8 * (size_t)S.tri_node_line0, H.tri_build->nodes.data(), H.tri_build->nodes.size() * sizeof(float4)));
    CHECK(!std::memcmp(H.lines.data() + 8 * (size_t)S.tri_chunk_line0, H.tri_build->chunks.data(), H.tri_build->chunks.size() * sizeof(float4)));
    CHECK(H.bvh_nodes == (uint64_t)S.tri_num_nodes + (uint64_t)S.ana_num_nodes);
    CHECK(H.traversal_bytes == (H.lines.size() + H.ana_recs.size()) * 16);
    CHECK(H.bvh_bytes == (H.lines.size() + H.tri_sh.size() + H.ana_recs.size()) * 16);
    // every source triangle once in the order; its record is that triangle's
    CHECK(H.tri_build->order.size() == nt && H.tri_sh.size() == 8 * nt);
    std::vector<int> seen((size_t)s.d.num_triangles, 0), want((size_t)s.d.num_triangles, 0);
    for (int32_t t : src) want[(size_t)t]++;
    for (size_t i = 0; i < nt; i++) {
        const uint32_t p = H.tri_build->order[i];
        CHECK(p < nt);
        if (p >= nt) return;
        const int t = src[p];
        seen[(size_t)t]++;
        const float4* r = &H.tri_sh[8 * i];
        CHECK(r[0].x == s.v1[3 * (size_t)t] && r[0].y == s.v1[3 * (size_t)t + 1] && r[0].z == s.v1[3 * (size_t)t + 2]);
        CHECK(r[0].w == s.v2[3 * (size_t)t] - s.v1[3 * (size_t)t]);
        CHECK(r[2].x == s.v3[3 * (size_t)t + 2] - s.v1[3 * (size_t)t + 2]);
        CHECK(r[3].y == s.n1[3 * (size_t)t + 1] && bits(r[5].y) == (uint32_t)s.tm[(size_t)t]);
        if (H.tri_uv) CHECK(r[6].x == s.t1[3 * (size_t)t] && r[6].z == s.t2[3 * (size_t)t] && r[7].y == s.t3[3 * (size_t)t + 1]);
        else CHECK(bits(r[6].x) == 0 && bits(r[7].y) == 0);
    }
    CHECK(seen == want);
    // chunks: word 0 = first record | (count - 1) << 29; the runs tile the records; a chunk's triangles are the records'
    std::vector<int> covered(nt, 0);
    for (size_t c = 0; c < H.tri_build->chunks.size() / 8; c++) {
        const float* w = reinterpret_cast<const float*>(&H.tri_build->chunks[8 * c]);
        const uint32_t w0 = bits(w[0]), first = w0 & 0x1FFFFFFFu, cnt = ((w0 >> 29) & 3u) + 1u;
        CHECK(cnt >= 1 && cnt <= 3 && (w0 >> 31) == 0 && first + cnt <= nt);
        if (first + cnt > nt) return;
        for (uint32_t t = 0; t < cnt; t++) {
            covered[first + t]++;
            CHECK(!std::memcmp(&w[1 + 9 * t], &H.tri_sh[8 * (size_t)(first + t)], 9 * sizeof(float)));
        }
        for (uint32_t k = 1 + 9 * cnt; k < 32; k++) CHECK(bits(w[k]) == 0);
    }
    for (size_t i = 0; i < nt; i++) CHECK(covered[i] == 1);
}

// ---- analytic records, heavy records, BLASes, lights
static void check_records(const FixScene& s, const pt::HostScene& H) {
    const pt_scene_desc& d = s.d;
    const pt::DevScene& S = H.S;
    const int lim[8] = {d.num_spheres, d.num_cubes, d.num_planes, 0, 0, d.num_sdf_shapes, d.num_volumes, d.num_transformed};
    size_t na = 0;
    for (int i = 0; i < d.num_shapes; i++) na += d.shape_kind[i] != PT_SHAPE_PLANE && d.shape_kind[i] != PT_SHAPE_TRIANGLE && d.shape_kind[i] != PT_SHAPE_MESH;
    CHECK(H.ana_recs.size() == 3 * na && (size_t)S.ana_count == na);
    std::vector<float4> heavy;
    std::vector<std::vector<int>> first(8);
    for (int k = 0; k < 8; k++) first[(size_t)k].assign((size_t)lim[k], -1);
    for (size_t i = 0; i < na; i++) {
        const uint32_t kind = bits(H.ana_recs[3 * i].w), j = bits(H.ana_recs[3 * i + 1].w), mat = bits(H.ana_recs[3 * i + 2].x);
        CHECK(kind == pt::KIND_SPHERE || kind == pt::KIND_CUBE || kind == pt::KIND_SDF || kind == pt::KIND_VOLUME || kind == pt::KIND_XFORM);
        CHECK(kind < 8 && (int)j < lim[kind & 7]);
        CHECK((int)mat <= d.num_materials);
        if (kind < 8 && (int)j < lim[kind] && first[kind][j] < 0) first[kind][j] = (int)i;
        if (kind >= pt::KIND_SDF) {
            CHECK(bits(H.ana_recs[3 * i + 2].y) == j);
            heavy.push_back(H.ana_recs[3 * i]);
        }
    }
    // heavy: exactly the SDF, Volume and transformed records, in record order, each with a box that is not empty
    CHECK(H.heavy.size() == 2 * heavy.size() && (size_t)S.heavy_count == heavy.size());
    size_t hi = 0;
    for (size_t i = 0; i < na && 2 * hi + 1 < H.heavy.size(); i++) {
        if (bits(H.ana_recs[3 * i].w) < (uint32_t)pt::KIND_SDF) continue;
        CHECK(bits(H.heavy[2 * hi].w) == (uint32_t)i);
        CHECK(H.heavy[2 * hi].x < H.heavy[2 * hi + 1].x && H.heavy[2 * hi].y < H.heavy[2 * hi + 1].y && H.heavy[2 * hi].z < H.heavy[2 * hi + 1].z);
        hi++;
    }
    // one BLAS per distinct instanced mesh; a transformed mesh's rec is its BLAS, another shape's its own ext record
    std::vector<int> blas_of((size_t)d.num_meshes, -1);
    int nblas = 0;
    CHECK(H.xforms.size() == (size_t)d.num_transformed && H.ext_recs.size() == 3 * H.xforms.size());
    for (int i = 0; i < d.num_transformed; i++) {
        const pt_transformed_shape& x = d.transformed[i];
        if (x.shape_kind == PT_SHAPE_MESH) {
            if (blas_of[(size_t)x.shape_index] < 0) blas_of[(size_t)x.shape_index] = nblas++;
            CHECK(H.xforms[(size_t)i].kind == pt::KIND_MESH && H.xforms[(size_t)i].rec == blas_of[(size_t)x.shape_index]);
        } else {
            CHECK(H.xforms[(size_t)i].rec == i);
            CHECK(bits(H.ext_recs[3 * (size_t)i + 1].w) == (uint32_t)x.shape_index);
        }
    }
    CHECK(H.blas.size() == (size_t)nblas);
    size_t recs = 0;
    for (int m = 0; m < d.num_meshes; m++)
        if (blas_of[(size_t)m] >= 0) {
            const pt::DevBlas& B = H.blas[(size_t)blas_of[(size_t)m]];
            CHECK((size_t)B.rec_off == recs && B.num_nodes > 0 && (size_t)(B.node_off + B.num_nodes) * 8 <= H.blas_nodes.size());
            recs += (size_t)d.mesh_count[m];
        }
    CHECK(H.blas_recs.size() == 3 * recs && H.blas_shade.size() == 3 * recs && H.blas_uv.size() == 2 * recs);
    // lights: the emissive shapes in Scene.Shapes order (MaterialAt(origin).Emittance > 0); a mesh contributes none
    std::vector<pt::DevLight> want;
    for (int i = 0; i < d.num_shapes; i++) {
        const int k = d.shape_kind[i], j = d.shape_index[i];
        const int ik = k == PT_SHAPE_TRANSFORMED ? d.transformed[j].shape_kind : k, ij = k == PT_SHAPE_TRANSFORMED ? d.transformed[j].shape_index : j;
        int mat = -1;
        if (ik == PT_SHAPE_SPHERE) mat = d.sphere_material[ij];
        else if (ik == PT_SHAPE_CUBE) mat = d.cube_material[ij];
        else if (ik == PT_SHAPE_PLANE) mat = d.plane_material[ij];
        else if (ik == PT_SHAPE_TRIANGLE) mat = d.tri_material[ij];
        else if (ik == PT_SHAPE_SDF) mat = d.sdf_shapes[ij].material;
        if (mat < 0 || !(d.materials[mat].emittance > 0)) continue;   // (the fixtures' Volumes and meshes are no lights)
        pt::DevLight L{};
        L.kind = k == PT_SHAPE_TRANSFORMED ? (int)pt::KIND_XFORM : k;
        L.mat = mat;
        L.phantom = k == PT_SHAPE_TRIANGLE || k == PT_SHAPE_TRANSFORMED;
        L.index = k == PT_SHAPE_TRIANGLE ? -1 : k == PT_SHAPE_PLANE ? 0 : first[(size_t)k][(size_t)j];
        want.push_back(L);
    }
    CHECK(H.lights.size() == want.size() && (size_t)S.num_lights == want.size());
    for (size_t i = 0; i < want.size() && i < H.lights.size(); i++) {
        const pt::DevLight& L = H.lights[i];
        CHECK(L.kind == want[i].kind && L.mat == want[i].mat && L.phantom == want[i].phantom && L.index == want[i].index);
        CHECK(L.radius > 0);
    }
}

// ---- every flag against its defining expression (pt_scene.h)
static void check_flags(const FixScene& s, const pt::HostScene& H, const pt::CompileOptions& opt) {
    const pt_scene_desc& d = s.d;
    const pt::DevScene& S = H.S;
    const int full_geom = d.num_sdf_shapes > 0 || d.num_volumes > 0 || d.num_transformed > 0;
    CHECK(S.full_geom == full_geom);
    CHECK(S.full == (d.num_textures > 0 || full_geom));
    int lean = 1;
    for (const pt::DevLight& L : H.lights)
        if (!L.phantom && (L.kind == pt::KIND_SDF || L.kind == pt::KIND_VOLUME || L.kind == pt::KIND_XFORM)) lean = 0;
    CHECK(S.lights_lean == lean);
    bool mat_tex = false;
    for (int i = 0; i < d.num_materials; i++)
        mat_tex = mat_tex || d.materials[i].texture || d.materials[i].normal_texture || d.materials[i].bump_texture || d.materials[i].gloss_texture;
    CHECK(S.shade_route == (S.full && !mat_tex && lean));
    CHECK(S.ana_linear == (S.ana_count > 0 && S.ana_count <= 8 && !full_geom));
    CHECK(S.route == (opt.route && full_geom && lean && S.ana_count <= 8 && S.heavy_count > 0 && S.tri_num_nodes > 64));
    CHECK(S.default_mat == d.num_materials && S.num_mats == d.num_materials + 1 && H.mats.size() == (size_t)S.num_mats);
    const pt::DevMaterial& dm = H.mats.back();
    CHECK(dm.color[0] == 0 && dm.color[1] == 0 && dm.color[2] == 0 && dm.emittance == 0);
    CHECK(dm.tex == -1 && dm.ntex == -1 && dm.btex == -1 && dm.gtex == -1);
    CHECK(S.env_tex == d.env_texture - 1 && S.env[1] == d.env_color[1]);
    CHECK(S.num_sdf == d.num_sdf_shapes && S.num_vol == d.num_volumes);
    // LDS staging: the SDF programs when they fit; the Volume only when it is the scene's one Volume
    const size_t sdf_need = H.sdf_prog.size() * sizeof(pt::DevSdfIns) + H.sdf_params.size() * sizeof(double);
    CHECK(S.sdf_prog_n == (int32_t)H.sdf_prog.size());
    CHECK(S.sdf_lds == (sdf_need > 0 && sdf_need <= 16384 ? (int32_t)sdf_need : 0));
    if (d.num_volumes == 1 && opt.vol_lds) CHECK(S.vol_lds > 0 && S.vol_lds % 16 == 0 && (size_t)S.vol_lds >= pt::kVolLdsHeader + H.vol_runs.size());
    else CHECK(S.vol_lds == 0);
    size_t cells = 0;
    for (const pt::HostVolume& v : H.volumes) {
        const size_t n = (size_t)(v.v.w + 1) * (v.v.h + 1) * (v.v.d + 1);
        CHECK(v.v.data == nullptr && v.v.windows == nullptr && v.v.runs == nullptr && v.v.cells == nullptr);
        CHECK(v.runs_off + n <= H.vol_runs.size());
        if (opt.vol_cells) { CHECK(v.cells_off == (int64_t)cells); cells += 8 * n; }
        else CHECK(v.cells_off == -1);
    }
    CHECK(H.vol_cells.size() == cells);
}

static void check_scene(const FixScene& s, const pt::CompileOptions& opt) {
    pt::HostScene H, H2;
    CHECK(compile(s, H, opt) == PT_OK);
    if (!H.tri_build) return;
    check_lines_and_triangles(s, H);
    check_records(s, H);
    check_flags(s, H, opt);
    CHECK(compile(s, H2, opt) == PT_OK);   // determinism: the same bytes in every array
    CHECK(digest(H) == digest(H2));
}

// ---- the fixed scene's own facts
static void check_fixed() {
    FixScene s, s1;
    fixed_scene(s, false);
    fixed_scene(s1, true);
    pt::CompileOptions off;
    off.vol_cells = off.vol_lds = off.route = false;
    for (const pt::CompileOptions& o : {pt::CompileOptions{}, off}) { check_scene(s, o); check_scene(s1, o); }
    pt::HostScene H, H1;
    CHECK(compile(s, H) == PT_OK && compile(s1, H1) == PT_OK);
    CHECK(H.sdf_shapes.size() == 2 && H.sdf_shapes[0].chain == 1 && H.sdf_shapes[1].chain == 0);
    CHECK(H.blas.size() == 1 && H.xforms[0].rec == 0 && H.xforms[1].rec == 0);   // one BLAS, shared by the two instances
    CHECK(H.tri_uv && H.S.num_planes == 1 && H.planes.size() == 2);
    CHECK(H.lights.size() == 5);   // sphere, cube, loose triangle, transformed sphere, the sphere again
    CHECK(H.lights[0].kind == pt::KIND_SPHERE && H.lights[4].kind == pt::KIND_SPHERE && H.lights[0].index == H.lights[4].index);
    CHECK(H.lights[2].kind == PT_SHAPE_TRIANGLE && H.lights[2].phantom == 1 && H.lights[3].kind == pt::KIND_XFORM && H.lights[3].phantom == 1);
    CHECK(H.S.vol_lds == 0 && H1.S.vol_lds > 0);   // two Volumes / the one-Volume variant
    CHECK(H.volumes.size() == 2 && H.windows.size() == 3 && H.volumes[1].win_off == 2 && H.volumes[1].vox_off == 27);
    CHECK(H.texs.size() == 2 && H.texs[1].off == 12 && H.tex_data.size() == 24);
    CHECK(H.S.route == 0 && H.S.full == 1 && H.S.full_geom == 1 && H.S.lights_lean == 1 && H.S.shade_route == 0);
}

// ---- the routed split's kind of scene; route follows the option
static void check_big() {
    FixScene s;
    big_scene(s, 20000, 41);
    pt::CompileOptions on, off;
    off.route = false;
    check_scene(s, on);
    check_scene(s, off);
    pt::HostScene H, H0;
    CHECK(compile(s, H, on) == PT_OK && compile(s, H0, off) == PT_OK);
    CHECK(H.S.route == 1 && H0.S.route == 0 && H.S.shade_route == 1 && H.S.vol_lds > 0);
    CHECK(H.tri_build == H0.tri_build);   // one geometry, one build
}

// ---- error cases: the code and a message
static void expect_error(const char* name, const pt_scene_desc* d, int code) {
    pt::HostScene H;
    std::string err;
    const int rc = pt::compile_scene(d, pt::CompileOptions{}, H, err);
    if (rc != code || err.empty()) {
        std::fprintf(stderr, "error case %s: got %d \"%s\", want %d\n", name, rc, err.c_str(), code);
        failures++;
    }
}
static void check_errors() {
    expect_error("null scene", nullptr, PT_ERR_INVALID_ARG);
    { FixScene s; fixed_scene(s, false); s.d.num_materials = 0; expect_error("no materials", &s.d, PT_ERR_INVALID_ARG); }
    { FixScene s; fixed_scene(s, false); s.sm[0] = 99; expect_error("material index", &s.d, PT_ERR_INVALID_ARG); }
    { FixScene s; fixed_scene(s, false); s.texs[0].width = 1; s.texs[0].height = 1; expect_error("1x1 texture", &s.d, PT_ERR_INVALID_ARG); }
    { FixScene s; fixed_scene(s, false); s.children[(size_t)s.nodes[1].first_child] = 1; expect_error("SDF child order", &s.d, PT_ERR_INVALID_ARG); }
    { FixScene s; fixed_scene(s, false); s.nodes[1].num_children = 0; expect_error("SDF child count", &s.d, PT_ERR_INVALID_ARG); }
    {   // kSdfStack nested scalings need kSdfStack + 1 point-stack entries
        FixScene s;
        fixed_scene(s, false);
        int n = s.node(PT_SDF_CUBE, {1, 1, 1}, {});
        for (int k = 0; k < pt::kSdfStack; k++) n = s.node(PT_SDF_SCALE, {0.9}, {n});
        s.sdfs[0].root = n;
        s.finish(2);
        expect_error("SDF depth", &s.d, PT_ERR_UNSUPPORTED);
    }
    { FixScene s; fixed_scene(s, false); s.mcount[0] = 7; expect_error("mesh range", &s.d, PT_ERR_INVALID_ARG); }
    { FixScene s; fixed_scene(s, false); s.xf[2].shape_index = 99; expect_error("inner index", &s.d, PT_ERR_INVALID_ARG); }
    { FixScene s; fixed_scene(s, false); s.xf[2].shape_kind = PT_SHAPE_TRIANGLE; expect_error("inner kind", &s.d, PT_ERR_UNSUPPORTED); }
    { FixScene s; fixed_scene(s, false); s.d.tri_t2 = nullptr; expect_error("t1 without t2", &s.d, PT_ERR_INVALID_ARG); }
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--digest")) {
        const std::string which = argc > 2 ? argv[2] : "fixed", off = argc > 3 ? argv[3] : "";
        FixScene s;
        if (which == "big") big_scene(s, 20000, 41);
        else fixed_scene(s, which == "fixed1");
        pt::CompileOptions opt;
        opt.vol_cells = off != "cells0"; opt.vol_lds = off != "lds0"; opt.route = off != "route0";
        pt::HostScene H;
        if (compile(s, H, opt) != PT_OK) return 1;
        for (const std::string& l : digest(H)) std::printf("%s\n", l.c_str());
        return 0;
    }
    check_fixed();
    check_big();
    check_errors();
    std::printf("scene_compile_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
