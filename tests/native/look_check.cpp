// look_check.cpp — the host side of pt_update_materials and pt_update_textures, stand-alone.
//
//   lights   For the fixture scenes (scene_fixture.h: fixed_scene with one and two volumes, big_scene) and a set of
//            material edits, the factored derivation (pt_scene_compile.h look_lights / look_flags) run on the tables
//            of the ORIGINAL compile with the edited material table gives, byte for byte, the lights, the side tables
//            (RefitTables::light_tri, ShapeRefitTables::light_kind / light_index, VolumeTables::slots / emittance,
//            LookTables::light_slot) and the flags (num_lights, lights_lean, route, shade_route) of a fresh
//            compile_scene of the descriptor with those materials substituted.  The edits: a recolour, a light dimmed,
//            one light off, every light off, each non-emissive material switched on (spheres, cubes, the plane, the SDF
//            shapes, both Volumes' windows, shapes that lie before existing lights in Scene.Shapes), a texture slot
//            taken away and one given.  Then the same after motion: a sphere, a cube, a transformed shape and the
//            loose triangle moved in the tables' current parameters against a fresh compile of the moved descriptor.
//   scenes   `look_check --scene NAME FILE`: the same comparison on a scene of ptsharp_amd/scenes.py that
//            tests/test_look_host.py flattened into FILE, under the same set of edits restated for any material table
//            (each material toggled by itself among them).
//   decode   pt_texture.h's tex_decode_run, run on the host in the kernel's lane order (block by block, lane by lane),
//            equals lut[byte] per channel for 2x2, 3x5, 67x33 and 256x2 (every byte value in every channel) in both
//            8-bit formats, at every source byte offset 0..3 and 16 and at texel slices on and off the 16-byte grid;
//            the doubles before and after the slice stay as they were.  The buffers are exactly as long as the image,
//            so AddressSanitizer sees any read or write past it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ptsharp_amd/csrc/pt_scene_compile.h"
#include "../../ptsharp_amd/csrc/pt_texture.h"
#include "scene_fixture.h"

static int failures = 0;
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            if (failures < 40) std::fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
            failures++;                                                           \
        }                                                                         \
    } while (0)

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

// ---- lights
typedef void (*Build)(FixScene&);
static void build_fixed2(FixScene& s) { fixed_scene(s, false); }
static void build_fixed1(FixScene& s) { fixed_scene(s, true); }
static void build_big(FixScene& s) { big_scene(s, 3000, 7u); }

typedef void (*Edit)(std::vector<pt_material>&);
struct NamedEdit { const char* name; Edit edit; };
static const NamedEdit kEdits[] = {
    {"none", [](std::vector<pt_material>&) {}},
    {"recolour", [](std::vector<pt_material>& m) { m[0].color[0] = 0.3; m[0].gloss = 0.2; m[0].index = 1.5; }},
    {"dim", [](std::vector<pt_material>& m) { m[1].emittance = 3; }},
    {"light-off", [](std::vector<pt_material>& m) { m[1].emittance = 0; }},
    {"all-off", [](std::vector<pt_material>& m) { for (auto& x : m) x.emittance = 0; }},
    {"white-on", [](std::vector<pt_material>& m) { m[0].emittance = 2; }},              // spheres, cubes, plane, SDF, window
    {"textured-on", [](std::vector<pt_material>& m) { m[2].emittance = 4; }},          // mesh triangles: a Mesh is no light
    {"glass-on", [](std::vector<pt_material>& m) { m[3].emittance = 1; }},             // SDF chain, Volume windows
    {"all-on", [](std::vector<pt_material>& m) { for (auto& x : m) x.emittance = 7; }},
    {"nan-and-negative", [](std::vector<pt_material>& m) { m[0].emittance = -1; m[1].emittance = std::nan(""); m[3].emittance = 1e-300; }},
    {"texture-off", [](std::vector<pt_material>& m) { for (auto& x : m) x.texture = 0; }},
    {"texture-on", [](std::vector<pt_material>& m) { for (auto& x : m) x.texture = 0; m[0].gloss_texture = 2; m[3].bump_texture = 1; }},
};

static void compare(const char* scene, const char* edit, const pt::HostScene& H0, const pt::ShapeRefitTables& T, const pt::LookTables& K,
                    const pt::HostScene& H1, const pt_scene_desc& d1, bool moved = false) {
    const int before = failures;
    std::vector<pt::DevMaterial> mats = H0.mats;
    CHECK((int)mats.size() == d1.num_materials + 1);
    for (int i = 0; i < d1.num_materials && i + 1 < (int)mats.size(); i++) pt::pack_material(d1.materials[i], mats[(size_t)i]);
    CHECK(same(mats, H1.mats));
    pt::LookLights L;
    pt::look_lights(K, T, mats, L);
    pt::DevScene S = H0.S;
    pt::look_flags(K, L.lights, mats, S.tri_num_nodes, S);
    S.num_lights = (int32_t)L.lights.size();
    // (after motion a fresh compile sorts the analytic BVH again: DevLight::index, a light's position among the analytic
    // records, is the one word that follows the order; an update keeps the order, so it is left out there)
    std::vector<pt::DevLight> mine = L.lights, theirs = H1.lights;
    if (moved) for (std::vector<pt::DevLight>* v : {&mine, &theirs}) for (pt::DevLight& l : *v) l.index = 0;
    CHECK(same(mine, theirs));
    CHECK(same(L.light_tri, H1.refit.light_tri));
    CHECK(same(L.light_kind, H1.shape_refit.light_kind));
    CHECK(same(L.light_index, H1.shape_refit.light_index));
    CHECK(same(L.vol_slots, H1.volume_update.slots));
    CHECK(same(L.emittance, H1.volume_update.emittance));
    CHECK(same(L.light_slot, H1.look.light_slot));
    CHECK(S.num_lights == H1.S.num_lights && S.lights_lean == H1.S.lights_lean && S.route == H1.S.route && S.shade_route == H1.S.shade_route);
    std::printf("case %s %s %s: lights %zu lean %d route %d shade_route %d\n", scene, edit, failures == before ? "ok" : "FAILED",
                L.lights.size(), S.lights_lean, S.route, S.shade_route);
}

static void lights_cases(const char* name, Build build, bool textures) {
    FixScene s0;
    build(s0);
    pt::HostScene H0;
    std::string err;
    const pt::CompileOptions opt;
    CHECK(pt::compile_scene(&s0.d, opt, H0, err) == PT_OK);
    for (const NamedEdit& e : kEdits) {
        if (!textures && !std::strncmp(e.name, "texture-", 8)) continue;   // a scene without textures has no slot to give
        FixScene s1;
        build(s1);
        e.edit(s1.mats);
        pt::HostScene H1;
        CHECK(pt::compile_scene(&s1.d, opt, H1, err) == PT_OK);
        compare(name, e.name, H0, H0.shape_refit, H0.look, H1, s1.d);
    }
    // after motion: the tables' current parameters moved as the updates move them, the moved descriptor compiled fresh
    FixScene s1;
    build(s1);
    for (auto& m : s1.mats) m.emittance = 6;   // everything that can be a light is one
    pt::ShapeRefitTables T = H0.shape_refit;
    pt::LookTables K = H0.look;
    for (size_t i = 0; i < s1.sc.size(); i++) s1.sc[i] += 0.25f * (float)(i % 3 + 1);
    for (size_t i = 0; i < s1.sr.size(); i++) s1.sr[i] *= 1.5;
    for (size_t i = 0; i < s1.cmin.size(); i++) { s1.cmin[i] -= 0.5f; s1.cmax[i] += 0.125f * (float)(i + 1); }
    for (auto& x : s1.xf) FixScene::translation(x.matrix, x.inverse, x.matrix[3] + 1.0, x.matrix[7] - 2.0, x.matrix[11] + 0.5);
    T.sphere_center = s1.sc; T.sphere_radius = s1.sr; T.cube_min = s1.cmin; T.cube_max = s1.cmax;
    for (size_t i = 0; i < s1.xf.size(); i++) {
        std::memcpy(&T.xf_matrix[16 * i], s1.xf[i].matrix, 16 * sizeof(double));
        std::memcpy(&T.xf_inverse[16 * i], s1.xf[i].inverse, 16 * sizeof(double));
    }
    for (const pt::LookSlot& slot : K.slots) {   // the loose triangles, moved in the descriptor and in the mirror
        if (slot.vert < 0) continue;
        const size_t j = (size_t)slot.index;
        for (int q = 0; q < 3; q++) { s1.v1[3 * j + q] += 1.f; s1.v2[3 * j + q] += 2.f; s1.v3[3 * j + q] -= 0.5f; }
        std::memcpy(&K.tri_verts[(size_t)slot.vert], &s1.v1[3 * j], 12);
        std::memcpy(&K.tri_verts[(size_t)slot.vert + 3], &s1.v2[3 * j], 12);
        std::memcpy(&K.tri_verts[(size_t)slot.vert + 6], &s1.v3[3 * j], 12);
    }
    pt::HostScene H1;
    CHECK(pt::compile_scene(&s1.d, opt, H1, err) == PT_OK);
    compare(name, "after-motion", H0, T, K, H1, s1.d, true);
}

// ---- a scene of ptsharp_amd/scenes.py, flattened by tests/test_look_host.py into a file (scene_file below reads what
// that test's dump_scene writes: the fields of pt_scene_desc in order, counts as int32, arrays raw)
struct FileScene {
    std::vector<char> bytes;
    size_t at = 0;
    bool ok = true;
    std::vector<pt_texture> texs;
    std::vector<pt_volume> vols;
    pt_scene_desc d;
    int32_t i32() { int32_t v = 0; take(&v, 4); return v; }
    double f64() { double v = 0; take(&v, 8); return v; }
    void take(void* dst, size_t n) {
        if (at + n > bytes.size()) { ok = false; std::memset(dst, 0, n); return; }
        std::memcpy(dst, bytes.data() + at, n);
        at += n;
    }
    template <class T>
    T* arr(size_t n) {   // in place: the file's arrays are 8-byte aligned by the writer
        const size_t b = n * sizeof(T);
        if (at + b > bytes.size()) { ok = false; return nullptr; }
        T* p = (T*)(bytes.data() + at);
        at += (b + 7) & ~(size_t)7;
        return n ? p : nullptr;
    }
};
static bool scene_file(const char* path, FileScene& f) {
    FILE* fp = std::fopen(path, "rb");
    if (!fp) return false;
    std::fseek(fp, 0, SEEK_END);
    const long n = std::ftell(fp);
    std::fseek(fp, 0, SEEK_SET);
    f.bytes.resize((size_t)n);
    const bool read = std::fread(f.bytes.data(), 1, (size_t)n, fp) == (size_t)n;
    std::fclose(fp);
    if (!read) return false;
    pt_scene_desc& d = f.d;
    std::memset(&d, 0, sizeof d);
    if (f.i32() != 0x4B4F4F4C || f.i32() != (int32_t)sizeof(pt_scene_desc)) return false;   // "LOOK", and the ABI's struct
    d.num_materials = f.i32(); f.i32(); d.materials = f.arr<pt_material>((size_t)d.num_materials);
    d.num_shapes = f.i32(); f.i32(); d.shape_kind = f.arr<int32_t>((size_t)d.num_shapes); d.shape_index = f.arr<int32_t>((size_t)d.num_shapes);
    d.num_spheres = f.i32(); f.i32();
    d.sphere_center = f.arr<float>(3 * (size_t)d.num_spheres); d.sphere_radius = f.arr<double>((size_t)d.num_spheres); d.sphere_material = f.arr<int32_t>((size_t)d.num_spheres);
    d.num_cubes = f.i32(); f.i32();
    d.cube_min = f.arr<float>(3 * (size_t)d.num_cubes); d.cube_max = f.arr<float>(3 * (size_t)d.num_cubes); d.cube_material = f.arr<int32_t>((size_t)d.num_cubes);
    d.num_planes = f.i32(); f.i32();
    d.plane_point = f.arr<float>(3 * (size_t)d.num_planes); d.plane_normal = f.arr<float>(3 * (size_t)d.num_planes); d.plane_material = f.arr<int32_t>((size_t)d.num_planes);
    d.num_triangles = f.i32(); f.i32();
    const size_t nt = (size_t)d.num_triangles;
    d.tri_v1 = f.arr<float>(3 * nt); d.tri_v2 = f.arr<float>(3 * nt); d.tri_v3 = f.arr<float>(3 * nt);
    d.tri_n1 = f.arr<float>(3 * nt); d.tri_n2 = f.arr<float>(3 * nt); d.tri_n3 = f.arr<float>(3 * nt);
    d.tri_material = f.arr<int32_t>(nt);
    d.tri_t1 = f.arr<float>(3 * nt); d.tri_t2 = f.arr<float>(3 * nt); d.tri_t3 = f.arr<float>(3 * nt);
    d.num_meshes = f.i32(); f.i32(); d.mesh_first = f.arr<int32_t>((size_t)d.num_meshes); d.mesh_count = f.arr<int32_t>((size_t)d.num_meshes);
    for (int k = 0; k < 3; k++) d.env_color[k] = f.f64();
    d.env_texture_angle = f.f64();
    d.env_texture = f.i32();
    d.num_textures = f.i32();
    for (int i = 0; i < d.num_textures && f.ok; i++) {
        pt_texture t;
        t.width = f.i32(); t.height = f.i32();
        t.data = f.arr<double>(3 * (size_t)t.width * (size_t)t.height);
        f.texs.push_back(t);
    }
    d.textures = f.texs.data();
    d.num_sdf_nodes = f.i32();
    const int32_t nchildren = f.i32();
    d.sdf_nodes = f.arr<pt_sdf_node>((size_t)d.num_sdf_nodes); d.sdf_children = f.arr<int32_t>((size_t)nchildren);
    d.num_sdf_shapes = f.i32(); f.i32(); d.sdf_shapes = f.arr<pt_sdf_shape>((size_t)d.num_sdf_shapes);
    d.num_volumes = f.i32(); f.i32();
    for (int i = 0; i < d.num_volumes && f.ok; i++) {
        pt_volume v;
        std::memset(&v, 0, sizeof v);
        v.w = f.i32(); v.h = f.i32(); v.d = f.i32(); v.num_windows = f.i32();
        v.zscale = f.f64();
        f.take(v.box_min, 12); f.take(v.box_max, 12);
        v.data = f.arr<double>((size_t)v.w * v.h * v.d);
        v.windows = f.arr<pt_volume_window>((size_t)v.num_windows);
        f.vols.push_back(v);
    }
    d.volumes = f.vols.data();
    d.num_transformed = f.i32(); f.i32(); d.transformed = f.arr<pt_transformed_shape>((size_t)d.num_transformed);
    return f.ok && f.at == f.bytes.size();
}

// The edits of kEdits restated for any material table: a recolour, every light dimmed, every light off, each material
// switched on by itself (a shape of every kind the scene has becomes a light in one of them, shapes before and after
// the existing lights), all on, NaN / negative / denormal-small emittances, every texture slot taken away, one given
static int file_cases(const char* name, const char* path) {
    FileScene f;
    if (!scene_file(path, f)) { std::fprintf(stderr, "%s: not a scene file\n", path); return 2; }
    pt_material* m = const_cast<pt_material*>(f.d.materials);
    const std::vector<pt_material> orig(m, m + f.d.num_materials);
    const size_t nm = orig.size();
    pt::HostScene H0;
    std::string err;
    const pt::CompileOptions opt;
    if (pt::compile_scene(&f.d, opt, H0, err) != PT_OK) { std::fprintf(stderr, "%s: %s\n", name, err.c_str()); return 2; }
    auto run = [&](const std::string& edit) {
        pt::HostScene H1;
        CHECK(pt::compile_scene(&f.d, opt, H1, err) == PT_OK);   // (the triangle BVH comes from the process-wide cache)
        compare(name, edit.c_str(), H0, H0.shape_refit, H0.look, H1, f.d);
        std::copy(orig.begin(), orig.end(), m);
    };
    run("none");
    m[0].color[0] = 0.3; m[0].gloss = 0.2; m[0].index = 1.5; run("recolour");
    for (size_t i = 0; i < nm; i++) m[i].emittance *= 0.3;
    run("dim");
    for (size_t i = 0; i < nm; i++) m[i].emittance = 0;
    run("all-off");
    for (size_t i = 0; i < nm; i++) { m[i].emittance = orig[i].emittance > 0 ? 0.0 : 2.0; run("toggle-" + std::to_string(i)); }
    for (size_t i = 0; i < nm; i++) m[i].emittance = 7;
    run("all-on");
    for (size_t i = 0; i < nm; i++) m[i].emittance = i % 3 == 0 ? -1.0 : i % 3 == 1 ? std::nan("") : 1e-300;
    run("nan-and-negative");
    if (f.d.num_textures > 0) {
        for (size_t i = 0; i < nm; i++) m[i].texture = m[i].normal_texture = m[i].bump_texture = m[i].gloss_texture = 0;
        run("texture-off");
        for (size_t i = 0; i < nm; i++) m[i].texture = m[i].normal_texture = m[i].bump_texture = m[i].gloss_texture = 0;
        m[nm - 1].gloss_texture = f.d.num_textures; run("texture-on");
    }
    std::printf("look_check %s: %d failures\n", name, failures);
    return failures ? 1 : 0;
}

// ---- decode
static void decode_case(int w, int h, int format, uint64_t src_off, int dst_shift) {
    const int before = failures;
    const int bpp = pt::tex_bpp(format);
    const uint64_t pixels = pt::tex_pixels(w, h);
    std::vector<double> lut(pt::kTexLut);
    for (int i = 0; i < pt::kTexLut; i++) lut[(size_t)i] = 0.5 * (double)i / 255.0 + 1e-3 * (double)(i * i);   // all distinct
    std::vector<uint8_t> src((size_t)src_off + (size_t)pixels * (size_t)bpp);   // exactly the staging up to the image's end
    for (size_t i = 0; i < src.size(); i++) src[i] = (uint8_t)((i * 37u + 11u) & 255u);
    if (w == 256) for (uint64_t p = 0; p < pixels; p++) for (int c = 0; c < bpp; c++) src[(size_t)src_off + p * bpp + c] = (uint8_t)(p & 255u);
    // the slice between two guards of 2 doubles; dst_shift moves it off (1) or onto (0) the 16-byte grid
    std::vector<double> all(4 + 3 * (size_t)pixels + 2, -7.0);
    double* base = all.data();
    if ((((uintptr_t)base >> 3) & 1u) != (uintptr_t)(dst_shift & 1)) base += 1;   // base's parity = dst_shift
    double* dst = base + 2;
    const uint64_t blocks = pt::tex_block_count(pixels);
    CHECK(blocks * pt::kTexBlock * pt::kTexRun >= pixels && (blocks - 1) * pt::kTexBlock * pt::kTexRun < pixels);
    for (uint64_t b = 0; b < blocks; b++)
        for (int lane = 0; lane < pt::kTexBlock; lane++) {
            const uint64_t run = b * pt::kTexBlock + (uint64_t)lane;
            if (run < pt::tex_run_count(pixels)) pt::tex_decode_run(src.data(), src_off, bpp, run, pixels, lut.data(), dst);
        }
    for (uint64_t p = 0; p < pixels; p++)
        for (int c = 0; c < 3; c++) {
            const double want = lut[src[(size_t)src_off + p * bpp + c]];
            CHECK(!std::memcmp(&dst[3 * p + c], &want, 8));
        }
    CHECK(dst[-1] == -7.0 && dst[-2] == -7.0 && dst[3 * pixels] == -7.0);
    if (failures != before) std::printf("decode %dx%d format %d src_off %llu dst_shift %d FAILED\n", w, h, format, (unsigned long long)src_off, dst_shift);
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "--scene")) return file_cases(argv[2], argv[3]);
    lights_cases("fixed-two-volumes", build_fixed2, true);
    lights_cases("fixed-one-volume", build_fixed1, true);
    lights_cases("big", build_big, false);
    const int sizes[4][2] = {{2, 2}, {3, 5}, {67, 33}, {256, 2}};
    for (const auto& wh : sizes) {
        const int before = failures;
        for (int format = 1; format <= 2; format++)
            for (uint64_t src_off : {0ull, 1ull, 2ull, 3ull, 16ull})
                for (int shift = 0; shift < 2; shift++) decode_case(wh[0], wh[1], format, src_off, shift);
        std::printf("case decode %dx%d %s\n", wh[0], wh[1], failures == before ? "ok" : "FAILED");
    }
    CHECK(pt::tex_run_count(0) == 0 && pt::tex_run_len(0, 0) == 0 && pt::tex_run_len(1, 7) == 3 && pt::tex_run_len(1, 8) == 4);
    CHECK(pt::tex_src_byte(5, 1ull << 33, 4) == 5 + (1ull << 35) && pt::tex_dst_first(1ull << 33) == 3ull << 33);   // past 2^32
    CHECK(pt::tex_block_count(8192ull * 8192ull) == 8192ull * 8192ull / 1024);
    std::printf("look_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
