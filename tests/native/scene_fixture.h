// scene_fixture.h — pt_scene_desc scenes built in C++ for the host-only scene compile
// (ptsharp_amd/csrc/pt_scene_compile.h): scene_compile_check.cpp and sanitize_host.cpp.
//   fixed_scene   the smallest scene that reaches every branch of the compile: 2 spheres (one emissive), 2 cubes
//                 (one emissive), a plane, a loose emissive triangle, a 6-triangle mesh with uv at top level and
//                 inside two transformed shapes, a transformed emissive sphere, an SDF chain (scale of a cube), an
//                 SDF union of a transformed sphere and a difference of a repeated torus and a cylinder, a 3x3x3
//                 Volume with two windows, a transformed 2x2x2 Volume (left out with one_volume), a 2x2 texture on
//                 one material, an environment texture; the emissive sphere is in Scene.Shapes twice.
//   big_scene     n random triangles as one mesh, two spheres (one emissive), a cube, one SDF shape, one Volume:
//                 the kind of scene the routed split takes.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ptsharp_hip.h"

struct FixScene {
    std::vector<pt_material> mats;
    std::vector<int32_t> kinds, idx;
    std::vector<float> sc, cmin, cmax, pp, pn;
    std::vector<double> sr;
    std::vector<int32_t> sm, cm, pm, tm, mfirst, mcount;
    std::vector<float> v1, v2, v3, n1, n2, n3, t1, t2, t3;
    std::vector<double> tex0, tex1, vox0, vox1;
    std::vector<pt_texture> texs;
    std::vector<pt_sdf_node> nodes;
    std::vector<int32_t> children;
    std::vector<pt_sdf_shape> sdfs;
    std::vector<pt_volume_window> win0, win1;
    std::vector<pt_volume> vols;
    std::vector<pt_transformed_shape> xf;
    pt_scene_desc d;

    FixScene() { std::memset(&d, 0, sizeof d); }
    FixScene(const FixScene&) = delete;
    FixScene& operator=(const FixScene&) = delete;

    int material(double r, double g, double b, double emittance) {
        pt_material m;
        std::memset(&m, 0, sizeof m);
        m.color[0] = r; m.color[1] = g; m.color[2] = b;
        m.emittance = emittance; m.index = 1; m.reflectivity = -1;
        mats.push_back(m);
        return (int)mats.size() - 1;
    }
    void shape(int kind, int index) { kinds.push_back(kind); idx.push_back(index); }
    int sphere(float x, float y, float z, double r, int mat) {
        sc.insert(sc.end(), {x, y, z}); sr.push_back(r); sm.push_back(mat);
        return (int)sr.size() - 1;
    }
    int cube(float x0, float y0, float z0, float x1, float y1, float z1, int mat) {
        cmin.insert(cmin.end(), {x0, y0, z0}); cmax.insert(cmax.end(), {x1, y1, z1}); cm.push_back(mat);
        return (int)cm.size() - 1;
    }
    int triangle(const float* a, const float* b, const float* c, int mat) {
        v1.insert(v1.end(), a, a + 3); v2.insert(v2.end(), b, b + 3); v3.insert(v3.end(), c, c + 3);
        for (std::vector<float>* n : {&n1, &n2, &n3}) n->insert(n->end(), {0.f, 1.f, 0.f});
        t1.insert(t1.end(), {a[0], a[2], 0.f}); t2.insert(t2.end(), {b[0], b[2], 0.f}); t3.insert(t3.end(), {c[0], c[2], 0.f});
        tm.push_back(mat);
        return (int)tm.size() - 1;
    }
    int node(int op, std::initializer_list<double> params, std::initializer_list<int> kids) {
        pt_sdf_node n;
        std::memset(&n, 0, sizeof n);
        n.op = op;
        n.num_children = (int32_t)kids.size();
        n.first_child = (int32_t)children.size();
        int k = 0;
        for (double p : params) n.params[k++] = p;
        for (int i = 0; i < 4; i++) n.matrix[5 * i] = n.inverse[5 * i] = 1.0;
        for (int c : kids) children.push_back(c);
        nodes.push_back(n);
        return (int)nodes.size() - 1;
    }
    static void translation(double* m, double* inv, double x, double y, double z) {
        for (int i = 0; i < 16; i++) m[i] = inv[i] = (i % 5 == 0) ? 1.0 : 0.0;
        m[3] = x; m[7] = y; m[11] = z;
        inv[3] = -x; inv[7] = -y; inv[11] = -z;
    }
    int transformed(int kind, int index, double x, double y, double z) {
        pt_transformed_shape t;
        std::memset(&t, 0, sizeof t);
        t.shape_kind = kind; t.shape_index = index;
        translation(t.matrix, t.inverse, x, y, z);
        xf.push_back(t);
        return (int)xf.size() - 1;
    }
    int volume(int w, int h, int dd, std::vector<double>& data, std::vector<pt_volume_window>& win, float x0, float x1) {
        data.resize((size_t)w * h * dd);
        for (size_t i = 0; i < data.size(); i++) data[i] = (double)((i * 7) % 11) / 10.0;
        pt_volume v;
        std::memset(&v, 0, sizeof v);
        v.w = w; v.h = h; v.d = dd; v.num_windows = (int32_t)win.size(); v.zscale = 1.0;
        v.box_min[0] = x0; v.box_min[1] = 0.f; v.box_min[2] = -1.f;
        v.box_max[0] = x1; v.box_max[1] = 2.f; v.box_max[2] = 1.f;
        vols.push_back(v);
        return (int)vols.size() - 1;
    }
    // pointers last: the vectors no longer move
    void finish(int env_texture) {
        if (!vols.empty()) { vols[0].data = vox0.data(); vols[0].windows = win0.data(); }
        if (vols.size() > 1) { vols[1].data = vox1.data(); vols[1].windows = win1.data(); }
        d.num_materials = (int32_t)mats.size(); d.materials = mats.data();
        d.num_shapes = (int32_t)kinds.size(); d.shape_kind = kinds.data(); d.shape_index = idx.data();
        d.num_spheres = (int32_t)sr.size(); d.sphere_center = sc.data(); d.sphere_radius = sr.data(); d.sphere_material = sm.data();
        d.num_cubes = (int32_t)cm.size(); d.cube_min = cmin.data(); d.cube_max = cmax.data(); d.cube_material = cm.data();
        d.num_planes = (int32_t)pm.size(); d.plane_point = pp.data(); d.plane_normal = pn.data(); d.plane_material = pm.data();
        d.num_triangles = (int32_t)tm.size();
        d.tri_v1 = v1.data(); d.tri_v2 = v2.data(); d.tri_v3 = v3.data();
        d.tri_n1 = n1.data(); d.tri_n2 = n2.data(); d.tri_n3 = n3.data();
        d.tri_t1 = t1.data(); d.tri_t2 = t2.data(); d.tri_t3 = t3.data();
        d.tri_material = tm.data();
        d.num_meshes = (int32_t)mfirst.size(); d.mesh_first = mfirst.data(); d.mesh_count = mcount.data();
        d.env_color[0] = 0.1; d.env_color[1] = 0.2; d.env_color[2] = 0.3;
        d.num_textures = (int32_t)texs.size(); d.textures = texs.data();
        d.env_texture = env_texture; d.env_texture_angle = 0.25;
        d.num_sdf_nodes = (int32_t)nodes.size(); d.sdf_nodes = nodes.data(); d.sdf_children = children.data();
        d.num_sdf_shapes = (int32_t)sdfs.size(); d.sdf_shapes = sdfs.data();
        d.num_volumes = (int32_t)vols.size(); d.volumes = vols.data();
        d.num_transformed = (int32_t)xf.size(); d.transformed = xf.data();
    }
};

enum FixMat { MAT_WHITE = 0, MAT_LIGHT = 1, MAT_TEXTURED = 2, MAT_GLASS = 3, MAT_LIGHT2 = 4 };

inline void fixed_scene(FixScene& s, bool one_volume) {
    s.material(0.9, 0.9, 0.9, 0);
    s.material(1, 1, 1, 10);
    s.material(0.5, 0.6, 0.7, 0);
    s.material(0.2, 0.3, 0.4, 0);
    s.material(1, 0.9, 0.8, 5);
    s.tex0 = {0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 0.9, 0.8};
    s.tex1 = {0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.0, 0.1, 0.2};
    s.texs = {pt_texture{2, 2, s.tex0.data()}, pt_texture{2, 2, s.tex1.data()}};
    s.mats[MAT_TEXTURED].texture = 1;
    const int s0 = s.sphere(0.f, 1.f, 0.f, 1.0, MAT_WHITE), s1 = s.sphere(3.f, 4.f, 0.f, 0.5, MAT_LIGHT);
    const int s2 = s.sphere(0.f, 0.f, 0.f, 0.25, MAT_LIGHT);   // the transformed shape's inner sphere
    const int c0 = s.cube(-5.f, -1.f, -5.f, 5.f, 0.f, 5.f, MAT_WHITE), c1 = s.cube(-4.f, 5.f, -1.f, -3.f, 6.f, 1.f, MAT_LIGHT2);
    s.pp = {0.f, -2.f, 0.f}; s.pn = {0.f, 1.f, 0.f}; s.pm = {MAT_WHITE};
    const float a[3] = {6.f, 3.f, 0.f}, b[3] = {7.f, 3.f, 0.f}, c[3] = {6.f, 3.f, 1.f};
    const int loose = s.triangle(a, b, c, MAT_LIGHT);
    for (int i = 0; i < 6; i++) {   // a strip above the floor
        const float p[3] = {(float)i * 0.5f, 0.5f, 2.f}, q[3] = {(float)i * 0.5f + 0.5f, 0.5f, 2.f}, r[3] = {(float)i * 0.5f, 0.75f, 2.5f};
        s.triangle(p, q, r, MAT_TEXTURED);
    }
    s.mfirst = {1}; s.mcount = {6};
    const int cube = s.node(PT_SDF_CUBE, {1, 1, 1}, {});
    const int chain = s.node(PT_SDF_SCALE, {0.5}, {cube});
    const int ball = s.node(PT_SDF_SPHERE, {0.5, 2}, {});
    const int moved = s.node(PT_SDF_TRANSFORM, {}, {ball});
    FixScene::translation(s.nodes[(size_t)moved].matrix, s.nodes[(size_t)moved].inverse, 0.5, 0, 0);
    const int torus = s.node(PT_SDF_TORUS, {1, 0.25, 2, 2}, {});
    const int rep = s.node(PT_SDF_REPEAT, {4, 4, 4}, {torus});
    const int cyl = s.node(PT_SDF_CYLINDER, {0.2, 2}, {});
    const int diff = s.node(PT_SDF_DIFFERENCE, {}, {rep, cyl});
    const int uni = s.node(PT_SDF_UNION, {}, {moved, diff});
    s.sdfs = {pt_sdf_shape{chain, MAT_GLASS}, pt_sdf_shape{uni, MAT_WHITE}};
    s.win0 = {pt_volume_window{0.2, 0.5, MAT_WHITE, 0}, pt_volume_window{0.6, 0.9, MAT_GLASS, 0}};
    s.win1 = {pt_volume_window{0.3, 0.8, MAT_GLASS, 0}};
    const int vol0 = s.volume(3, 3, 3, s.vox0, s.win0, 8.f, 10.f);
    const int x0 = s.transformed(PT_SHAPE_MESH, 0, 0, 3, 0), x1 = s.transformed(PT_SHAPE_MESH, 0, 0, 6, 0);
    const int x2 = s.transformed(PT_SHAPE_SPHERE, s2, -6, 2, 0);
    s.shape(PT_SHAPE_SPHERE, s0); s.shape(PT_SHAPE_SPHERE, s1);
    s.shape(PT_SHAPE_CUBE, c0); s.shape(PT_SHAPE_CUBE, c1);
    s.shape(PT_SHAPE_PLANE, 0);
    s.shape(PT_SHAPE_TRIANGLE, loose);
    s.shape(PT_SHAPE_MESH, 0);
    s.shape(PT_SHAPE_TRANSFORMED, x0); s.shape(PT_SHAPE_TRANSFORMED, x1); s.shape(PT_SHAPE_TRANSFORMED, x2);
    s.shape(PT_SHAPE_SDF, 0); s.shape(PT_SHAPE_SDF, 1);
    s.shape(PT_SHAPE_VOLUME, vol0);
    if (!one_volume) {
        const int vol1 = s.volume(2, 2, 2, s.vox1, s.win1, -1.f, 1.f);
        s.shape(PT_SHAPE_TRANSFORMED, s.transformed(PT_SHAPE_VOLUME, vol1, 12, 0, 0));
    }
    s.shape(PT_SHAPE_SPHERE, s1);   // a second time: records and lights name its first occurrence
    s.finish(2);
}

// A 32-bit LCG, so the triangles are the same whatever the standard library
struct FixRng {
    uint32_t s;
    float next() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f); }
};

inline void big_scene(FixScene& s, int ntri, uint32_t seed) {
    s.material(0.9, 0.9, 0.9, 0);
    s.material(1, 1, 1, 10);
    s.material(0.5, 0.6, 0.7, 0);
    s.material(0.2, 0.3, 0.4, 0);
    FixRng r{seed};
    for (int i = 0; i < ntri; i++) {
        const float cx = r.next() * 20.f - 10.f, cy = r.next() * 10.f, cz = r.next() * 20.f - 10.f;
        float p[3][3];
        for (auto& v : p) { v[0] = cx + r.next() * 0.2f; v[1] = cy + r.next() * 0.2f; v[2] = cz + r.next() * 0.2f; }
        s.triangle(p[0], p[1], p[2], MAT_TEXTURED);
    }
    s.mfirst = {0}; s.mcount = {ntri};
    const int s0 = s.sphere(0.f, 12.f, 0.f, 1.0, MAT_WHITE), s1 = s.sphere(3.f, 14.f, 0.f, 0.5, MAT_LIGHT);
    const int c0 = s.cube(-12.f, -1.f, -12.f, 12.f, 0.f, 12.f, MAT_WHITE);
    const int cube = s.node(PT_SDF_CUBE, {1, 1, 1}, {});
    s.sdfs = {pt_sdf_shape{s.node(PT_SDF_SCALE, {0.5}, {cube}), MAT_GLASS}};
    s.win0 = {pt_volume_window{0.2, 0.5, MAT_WHITE, 0}};
    const int vol0 = s.volume(4, 3, 5, s.vox0, s.win0, 13.f, 15.f);
    s.shape(PT_SHAPE_MESH, 0);
    s.shape(PT_SHAPE_SPHERE, s0); s.shape(PT_SHAPE_SPHERE, s1);
    s.shape(PT_SHAPE_CUBE, c0);
    s.shape(PT_SHAPE_SDF, 0);
    s.shape(PT_SHAPE_VOLUME, vol0);
    s.finish(0);
}
