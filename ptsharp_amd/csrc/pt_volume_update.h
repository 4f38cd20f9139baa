// pt_volume_update.h — a Volume's derived tables stated once, per cell, for the host and the device.
//
// pt_upload_scene builds two tables per Volume over the lattice of Volume.Sample's cells, x0 in -1..w-1, y0 in
// -1..h-1, z0 in -1..d-1, x fastest: the uniform-cell signs of the march skip (1 B per cell) and the cell-major
// corners (64 B per cell).  pt_update_volumes rebuilds them on the device after new voxels or new windows.  Both
// run the functions below cell by cell: the host's loops (vol_build_runs, vol_build_cells) at upload, the kernels
// of pt_volume.hip at an update, so the two cannot drift apart.  tests/native/volumes_check.cpp compares them
// with a restatement of the loops they replaced, byte for byte.
//
// Host only, below them: pt_update_volumes' argument check and its light-membership test.
//
// pt_ext.h includes this header at its end (its table builders live here); including either gives both.
#pragma once
#include <stdint.h>

#include "../../include/ptsharp_hip.h"
#include "pt_ext.h"

#pragma clang fp contract(off)

namespace pt {

// ---------------------------------------------------------------- the lattice, in 64 bits
// Every index and byte offset of the tables is formed in 64 bits: 64 B per cell passes 2^31 at 33M cells, below a
// 512^3 grid (DESIGN.md §10 records what a 32-bit offset did once).
PT_HD uint64_t vol_cell_count(int32_t w, int32_t h, int32_t d) {
    return ((uint64_t)w + 1) * ((uint64_t)h + 1) * ((uint64_t)d + 1);
}
PT_HD uint64_t vol_cell_index(int32_t w, int32_t h, int x0, int y0, int z0) {
    const uint64_t sx = (uint64_t)w + 1, sy = (uint64_t)h + 1;
    return (uint64_t)(x0 + 1) + (uint64_t)(y0 + 1) * sx + (uint64_t)(z0 + 1) * sx * sy;
}
// cell i's first double in the cells table, and its byte offset there
PT_HD uint64_t vol_cell_first(uint64_t i) { return 8 * i; }
PT_HD uint64_t vol_cell_byte(uint64_t i) { return 64 * i; }
// the inverse of vol_cell_index
PT_HD void vol_cell_coords(int32_t w, int32_t h, uint64_t i, int& x0, int& y0, int& z0) {
    const uint64_t sx = (uint64_t)w + 1, sy = (uint64_t)h + 1;
    if (i <= 0xffffffffull && sx * sy <= 0xffffffffull) {   // the usual case in 32-bit divisions
        const uint32_t j = (uint32_t)i, a = (uint32_t)sx, b = (uint32_t)(sx * sy);
        const uint32_t z = j / b, r = j - z * b, y = r / a;
        x0 = (int)(r - y * a) - 1; y0 = (int)y - 1; z0 = (int)z - 1;
        return;
    }
    const uint64_t z = i / (sx * sy), r = i - z * (sx * sy), y = r / sx;
    x0 = (int)(r - y * sx) - 1; y0 = (int)y - 1; z0 = (int)z - 1;
}

// ---------------------------------------------------------------- one cell
// The eight corners of cell (x0, y0, z0) by the vol_get rule (0 outside the grid), c = 4 dx + 2 dy + dz:
// vol_sample's v000 v001 v010 v011 v100 v101 v110 v111, the order of a cells record.
PT_HD void vol_cell_corners(const DevVolume& v, int x0, int y0, int z0, double c[8]) {
    for (int k = 0; k < 8; k++) c[k] = vol_get(v, x0 + (k >> 2), y0 + (k >> 1 & 1), z0 + (k & 1));
}
PT_HD int vol_sign_of_band(const DevVolume& v, int b) { return (b & 1) ? 0 : (b == 2 * v.nwin ? v.nwin + 1 : 1); }
// DevVolume::zero_sign: the Sign of a cell with every corner outside the grid
PT_HD int32_t vol_zero_sign(const DevVolume& v) { return vol_sign_of_band(v, vol_band(v, 0.0)); }
// The cell's byte in the runs table from its corners: the Sign every sample inside the cell has, or 0 for "cannot
// vouch".  The corner range, widened by a margin far above the interpolation's rounding, must lie in one band; a
// NaN or infinite corner can interpolate to NaN (Sign 0); a Sign past int8 (above every window of 127 or more) is
// stored as 0, "no shortcut".  Reads v's windows and nwin only.
PT_HD int8_t vol_cell_sign(const DevVolume& v, const double c[8]) {
    double mn = c[0], mx = c[0];
    bool finite = true;
    for (int k = 0; k < 8; k++) {
        const double g = c[k];
        finite = finite && isfinite(g);
        if (g < mn) mn = g;
        if (g > mx) mx = g;
    }
    const double margin = 1e-9 * (1.0 + fabs(mn) + fabs(mx));
    const int b0 = vol_band(v, mn - margin), b1 = vol_band(v, mx + margin);
    const int sg = (finite && b0 == b1) ? vol_sign_of_band(v, b0) : 0;
    return (int8_t)(sg > 127 ? 0 : sg);
}

// ---------------------------------------------------------------- the upload's loops
// Host: fill out[vol_cell_index(x0, y0, z0)] for every cell of the lattice (a cell outside it has every corner
// outside the grid: zero_sign).
inline void vol_build_runs(const DevVolume& v, int8_t* out, int32_t& zero_sign) {
    zero_sign = vol_zero_sign(v);
    uint64_t i = 0;
    for (int z0 = -1; z0 < v.d; z0++)
        for (int y0 = -1; y0 < v.h; y0++)
            for (int x0 = -1; x0 < v.w; x0++, i++) {
                double c[8];
                vol_cell_corners(v, x0, y0, z0, c);
                out[i] = vol_cell_sign(v, c);
            }
}
// Host: fill out[vol_cell_first(i) + c] = corner c of cell i, the runs table's cells.
inline void vol_build_cells(const DevVolume& v, double* out) {
    uint64_t i = 0;
    for (int z0 = -1; z0 < v.d; z0++)
        for (int y0 = -1; y0 < v.h; y0++)
            for (int x0 = -1; x0 < v.w; x0++, i++) vol_cell_corners(v, x0, y0, z0, out + vol_cell_first(i));
}

// ---------------------------------------------------------------- pt_update_volumes, host side
// What the context keeps of an uploaded Volume: its header (the pointer fields unused) and its window rows as the
// device holds them now.
struct VolState {
    DevVolume v;
    const DevWindow* windows;   // [v.nwin]
};
// The argument check: PT_OK, or PT_ERR_INVALID_ARG with *why naming the argument.  vols: the uploaded scene's.
inline int vol_update_check(const pt_volume_update* u, int32_t num_volumes, const VolState* vols, const char** why) {
    auto bad = [&](const char* w) { *why = w; return (int)PT_ERR_INVALID_ARG; };
    if (!u) return bad("u is NULL");
    if (u->reserved[0] != 0 || u->reserved[1] != 0 || u->reserved[2] != 0) return bad("reserved must be 0");
    if (u->num_volumes != num_volumes) return bad("num_volumes differs from the uploaded scene's");
    if (!u->windows) return PT_OK;
    for (int32_t i = 0; i < num_volumes; i++) {
        const pt_volume_window* w = u->windows[i];
        if (!w) continue;
        for (int32_t k = 0; k < vols[i].v.nwin; k++)
            if (w[k].material != vols[i].windows[k].mat) return bad("a window's material differs from the uploaded one");
    }
    return PT_OK;
}
// True when the update changes something: a volume with new voxels or new windows.
inline bool vol_update_any(const pt_volume_update* u) {
    for (int32_t i = 0; i < u->num_volumes; i++)
        if ((u->data && u->data[i]) || (u->windows && u->windows[i])) return true;
    return false;
}

// Scene.Add's light test (Scene.cs:29-38) of a Volume, or of a TransformedShape over one: MaterialAt(new Vector())
// .Emittance > 0.  TransformedShape.MaterialAt hands the point to its shape unmapped (TransformedShape.cs:84-87), so
// both test the Volume at the origin.  There Volume.Sample reads no voxel: z / zscale is 0 (or NaN, which samples
// 0), and Sample's y-from-z slip makes the z index ((0 + 2) / 2) d = d, past the last slice, so all eight corners
// are outside the grid and the sample is 0 whatever the data.  The material therefore depends on the windows alone,
// and vol_material runs on a host view without voxels.  vol_origin_reads_nothing states that premise as a test of
// the view; the material is taken only where it holds.
inline bool vol_origin_reads_nothing(const DevVolume& v) {
    const double z = vol_zdiv(v, 0.0);
    const double x = ((0.0 + 1) / 2) * (double)v.w, y = ((z + 1) / 2) * (double)v.h, zz = ((z + 2) / 2) * (double)v.d;
    const double lim = 2147483647.0;
    if (!(fabs(x) < lim && fabs(y) < lim && fabs(zz) < lim)) return true;   // Sample returns 0 before any read
    const int x0 = (int)floor(x), y0 = (int)floor(y), z0 = (int)floor(zz);
    for (int k = 0; k < 8; k++) {
        const int cx = x0 + (k >> 2), cy = y0 + (k >> 1 & 1), cz = z0 + (k & 1);
        if (cx >= 0 && cy >= 0 && cz >= 0 && cx < v.w && cy < v.h && cz < v.d) return false;
    }
    return true;
}
// MaterialAt(origin) of the volume with header hdr and window rows win; false when the premise above fails.
inline bool vol_origin_material(const DevVolume& hdr, const DevWindow* win, int32_t default_mat, int32_t& mat) {
    DevVolume v = hdr;
    v.data = nullptr; v.runs = nullptr; v.cells = nullptr;
    v.windows = win;
    if (!vol_origin_reads_nothing(v)) return false;
    mat = vol_material(v, v3{0.f, 0.f, 0.f}, default_mat);
    return true;
}
// A Scene.Shapes slot that is a Volume or a TransformedShape over one: its volume, and the lights entry the upload
// (or the last pt_update_materials) registered for it (-1: not a light).
struct VolLightSlot {
    int32_t volume, light;
};
inline bool vol_emissive(int32_t mat, const double* emittance, int32_t num_materials) {
    return mat >= 0 && mat < num_materials && emittance[mat] > 0;
}
// The light test of every slot with the windows an update would leave (win[i]: volume i's rows).  PT_OK and
// mats[s] = the slot's MaterialAt(origin), or PT_ERR_UNSUPPORTED when a slot's membership would differ from the
// current set's (the upload's, or the one the last pt_update_materials left).  emittance: [num_materials], the scene's own materials (`new Material()`, default_mat = num_materials,
// does not emit).
inline int vol_update_lights(const VolLightSlot* slots, size_t num_slots, const DevVolume* hdrs, const DevWindow* const* win,
                             const double* emittance, int32_t num_materials, int32_t* mats, const char** why) {
    for (size_t s = 0; s < num_slots; s++) {
        const int32_t i = slots[s].volume;
        int32_t m = num_materials;
        if (!vol_origin_material(hdrs[i], win[i], num_materials, m)) {
            *why = "a Volume whose sample at the origin reads voxels: upload the scene again";
            return (int)PT_ERR_UNSUPPORTED;
        }
        if (mats) mats[s] = m;
        const bool lit = vol_emissive(m, emittance, num_materials);
        if (lit != (slots[s].light >= 0)) {
            *why = lit ? "a Volume that is no light now would become one: pt_update_materials or an upload changes the lights"
                       : "a Volume that is a light now would stop being one: pt_update_materials or an upload changes the lights";
            return (int)PT_ERR_UNSUPPORTED;
        }
    }
    return PT_OK;
}

}  // namespace pt
