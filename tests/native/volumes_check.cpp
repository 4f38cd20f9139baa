// volumes_check — pt_volume_update.h on the host (no GPU): the per-cell functions that both the upload's loops and
// the kernels of pt_update_volumes run, driven cell by cell through the index functions the kernel uses, against a
// plain restatement, written here, of the table loops the upload had before the two shared one statement; then
// zero_sign, the argument check's every refusal, the light test, and the 64-bit index arithmetic.
//   volumes_check             prints "case <name> ok" per case and "volumes_check: <n> failures"
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "pt_volume_update.h"

using namespace pt;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (g_fail < 40) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
            g_fail++;                                                        \
        }                                                                    \
    } while (0)

// ---- the old loops, restated (what pt_ext.h's vol_build_runs / vol_build_cells were)
static double old_get(const std::vector<double>& g, int w, int h, int d, int x, int y, int z) {
    if (x < 0 || y < 0 || z < 0 || x >= w || y >= h || z >= d) return 0;
    return g[(size_t)x + (size_t)y * (size_t)w + (size_t)z * (size_t)w * (size_t)h];
}
static int old_band(const std::vector<DevWindow>& win, double s) {
    const int n = (int)win.size();
    for (int i = 0; i < n; i++) {
        if (s < win[(size_t)i].lo) return 2 * i;
        if (s <= win[(size_t)i].hi) return 2 * i + 1;
    }
    return 2 * n;
}
static int old_sign_of_band(const std::vector<DevWindow>& win, int b) {
    const int n = (int)win.size();
    return (b & 1) ? 0 : (b == 2 * n ? n + 1 : 1);
}
static void old_runs(const std::vector<double>& g, int w, int h, int d, const std::vector<DevWindow>& win, std::vector<int8_t>& out,
                     int32_t& zero_sign) {
    const int sx = w + 1, sy = h + 1;
    out.assign((size_t)sx * sy * (d + 1), 99);
    zero_sign = old_sign_of_band(win, old_band(win, 0.0));
    for (int z0 = -1; z0 < d; z0++)
        for (int y0 = -1; y0 < h; y0++)
            for (int x0 = -1; x0 < w; x0++) {
                double mn = 0, mx = 0;
                bool first = true, finite = true;
                for (int c = 0; c < 8; c++) {
                    const double v = old_get(g, w, h, d, x0 + (c >> 2 & 1), y0 + (c >> 1 & 1), z0 + (c & 1));
                    finite = finite && isfinite(v);
                    if (first || v < mn) mn = v;
                    if (first || v > mx) mx = v;
                    first = false;
                }
                const double margin = 1e-9 * (1.0 + fabs(mn) + fabs(mx));
                const int b0 = old_band(win, mn - margin), b1 = old_band(win, mx + margin);
                const int sg = (finite && b0 == b1) ? old_sign_of_band(win, b0) : 0;
                out[(size_t)(x0 + 1) + (size_t)(y0 + 1) * sx + (size_t)(z0 + 1) * sx * sy] = (int8_t)(sg > 127 ? 0 : sg);
            }
}
static void old_cells(const std::vector<double>& g, int w, int h, int d, std::vector<double>& out) {
    out.assign(8 * (size_t)(w + 1) * (h + 1) * (d + 1), -7.0);
    size_t i = 0;
    for (int z0 = -1; z0 < d; z0++)
        for (int y0 = -1; y0 < h; y0++)
            for (int x0 = -1; x0 < w; x0++, i++)
                for (int c = 0; c < 8; c++) out[8 * i + (size_t)c] = old_get(g, w, h, d, x0 + (c >> 2), y0 + (c >> 1 & 1), z0 + (c & 1));
}

// ---- inputs
static uint64_t g_rng = 0;
static double rnd() {   // [0, 1)
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_rng >> 11) * (1.0 / 9007199254740992.0);
}
static std::vector<double> seeded_grid(int w, int h, int d, uint64_t seed) {
    g_rng = seed;
    std::vector<double> g((size_t)w * h * d);
    // smooth-ish: a ramp plus noise, so that many cells are uniform and many straddle a window
    for (int z = 0; z < d; z++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
                g[(size_t)x + (size_t)y * w + (size_t)z * w * h] = 0.8 * (double)(x + y + z) / (double)(w + h + d) + 0.1 * rnd();
    return g;
}
static DevWindow W(double lo, double hi, int mat) { return DevWindow{lo, hi, mat, 0}; }
struct WindowSet {
    const char* name;
    std::vector<DevWindow> win;
};
static std::vector<WindowSet> window_sets() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<WindowSet> s;
    s.push_back({"none", {}});
    WindowSet ex{"example", {}};   // Example.volume's five: start 0.2, size 0.01, step 0.1, in its fp32 arithmetic
    for (int i = 0; i < 5; i++) {
        const double lo = (double)(0.2f + 0.1f * (float)i);
        ex.win.push_back(W(lo, (double)((float)lo + 0.01f), i));
    }
    s.push_back(ex);
    s.push_back({"overlapping-unsorted", {W(0.5, 0.7, 0), W(0.1, 0.55, 1), W(0.6, 0.2, 2), W(0.3, 0.3, 3), W(-1.0, 0.05, 4)}});
    WindowSet many{"130-windows", {}};   // a Sign above every window is 131, past int8: stored 0
    for (int i = 0; i < 130; i++) many.win.push_back(W(-2.0 - 0.001 * i, -2.0 - 0.001 * i + 0.0005, i % 7));
    s.push_back(many);
    s.push_back({"on-the-bounds", {W(0.25, 0.5, 0), W(0.5, 0.75, 1)}});   // the grid gets voxels exactly 0.25, 0.5, 0.75
    s.push_back({"non-finite-bounds", {W(-inf, 0.1, 0), W(nan, 0.3, 1), W(0.4, nan, 2), W(0.6, inf, 3)}});
    return s;
}

// A host view: a DevVolume over host arrays (zscale, box: not read by the tables)
static DevVolume view(const std::vector<double>& g, int w, int h, int d, const std::vector<DevWindow>& win) {
    DevVolume v{};
    v.data = g.data(); v.windows = win.data();
    v.w = w; v.h = h; v.d = d; v.nwin = (int32_t)win.size();
    v.zscale = 1.0; v.zinv = 0.0;
    return v;
}

static void compare_tables(const std::string& name, const std::vector<double>& g, int w, int h, int d, const std::vector<DevWindow>& win) {
    const int before = g_fail;
    std::vector<int8_t> want_runs;
    std::vector<double> want_cells;
    int32_t want_zero = -1;
    old_runs(g, w, h, d, win, want_runs, want_zero);
    old_cells(g, w, h, d, want_cells);
    const DevVolume v = view(g, w, h, d, win);
    const uint64_t n = vol_cell_count(w, h, d);
    CHECK(n == want_runs.size(), "%s: %llu cells, the old loop has %zu", name.c_str(), (unsigned long long)n, want_runs.size());
    CHECK(vol_zero_sign(v) == want_zero, "%s: zero_sign %d, want %d", name.c_str(), vol_zero_sign(v), want_zero);
    // cell by cell, as the kernel walks: linear index -> coordinates -> corners -> record and sign
    for (uint64_t i = 0; i < n; i++) {
        int x0, y0, z0;
        vol_cell_coords(w, h, i, x0, y0, z0);
        CHECK(vol_cell_index(w, h, x0, y0, z0) == i, "%s: cell %llu -> (%d %d %d) -> %llu", name.c_str(), (unsigned long long)i, x0, y0,
              z0, (unsigned long long)vol_cell_index(w, h, x0, y0, z0));
        double c[8];
        vol_cell_corners(v, x0, y0, z0, c);
        CHECK(memcmp(c, &want_cells[vol_cell_first(i)], 64) == 0, "%s: cell %llu corners differ", name.c_str(), (unsigned long long)i);
        CHECK(vol_cell_byte(i) == 8 * sizeof(double) * i, "%s: byte offset", name.c_str());
        const int8_t sg = vol_cell_sign(v, c);
        CHECK(sg == want_runs[i], "%s: cell %llu (%d %d %d) sign %d, want %d", name.c_str(), (unsigned long long)i, x0, y0, z0, sg,
              want_runs[i]);
        // the windows-only kernel takes the corners from the record: the same sign
        CHECK(vol_cell_sign(v, &want_cells[vol_cell_first(i)]) == want_runs[i], "%s: cell %llu sign from its record", name.c_str(),
              (unsigned long long)i);
    }
    // the upload's loops over them
    std::vector<int8_t> runs(n, 99);
    std::vector<double> cells(8 * n, -7.0);
    int32_t zero = -1;
    vol_build_runs(v, runs.data(), zero);
    vol_build_cells(v, cells.data());
    CHECK(zero == want_zero, "%s: vol_build_runs zero_sign %d, want %d", name.c_str(), zero, want_zero);
    CHECK(memcmp(runs.data(), want_runs.data(), n) == 0, "%s: vol_build_runs differs from the old loop", name.c_str());
    CHECK(memcmp(cells.data(), want_cells.data(), 64 * n) == 0, "%s: vol_build_cells differs from the old loop", name.c_str());
    if (g_fail == before) printf("case %s ok\n", name.c_str());
}

static void table_cases() {
    const int dims[4][3] = {{1, 1, 1}, {2, 3, 5}, {17, 9, 5}, {24, 24, 12}};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const std::vector<WindowSet> sets = window_sets();
    for (int k = 0; k < 4; k++) {
        const int w = dims[k][0], h = dims[k][1], d = dims[k][2];
        const std::string dn = std::to_string(w) + "x" + std::to_string(h) + "x" + std::to_string(d);
        std::vector<double> g = seeded_grid(w, h, d, 1000 + (uint64_t)k);
        for (const WindowSet& s : sets) {
            std::vector<double> gg = g;
            if (!strcmp(s.name, "on-the-bounds"))   // voxels exactly on a lo and a hi
                for (size_t i = 0; i < gg.size(); i++) gg[i] = i % 5 == 0 ? 0.25 : i % 5 == 1 ? 0.5 : i % 5 == 2 ? 0.75 : gg[i];
            compare_tables(dn + " " + s.name, gg, w, h, d, s.win);
        }
        // NaN and infinite voxels, first corner and later corners, with the example windows and the non-finite bounds
        std::vector<double> bad = g;
        for (size_t i = 0; i < bad.size(); i += 7) bad[i] = i % 3 == 0 ? nan : i % 3 == 1 ? inf : -inf;
        bad[0] = nan;
        bad[bad.size() - 1] = -inf;
        compare_tables(dn + " non-finite-voxels example", bad, w, h, d, sets[1].win);
        compare_tables(dn + " non-finite-voxels non-finite-bounds", bad, w, h, d, sets[5].win);
        compare_tables(dn + " non-finite-voxels none", bad, w, h, d, sets[0].win);
    }
    // the sign past int8: above 130 windows the Sign is 131, stored as 0; zero_sign itself is not clipped
    {
        const std::vector<DevWindow>& many = sets[3].win;
        const std::vector<double> g(8, 0.5);
        const DevVolume v = view(g, 2, 2, 2, many);
        double c[8] = {0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5};
        const int before = g_fail;
        CHECK(vol_cell_sign(v, c) == 0, "a Sign of 131 must store 0, got %d", vol_cell_sign(v, c));
        CHECK(vol_zero_sign(v) == 131, "zero_sign above 130 windows is 131, got %d", vol_zero_sign(v));
        if (g_fail == before) printf("case sign-past-int8 ok\n");
    }
}

// ---- 64-bit indices: dimensions whose cell count times 64 passes 2^32, through the index functions alone
static void index_cases() {
    const int before = g_fail;
    const int dims[4][3] = {{1023, 1023, 511}, {2047, 2047, 2047}, {511, 4095, 8191}, {69999, 69999, 1}};
    for (int k = 0; k < 4; k++) {
        const int w = dims[k][0], h = dims[k][1], d = dims[k][2];
        const unsigned __int128 n128 = (unsigned __int128)(w + 1) * (unsigned __int128)(h + 1) * (unsigned __int128)(d + 1);
        const uint64_t n = vol_cell_count(w, h, d);
        CHECK((unsigned __int128)n == n128, "dims %d: cell count", k);
        CHECK((unsigned __int128)vol_cell_byte(n) == n128 * 64 && vol_cell_byte(n) > 0xffffffffull, "dims %d: bytes must pass 2^32", k);
        g_rng = 77 + (uint64_t)k;
        for (int t = 0; t < 20000; t++) {
            int x0, y0, z0;
            if (t == 0) { x0 = w - 1; y0 = h - 1; z0 = d - 1; }         // the last cell
            else if (t == 1) { x0 = -1; y0 = -1; z0 = -1; }            // the first
            else if (t == 2) { x0 = -1; y0 = -1; z0 = d - 1; }
            else { x0 = (int)(rnd() * (w + 1)) - 1; y0 = (int)(rnd() * (h + 1)) - 1; z0 = (int)(rnd() * (d + 1)) - 1; }
            const unsigned __int128 want = (unsigned __int128)(x0 + 1) + (unsigned __int128)(y0 + 1) * (unsigned)(w + 1) +
                                           (unsigned __int128)(z0 + 1) * (unsigned)(w + 1) * (unsigned __int128)(h + 1);
            const uint64_t i = vol_cell_index(w, h, x0, y0, z0);
            CHECK((unsigned __int128)i == want && i < n, "dims %d: index of (%d %d %d)", k, x0, y0, z0);
            CHECK((unsigned __int128)vol_cell_byte(i) == want * 64 && (unsigned __int128)vol_cell_first(i) == want * 8, "dims %d: offsets", k);
            int x1, y1, z1;
            vol_cell_coords(w, h, i, x1, y1, z1);
            CHECK(x1 == x0 && y1 == y0 && z1 == z0, "dims %d: coords of %llu: (%d %d %d), want (%d %d %d)", k, (unsigned long long)i, x1,
                  y1, z1, x0, y0, z0);
        }
    }
    if (g_fail == before) printf("case index-64-bit ok\n");
}

// ---- the argument check
static void argument_cases() {
    const int before = g_fail;
    std::vector<DevWindow> w0 = {W(0.1, 0.2, 3), W(0.3, 0.4, 5)}, w1 = {W(0.5, 0.6, 1)};
    VolState vols[2];
    vols[0].v = DevVolume{}; vols[0].v.w = 2; vols[0].v.h = 2; vols[0].v.d = 2; vols[0].v.nwin = 2; vols[0].windows = w0.data();
    vols[1].v = DevVolume{}; vols[1].v.w = 3; vols[1].v.h = 1; vols[1].v.d = 1; vols[1].v.nwin = 1; vols[1].windows = w1.data();
    const char* why = nullptr;
    CHECK(vol_update_check(nullptr, 2, vols, &why) == PT_ERR_INVALID_ARG && why, "a NULL u");
    pt_volume_update u{};
    u.num_volumes = 2;
    CHECK(vol_update_check(&u, 2, vols, &why) == PT_OK && !vol_update_any(&u), "both arrays NULL is PT_OK and changes nothing");
    for (int k = 0; k < 3; k++) {
        pt_volume_update r = u;
        r.reserved[k] = 1;
        CHECK(vol_update_check(&r, 2, vols, &why) == PT_ERR_INVALID_ARG, "reserved[%d] != 0", k);
    }
    for (int n : {0, 1, 3, -1}) {
        pt_volume_update r = u;
        r.num_volumes = n;
        CHECK(vol_update_check(&r, 2, vols, &why) == PT_ERR_INVALID_ARG, "num_volumes %d against 2", n);
    }
    const double grid[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    const double* data[2] = {nullptr, nullptr};
    const pt_volume_window* wins[2] = {nullptr, nullptr};
    u.data = data; u.windows = wins;
    CHECK(vol_update_check(&u, 2, vols, &why) == PT_OK && !vol_update_any(&u), "every entry NULL is PT_OK and changes nothing");
    data[0] = grid;
    CHECK(vol_update_check(&u, 2, vols, &why) == PT_OK && vol_update_any(&u), "data for one volume");
    data[0] = nullptr;
    pt_volume_window good0[2] = {{0.15, 0.25, 3, 0}, {0.35, 0.45, 5, 0}}, bad0[2] = {{0.15, 0.25, 3, 0}, {0.35, 0.45, 4, 0}};
    pt_volume_window good1[1] = {{-1.0, std::numeric_limits<double>::quiet_NaN(), 1, 0}}, bad1[1] = {{0.5, 0.6, 0, 0}};
    wins[0] = good0; wins[1] = good1;
    CHECK(vol_update_check(&u, 2, vols, &why) == PT_OK && vol_update_any(&u), "the uploaded materials, any lo and hi");
    wins[0] = bad0;
    CHECK(vol_update_check(&u, 2, vols, &why) == PT_ERR_INVALID_ARG, "a second window's material changed");
    wins[0] = nullptr; wins[1] = bad1;
    CHECK(vol_update_check(&u, 2, vols, &why) == PT_ERR_INVALID_ARG, "the second volume's window material changed");
    pt_volume_update none{};   // a scene without volumes and num_volumes 0
    CHECK(vol_update_check(&none, 0, nullptr, &why) == PT_OK && !vol_update_any(&none), "no volumes");
    if (g_fail == before) printf("case arguments ok\n");
}

// ---- the light test
static void light_cases() {
    const int before = g_fail;
    // materials 0 dull, 1 emits, 2 dull, 3 emits; default_mat = 4
    const double emit[4] = {0.0, 5.0, 0.0, 2.5};
    // the premise: at the origin Sample reads no voxel, whatever the dimensions and zscale
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (int w : {1, 2, 17, 64})
        for (int h : {1, 3, 64})
            for (int d : {1, 5, 32})
                for (double zs : {1.0, 0.5, 3.4816, -2.0, 1e-300, 1e300, 0.0, inf, nan}) {
                    DevVolume v{};
                    v.w = w; v.h = h; v.d = d; v.zscale = zs; v.zinv = vol_zinv(zs);
                    CHECK(vol_origin_reads_nothing(v), "%dx%dx%d zscale %g: the origin's sample would read a voxel", w, h, d, zs);
                    DevVolume q = v;   // and vol_sample agrees: 0 with no grid behind it would crash otherwise, so give it one
                    std::vector<double> ones((size_t)w * h * d, 1.0);
                    q.data = ones.data();
                    CHECK(vol_sample(q, 0.0, 0.0, 0.0) == 0.0, "%dx%dx%d zscale %g: sample at the origin of a grid of ones", w, h, d, zs);
                }
    DevVolume hdr[2];
    for (int i = 0; i < 2; i++) { hdr[i] = DevVolume{}; hdr[i].w = 4 + i; hdr[i].h = 3; hdr[i].d = 2; hdr[i].zscale = 1.5; hdr[i].zinv = vol_zinv(1.5); hdr[i].nwin = 2; }
    // volume 0: window 0 dull around 0.3, window 1 emissive around 0.8: the sample 0 is nearest window 0: no light
    // volume 1: window 0 emissive holding 0: a light (material 3)
    std::vector<DevWindow> a = {W(0.25, 0.35, 0), W(0.75, 0.85, 1)}, b = {W(-0.1, 0.1, 3), W(0.5, 0.6, 2)};
    const DevWindow* win[2] = {a.data(), b.data()};
    // slots: volume 0 top-level (no light), volume 0 through a transform (no light), volume 1 top-level (light 0),
    // volume 1 through a transform (light 1)
    const VolLightSlot slots[4] = {{0, -1}, {0, -1}, {1, 0}, {1, 1}};
    int32_t mats[4] = {-9, -9, -9, -9};
    const char* why = nullptr;
    CHECK(vol_update_lights(slots, 4, hdr, win, emit, 4, mats, &why) == PT_OK, "the uploaded windows keep every membership");
    CHECK(mats[0] == 0 && mats[1] == 0 && mats[2] == 3 && mats[3] == 3, "materials at the origin: %d %d %d %d", mats[0], mats[1], mats[2], mats[3]);
    // an edit that keeps the memberships: volume 0's dull window moves, volume 1's emissive one still holds 0
    std::vector<DevWindow> a2 = {W(0.1, 0.2, 0), W(0.6, 0.9, 1)}, b2 = {W(-0.5, 0.0, 3), W(0.2, 0.3, 2)};
    win[0] = a2.data(); win[1] = b2.data();
    CHECK(vol_update_lights(slots, 4, hdr, win, emit, 4, mats, &why) == PT_OK, "an edit that keeps the memberships");
    // the emissive window's band turned onto the value at the test point: volume 0 would become a light
    std::vector<DevWindow> a3 = {W(0.25, 0.35, 0), W(-0.05, 0.05, 1)};
    win[0] = a3.data(); win[1] = b.data();
    CHECK(vol_update_lights(slots, 4, hdr, win, emit, 4, mats, &why) == PT_ERR_UNSUPPORTED && why, "a dull Volume turned light must be refused");
    CHECK(vol_update_lights(slots + 1, 1, hdr, win, emit, 4, nullptr, &why) == PT_ERR_UNSUPPORTED, "and through a transform");
    // nearest-window rule: no window holds 0, the emissive one is nearer
    std::vector<DevWindow> a4 = {W(0.25, 0.35, 0), W(0.1, 0.15, 1)};
    win[0] = a4.data();
    CHECK(vol_update_lights(slots, 1, hdr, win, emit, 4, mats, &why) == PT_ERR_UNSUPPORTED, "the nearest window emits: refused");
    // a light that would stop being one: volume 1's emissive window dragged off 0, the dull one nearer
    std::vector<DevWindow> b3 = {W(0.7, 0.9, 3), W(0.2, 0.3, 2)};
    win[0] = a.data(); win[1] = b3.data();
    CHECK(vol_update_lights(slots, 4, hdr, win, emit, 4, mats, &why) == PT_ERR_UNSUPPORTED, "a light turned dull must be refused");
    CHECK(vol_update_lights(slots + 3, 1, hdr, win, emit, 4, mats, &why) == PT_ERR_UNSUPPORTED, "and through a transform");
    // windows far beyond 1e9 from 0: `new Material()` (default_mat, never emissive)
    std::vector<DevWindow> a5 = {W(3e9, 4e9, 1), W(-5e9, -4e9, 1)};
    win[0] = a5.data(); win[1] = b.data();
    CHECK(vol_update_lights(slots, 4, hdr, win, emit, 4, mats, &why) == PT_OK && mats[0] == 4, "beyond 1e9: the default material, %d", mats[0]);
    // NaN bounds: no comparison holds, the distance is NaN, never nearer: the default material
    std::vector<DevWindow> a6 = {W(nan, nan, 1), W(nan, nan, 1)};
    win[0] = a6.data();
    CHECK(vol_update_lights(slots, 2, hdr, win, emit, 4, mats, &why) == PT_OK && mats[0] == 4, "NaN bounds: the default material, %d", mats[0]);
    if (g_fail == before) printf("case lights ok\n");
}

int main() {
    table_cases();
    index_cases();
    argument_cases();
    light_cases();
    printf("volumes_check: %d failures\n", g_fail);
    return g_fail ? 1 : 0;
}
