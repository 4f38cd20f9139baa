// denoise_guided_check — the host build of the guided level of ptsharp_amd/csrc/pt_denoise.h, the
// per-pixel text pt_denoise_guided's kernels run on the device (tests/test_features_host.py compiles
// and runs it; plain g++, no HIP).
//
//   denoise_guided_check IN OUT
//
// IN:  int32 W, int32 H, int32 iterations, int32 0, float64 sigma_colour, sigma_normal, sigma_albedo,
//      sigma_depth, then M [H*W*3] float64, V [H*W*3] float64, N [H*W] int32, albedo [H*W*3] float64,
//      normal [H*W*3] float32, depth [H*W] float64, kind [H*W] int32 (native endian).
// OUT: the denoised colour [H*W*3] float64, then the propagated variance [H*W*3] float64.
//
// The passes are launch_denoise_guided's: prepare, blur, then the guided levels at steps 1, 2, 4, ...
// between two {c, s2} pairs; the guide records are packed as the device packs them (fp32 normal,
// (float)depth, (float)albedo, hit = kind >= 0).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../ptsharp_amd/csrc/pt_denoise.h"

template <class T>
static bool read_all(std::FILE* f, std::vector<T>& a) {
    return std::fread(a.data(), sizeof(T), a.size(), f) == a.size();
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: denoise_guided_check IN OUT\n");
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 1; }
    int32_t head[4] = {0, 0, 0, 0};
    double sig[4] = {0.0, 0.0, 0.0, 0.0};
    if (std::fread(head, sizeof(int32_t), 4, in) != 4 || std::fread(sig, sizeof(double), 4, in) != 4 || head[0] < 1 ||
        head[1] < 1 || head[2] < 1 || head[2] > 8 || head[3] != 0 || !(sig[0] > 0.0) || !(sig[1] >= 0.0) || !(sig[2] >= 0.0) ||
        !(sig[3] >= 0.0)) {
        std::fprintf(stderr, "bad header\n");
        return 1;
    }
    const int32_t W = head[0], H = head[1], iterations = head[2];
    const size_t P = (size_t)W * (size_t)H;
    std::vector<double> m(3 * P), v(3 * P), albedo(3 * P), depth(P);
    std::vector<float> normal(3 * P);
    std::vector<int32_t> n(P), kind(P);
    if (!read_all(in, m) || !read_all(in, v) || !read_all(in, n) || !read_all(in, albedo) || !read_all(in, normal) ||
        !read_all(in, depth) || !read_all(in, kind)) {
        std::fprintf(stderr, "short input\n");
        return 1;
    }
    std::fclose(in);
    std::vector<pt::DenoiseGuideRec> guide(P);
    for (size_t p = 0; p < P; p++) {
        pt::DenoiseGuideRec& g = guide[p];
        for (int k = 0; k < 3; k++) {
            g.n[k] = normal[3 * p + k];
            g.a[k] = (float)albedo[3 * p + k];
        }
        g.depth = (float)depth[p];
        g.hit = kind[p] >= 0 ? 1.f : 0.f;
    }
    const pt::DenoiseGuideSigmas sg{sig[2] * sig[2], sig[1] * sig[1], sig[3]};   // albedo², normal², depth
    std::vector<double> c[2] = {std::vector<double>(3 * P), std::vector<double>(3 * P)};
    std::vector<double> s2[2] = {std::vector<double>(3 * P), std::vector<double>(3 * P)};
    std::vector<uint8_t> valid(P);
    for (int32_t y = 0; y < H; y++)
        for (int32_t x = 0; x < W; x++) {
            const size_t p = pt::denoise_index(W, x, y);
            valid[p] = pt::denoise_prepare_at(m.data(), v.data(), n.data(), W, H, x, y, &c[0][3 * p], &s2[1][3 * p]) ? 1 : 0;
        }
    for (int32_t y = 0; y < H; y++)
        for (int32_t x = 0; x < W; x++)
            pt::denoise_blur_at(s2[1].data(), valid.data(), W, H, x, y, &s2[0][3 * pt::denoise_index(W, x, y)]);
    const double sigma2 = sig[0] * sig[0];
    int src = 0;
    for (int32_t j = 0; j < iterations; j++, src ^= 1)
        for (int32_t y = 0; y < H; y++)
            for (int32_t x = 0; x < W; x++) {
                const size_t p = pt::denoise_index(W, x, y);
                pt::denoise_level_guided_at(c[src].data(), s2[src].data(), valid.data(), guide.data(), W, H, x, y, (int32_t)1 << j,
                                            sigma2, sg, &c[src ^ 1][3 * p], &s2[src ^ 1][3 * p]);
            }
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 1; }
    const bool ok = std::fwrite(c[src].data(), sizeof(double), 3 * P, o) == 3 * P &&
                    std::fwrite(s2[src].data(), sizeof(double), 3 * P, o) == 3 * P;
    return std::fclose(o) == 0 && ok ? 0 : 1;
}
