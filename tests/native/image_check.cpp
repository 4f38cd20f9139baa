// image_check — the host build of ptsharp_amd/csrc/pt_image.h, the per-pixel text k_image_resolve
// runs on the device (tests/test_image_host.py compiles and runs it; plain g++, no HIP).
//
//   image_check IN OUT
//
// IN:  int32 W, int32 H, then M [H*W*3] float64, V [H*W*3] float64, N [H*W] int32 (native endian).
// OUT: the six channels' RGB images in pt_channel order, each [H*W*3] bytes.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../ptsharp_amd/csrc/pt_image.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: image_check IN OUT\n");
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 1; }
    int32_t wh[2] = {0, 0};
    if (std::fread(wh, sizeof(int32_t), 2, in) != 2 || wh[0] < 1 || wh[1] < 1) {
        std::fprintf(stderr, "bad header\n");
        return 1;
    }
    const int32_t W = wh[0], H = wh[1];
    const size_t P = (size_t)W * (size_t)H;
    std::vector<double> m(3 * P), v(3 * P);
    std::vector<int32_t> n(P);
    if (std::fread(m.data(), sizeof(double), 3 * P, in) != 3 * P || std::fread(v.data(), sizeof(double), 3 * P, in) != 3 * P ||
        std::fread(n.data(), sizeof(int32_t), P, in) != P) {
        std::fprintf(stderr, "short input\n");
        return 1;
    }
    std::fclose(in);
    int32_t max_n = 0;   // k_image_max_n: max(0, max N)
    for (size_t i = 0; i < P; i++) max_n = n[i] > max_n ? n[i] : max_n;
    std::vector<uint8_t> out(3 * P * pt::kChCount);
    for (int ch = 0; ch < pt::kChCount; ch++)
        for (size_t i = 0; i < P; i++)
            pt::image_resolve_at(ch, m.data(), v.data(), n.data(), W, H, max_n, i, &out[((size_t)ch * P + i) * 3]);
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 1; }
    const bool ok = std::fwrite(out.data(), 1, out.size(), o) == out.size();
    return std::fclose(o) == 0 && ok ? 0 : 1;
}
