// frame_msaa_host.cpp -- the device functions of the frame kernels (frame_msaa_step, frame_msaa_cover and frame_msaa_shade of
// nb_frame_msaa.inc, frame_edge, frame_cover and frame_shade of nb_frame.inc, the vertices, clip, depth, fragment and sRGB bytes of
// nb_raster.inc) compiled for the HOST and driven sample by sample, so that tests/test_frame_msaa_host.py can compare their
// arithmetic with the rule's restatements without a GPU.  The files are included whole (their kernels and launchers sit behind
// __HIPCC__); the few device builtins they use are stated below.  Build with -ffp-contract=off -msse2 -mfpmath=sse: one binary32
// operation per step, as on the device.
// usage: frame_msaa_host N WIDTH HEIGHT TW TH CAM.bin INST.bin SKIN.bin OUT.bin [one]   (TW = 0: the white skin; one: the
// one-sample frame -- keys by frame_cover, colour by frame_shade -- where the default is the 8-sample one)
#include <cstdint>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __HIP_MEMORY_SCOPE_WORKGROUP 0
#define __HIP_MEMORY_SCOPE_AGENT 1
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline int __float_as_int(float f) { int u; memcpy(&u, &f, 4); return u; }
static inline float __int_as_float(int u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint64_t __hip_atomic_load(uint64_t *p, int, int) { return *p; }
static inline void __hip_atomic_fetch_min(uint64_t *p, uint64_t v, int, int) { if (v < *p) *p = v; }
static inline int __builtin_amdgcn_readlane(int v, int) { return v; }
#include "nb_raster.inc"
#include "nb_eyes.inc"
#include "nb_frame.inc"
#include "nb_eyes_msaa.inc"
#include "nb_frame_msaa.inc"
static std::vector<char> slurp(const char *p) { FILE *f = fopen(p, "rb"); if (!f) exit(9); fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET); std::vector<char> b(n); if (fread(b.data(), 1, n, f) != (size_t)n) exit(9); fclose(f); return b; }
int main(int argc, char **argv)
{
    if (argc < 10) return 2;
    const uint32_t n = atoi(argv[1]), width = atoi(argv[2]), height = atoi(argv[3]), tw = atoi(argv[4]), th = atoi(argv[5]);
    auto cb = slurp(argv[6]), ib = slurp(argv[7]);
    std::vector<char> sb; if (tw) sb = slurp(argv[8]);
    const float4 *cam = (const float4 *)cb.data(), *inst = (const float4 *)ib.data(), *skin = tw ? (const float4 *)sb.data() : nullptr;
    const float h = (float)width * 0.5f, g = (float)height * 0.5f;
    const bool one = argc > 10 && !strcmp(argv[10], "one");
    const size_t pixels = (size_t)width * height, samples = one ? 1 : 8;
    std::vector<uint64_t> keys(pixels * samples, ~0ull);
    float C[16];
    raster_load16(cam, C);
    for (uint32_t j = 0; j < n; ++j) {
        float P[3][4];
        if (!raster_vertices_culled(C, inst, j, P)) continue;   // as the edges kernels: the z row first, the cull
        for (int k = 0; k < 3; ++k) {
            FrameSeg s{};
            if (!frame_edge(P[k], P[k == 2 ? 0 : k + 1], h, g, width, height, s)) continue;
            for (uint32_t m = s.lo; m < s.hi; ++m) {
                if (one) frame_cover(keys.data(), m, s, j, width);
                else for (uint32_t q = 0; q < 8; ++q) frame_msaa_cover(keys.data(), m, q, s, j, width);
            }
        }
    }
    std::vector<uint32_t> ids8(pixels * samples), bg(pixels); std::vector<float> d8(pixels * samples); std::vector<float4> rg(pixels);
    for (size_t i = 0; i < pixels * samples; ++i) { ids8[i] = raster_key_id(keys[i]); d8[i] = raster_key_depth(keys[i]); }
    for (uint32_t p = 0; p < pixels; ++p) {
        const float4 px = one ? frame_shade(keys[p], p % width, p / width, C, inst, width, height, skin, tw, th)
                              : frame_msaa_shade(keys.data() + (size_t)p * 8, p % width, p / width, C, inst, width, height, skin, tw, th);
        rg[p] = px;
        bg[p] = raster_bgra8(kSrgbEncodeT, px);
    }
    FILE *out = fopen(argv[9], "wb");
    fwrite(ids8.data(), 4, ids8.size(), out); fwrite(d8.data(), 4, d8.size(), out); fwrite(rg.data(), 16, rg.size(), out); fwrite(bg.data(), 4, bg.size(), out);
    fclose(out);
    return 0;
}
