// eyes_msaa_host.cpp -- the device functions of the eye kernels (eye_msaa_cover and eye_msaa_shade of nb_eyes_msaa.inc, eye_edge,
// eye_cover and eye_shade of nb_eyes.inc, the vertices, clip, depth, fragment and sRGB bytes of nb_raster.inc) compiled for the HOST
// and driven sample by sample, so that tests/test_eyes_msaa_host.py can compare their arithmetic with the rule's restatements
// without a GPU.  The three files are included whole (their kernels and launchers sit behind __HIPCC__); the few device builtins
// they use are stated below.  Build with -ffp-contract=off -msse2 -mfpmath=sse: one binary32 operation per step, as on the device.
// usage: eyes_msaa_host E N FIRST WIDTH SEE_SELF TW TH CAMS.bin INST.bin SKIN.bin OUT.bin [one]   (TW = 0: the white skin;
// one: the one-sample rows -- keys by eye_cover, colour by eye_shade -- where the default is the 8-sample ones)
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
#include "nb_eyes_msaa.inc"
static std::vector<char> slurp(const char *p) { FILE *f = fopen(p, "rb"); if (!f) exit(9); fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET); std::vector<char> b(n); if (fread(b.data(), 1, n, f) != (size_t)n) exit(9); fclose(f); return b; }
int main(int argc, char **argv)
{
    if (argc < 12) return 2;
    const uint32_t E = atoi(argv[1]), n = atoi(argv[2]), first = atoi(argv[3]), width = atoi(argv[4]), see_self = atoi(argv[5]), tw = atoi(argv[6]), th = atoi(argv[7]);
    auto cb = slurp(argv[8]), ib = slurp(argv[9]);
    std::vector<char> sb; if (tw) sb = slurp(argv[10]);
    const float4 *cams = (const float4 *)cb.data(), *inst = (const float4 *)ib.data(), *skin = tw ? (const float4 *)sb.data() : nullptr;
    const float h = (float)width * 0.5f;
    const bool one = argc > 12 && !strcmp(argv[12], "one");
    const uint32_t samples = one ? 1 : 8;
    FILE *out = fopen(argv[11], "wb");
    std::vector<uint64_t> keys(width * samples);
    std::vector<uint32_t> ids8(width * samples), bg(width); std::vector<float> d8(width * samples); std::vector<float4> rg(width);
    for (uint32_t e = 0; e < E; ++e) {
        for (auto &k : keys) k = ~0ull;
        float C[16];
        raster_load16(cams + (size_t)e * 4, C);
        for (uint32_t j = 0; j < n; ++j) {
            if (!see_self && j == first + e) continue;
            float P[3][4];
            if (!raster_vertices_culled(C, inst, j, P)) continue;   // as eyes_kernel: the z row first, the cull
            for (int k = 0; k < 3; ++k) {
                EyeSeg s{};
                if (!eye_edge(P[k], P[k == 2 ? 0 : k + 1], h, width, s)) continue;
                for (uint32_t c = s.lo; c < s.hi; ++c) {
                    if (one) eye_cover(keys.data(), c, s, j);
                    else for (uint32_t m = 0; m < 8; ++m) eye_msaa_cover(keys.data(), c, m, s, j);
                }
            }
        }
        for (uint32_t i = 0; i < width * samples; ++i) { ids8[i] = raster_key_id(keys[i]); d8[i] = raster_key_depth(keys[i]); }
        for (uint32_t c = 0; c < width; ++c) {
            const float4 px = one ? eye_shade(keys[c], c, C, inst, h, width, skin, tw, th) : eye_msaa_shade(keys.data(), c, C, inst, h, width, skin, tw, th);
            rg[c] = px;
            bg[c] = raster_bgra8(kSrgbEncodeT, px);
        }
        fwrite(ids8.data(), 4, ids8.size(), out); fwrite(d8.data(), 4, d8.size(), out); fwrite(rg.data(), 16, rg.size(), out); fwrite(bg.data(), 4, bg.size(), out);
    }
    fclose(out);
    return 0;
}
