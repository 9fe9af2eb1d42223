// frame_msaa_host.cpp -- the device functions of the 8-sample frame kernels (frame_msaa_step, frame_msaa_cover, frame_msaa_shade of
// nb_frame_msaa.inc, with frame_edge of nb_frame.inc, eye_msaa_fragment of nb_eyes_msaa.inc and eye_srgb_byte of nb_eyes.inc)
// compiled for the HOST and driven sample by sample, so that tests/test_frame_msaa_host.py can compare their arithmetic with the
// rule's restatement without a GPU.  The test cuts the four includes off before their kernels (which need a device) into
// frame_msaa_parts.inc; the few device builtins they use are stated below.  Build with -ffp-contract=off -msse2 -mfpmath=sse: one
// binary32 operation per step, as on the device.
// usage: frame_msaa_host N WIDTH HEIGHT TW TH CAM.bin INST.bin SKIN.bin OUT.bin   (TW = 0: the white skin)
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
#include "frame_msaa_parts.inc"
static std::vector<char> slurp(const char *p) { FILE *f = fopen(p, "rb"); if (!f) exit(9); fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET); std::vector<char> b(n); if (fread(b.data(), 1, n, f) != (size_t)n) exit(9); fclose(f); return b; }
int main(int argc, char **argv)
{
    if (argc < 10) return 2;
    const uint32_t n = atoi(argv[1]), width = atoi(argv[2]), height = atoi(argv[3]), tw = atoi(argv[4]), th = atoi(argv[5]);
    auto cb = slurp(argv[6]), ib = slurp(argv[7]);
    std::vector<char> sb; if (tw) sb = slurp(argv[8]);
    const float4 *cam = (const float4 *)cb.data(), *inst = (const float4 *)ib.data(), *skin = tw ? (const float4 *)sb.data() : nullptr;
    const float h = (float)width * 0.5f, g = (float)height * 0.5f;
    const float ax[3] = {-1.0f, 1.0f, -1.0f}, ay[3] = {-1.0f, 0.0f, 1.0f};
    const size_t pixels = (size_t)width * height;
    std::vector<uint64_t> keys(pixels * 8, ~0ull);
    float C[16];
    for (int k = 0; k < 4; ++k) { const float4 v = cam[k]; C[4 * k] = v.x, C[4 * k + 1] = v.y, C[4 * k + 2] = v.z, C[4 * k + 3] = v.w; }
    for (uint32_t j = 0; j < n; ++j) {
        float M[16], P[3][4];
        for (int k = 0; k < 4; ++k) { const float4 v = inst[j * 4 + k]; M[4 * k] = v.x, M[4 * k + 1] = v.y, M[4 * k + 2] = v.z, M[4 * k + 3] = v.w; }
        for (int v = 0; v < 3; ++v) {
            float w[4];
            for (int r = 0; r < 4; ++r) { const float t0 = M[r] * ax[v], t1 = M[4 + r] * ay[v], t2 = M[8 + r] * 0.0f, t3 = M[12 + r] * 1.0f; w[r] = ((t0 + t1) + t2) + t3; }
            for (int r = 0; r < 4; ++r) { const float t0 = C[r] * w[0], t1 = C[4 + r] * w[1], t2 = C[8 + r] * w[2], t3 = C[12 + r] * w[3]; P[v][r] = ((t0 + t1) + t2) + t3; }
        }
        for (int k = 0; k < 3; ++k) {
            FrameSeg s{};
            if (!frame_edge(P[k], P[k == 2 ? 0 : k + 1], h, g, width, height, s)) continue;
            for (uint32_t m = s.lo; m < s.hi; ++m) for (uint32_t q = 0; q < 8; ++q) frame_msaa_cover(keys.data(), m, q, s, j, width);
        }
    }
    std::vector<uint32_t> ids8(pixels * 8), bg(pixels); std::vector<float> d8(pixels * 8); std::vector<float4> rg(pixels);
    for (size_t i = 0; i < pixels * 8; ++i) { const bool none = keys[i] == ~0ull; ids8[i] = none ? 0xFFFFFFFFu : (uint32_t)keys[i]; d8[i] = none ? 1.0f : __uint_as_float((uint32_t)(keys[i] >> 32)); }
    for (uint32_t p = 0; p < pixels; ++p) {
        const float4 px = frame_msaa_shade(keys.data() + (size_t)p * 8, p % width, p / width, C, inst, width, height, skin, tw, th);
        rg[p] = px;
        bg[p] = eye_srgb_byte(kSrgbEncodeT, px.z) | eye_srgb_byte(kSrgbEncodeT, px.y) << 8 | eye_srgb_byte(kSrgbEncodeT, px.x) << 16 | 0xFF000000u;
    }
    FILE *out = fopen(argv[9], "wb");
    fwrite(ids8.data(), 4, ids8.size(), out); fwrite(d8.data(), 4, d8.size(), out); fwrite(rg.data(), 16, rg.size(), out); fwrite(bg.data(), 4, bg.size(), out);
    fclose(out);
    return 0;
}
