// nb_raster.inc -- the one copy of what the eye rows and the scene camera's frame share (DESIGN.md sections 10 - 11.1): the vertex
// products, the clip, the depth of a parameter, the fragment, the 8-sample mean, the key's halves, the sRGB bytes, the sample offsets.
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit ahead of nb_eyes.inc, nb_frame.inc, nb_eyes_msaa.inc and
// nb_frame_msaa.inc, which add their view's projection, cover, step and shade, their kernels and launchers.  Device functions only.
// Every function below is one binary32 operation per step in the order written (-ffp-contract=off, IEEE '/'): the four files agree
// bit for bit because they call these, and the host-compiled tests (tests/cpp) call them too.

// a column-major 4 x 4 matrix, four 16-byte records
__device__ __forceinline__ void raster_load16(const float4 *__restrict__ m, float *M)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 v = m[k];
        M[4 * k] = v.x, M[4 * k + 1] = v.y, M[4 * k + 2] = v.z, M[4 * k + 3] = v.w;
    }
}

// row r of A (x, y, z, w): ((a0 x + a1 y) + a2 z) + a3 w
__device__ __forceinline__ float raster_row(const float *A, int r, float x, float y, float z, float w)
{
    const float t0 = A[r] * x, t1 = A[4 + r] * y, t2 = A[8 + r] * z, t3 = A[12 + r] * w;
    return ((t0 + t1) + t2) + t3;
}

// rule step 1, the model half: w[v] = M a_v for a = (-1,-1,0,1), (1,0,0,1), (-1,1,0,1).  The products by 0 and 1 are taken (an
// infinite entry times zero is a NaN, as in the restatements).
__device__ __forceinline__ void raster_world(const float4 *__restrict__ inst, uint32_t j, float (*w)[4])
{
    const float ax[3] = {-1.0f, 1.0f, -1.0f}, ay[3] = {-1.0f, 0.0f, 1.0f};
    float M[16];
    raster_load16(inst + (size_t)j * 4, M);
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
        for (int r = 0; r < 4; ++r) w[v][r] = raster_row(M, r, ax[v], ay[v], 0.0f, 1.0f);
}

// rule step 1 for body j, every row: P[v] = C (M a_v)
__device__ __forceinline__ void raster_vertices(const float *C, const float4 *__restrict__ inst, uint32_t j, float (*P)[4])
{
    float w[3][4];
    raster_world(inst, j, w);
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
        for (int r = 0; r < 4; ++r) P[v][r] = raster_row(C, r, w[v][0], w[v][1], w[v][2], w[v][3]);
}

// The same with the near plane's row first: a body wholly behind the camera stops there (false; the other rows of P are left as they
// were), which costs it the z rows only.
__device__ __forceinline__ bool raster_vertices_culled(const float *C, const float4 *__restrict__ inst, uint32_t j, float (*P)[4])
{
    float w[3][4];
    raster_world(inst, j, w);
#pragma unroll
    for (int v = 0; v < 3; ++v) P[v][2] = raster_row(C, 2, w[v][0], w[v][1], w[v][2], w[v][3]);
    if (P[0][2] < 0.0f && P[1][2] < 0.0f && P[2][2] < 0.0f) return false;
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r == 2) continue;
            P[v][r] = raster_row(C, r, w[v][0], w[v][1], w[v][2], w[v][3]);
        }
    return true;
}

// what the colour needs of a clipped edge (rule step 7): the clip parameters and the ends' w
struct Tex {
    float t_in, t_out, w0, w1;
};

// Rule step 2: the edge P0 -> P1 of clip-space vertices (x, y, z, w) clipped (Liang-Barsky) to z >= 0, w - z >= 0, w + y >= 0,
// w - y >= 0; no x planes.  Q0, Q1: the clipped ends.  false: dropped (both ends outside one boundary -- before any divide --, an
// empty parameter range, or an end with w <= 0).
__device__ __forceinline__ bool raster_clip(const float *P0, const float *P1, float *Q0, float *Q1, Tex &x)
{
    float t_in = 0.0f, t_out = 1.0f;
    const float b0v[4] = {P0[2], P0[3] - P0[2], P0[3] + P0[1], P0[3] - P0[1]};   // near, far, y = -w, y = +w
    const float b1v[4] = {P1[2], P1[3] - P1[2], P1[3] + P1[1], P1[3] - P1[1]};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float b0 = b0v[k], b1 = b1v[k];
        if (b0 < 0.0f && b1 < 0.0f) return false;
        if (b0 < 0.0f && b1 >= 0.0f) {
            const float r = b0 / (b0 - b1);
            if (r > t_in) t_in = r;        // max(t_in, r); a NaN r changes nothing
        } else if (b1 < 0.0f && b0 >= 0.0f) {
            const float r = b0 / (b0 - b1);
            if (r < t_out) t_out = r;      // min(t_out, r)
        }
    }
    if (t_in > t_out) return false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float D = P1[r] - P0[r];
        const float a = t_in * D, b = t_out * D;
        Q0[r] = (t_in > 0.0f) ? P0[r] + a : P0[r];
        Q1[r] = (t_out < 1.0f) ? P0[r] + b : P1[r];
    }
    if (!(Q0[3] > 0.0f && Q1[3] > 0.0f)) return false;
    x.t_in = t_in, x.t_out = t_out, x.w0 = Q0[3], x.w1 = Q1[3];
    return true;
}

// The depth at parameter t of an edge (steps 4 - 5, M2, F5, FM2): d = d0 + t dd; a candidate iff d < 1 (Less against the clear value;
// a NaN never passes), then !(d > 0) -> +0.  false: no candidate.
__device__ __forceinline__ bool raster_depth(float d0, float dd, float t, float &d)
{
    const float q = t * dd;
    d = d0 + q;
    if (!(d < 1.0f)) return false;
    if (!(d > 0.0f)) d = 0.0f;
    return true;
}

// Steps 7 - 10: the fragment of edge `edge` (0, 1, 2; clipped: x) at parameter t of the clipped edge -- the perspective-correct
// parameter, the texture coordinate, one texel, the vignette.
__device__ __forceinline__ float4 raster_fragment(const Tex &x, int edge, float t, const float4 *__restrict__ skin, uint32_t tw, uint32_t th)
{
    const float s0 = x.t_in > 0.0f ? x.t_in : 0.0f, s1 = x.t_out < 1.0f ? x.t_out : 1.0f;   // step 7
    const float i0 = 1.0f / x.w0, i1 = 1.0f / x.w1;
    const float a0 = s0 * i0, a1 = s1 * i1;
    const float da = a1 - a0, di = i1 - i0;
    const float pa = t * da, pi = t * di;
    const float num = a0 + pa, den = i0 + pi;
    float s = num / den;
    if (!(s > 0.0f)) s = 0.0f;                                   // (also a NaN: an extrapolated t may make den zero or negative)
    if (s > 1.0f) s = 1.0f;
    const float r1 = 1.0f - s;
    const float u = edge == 0 ? 0.0f : edge == 1 ? s : r1;       // step 8: the vertices carry (0,0), (0,1), (1,1)
    const float v = edge == 0 ? s : edge == 1 ? 1.0f : r1;
    float4 tex = make_float4(1.0f, 1.0f, 1.0f, 1.0f);            // no skin: 1 x 1 white
    if (skin) {                                                  // step 9: ClampToEdge, one nearest sample
        const float fu = u * (float)tw, fv = v * (float)th;
        const uint32_t fx = (uint32_t)floorf(fu), fy = (uint32_t)floorf(fv);   // 0 <= u, v <= 1: in range of the conversion
        const uint32_t ix = fx < tw - 1u ? fx : tw - 1u, iy = fy < th - 1u ? fy : th - 1u;
        tex = skin[(size_t)iy * tw + ix];
    }
    const float du = u - 0.5f, dv = v - 0.5f;                    // step 10
    const float uu = du * du, vv = dv * dv;
    const float m2 = uu + vv;
    const float f = 1.0f - m2;
    return make_float4(tex.x * f, tex.y * f, tex.z * f, 1.0f);
}

__device__ __forceinline__ float4 raster_clear() { return make_float4(0.1f, 0.2f, 0.3f, 1.0f); }

// M5, FM5: the mean of one channel's eight samples
__device__ __forceinline__ float raster_mean8(const float *a)
{
    return (((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) * 0.125f;
}

// M3, FM3: of the samples in `todo` (a sample k holds body id[k]), those of the lowest one's body j
__device__ __forceinline__ uint32_t raster_lowest_body(uint32_t todo, const uint32_t *id, uint32_t &j)
{
    j = 0;
#pragma unroll
    for (int k = 7; k >= 0; --k)
        if (todo >> k & 1u) j = id[k];
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        if ((todo >> k & 1u) && id[k] == j) mine |= 1u << k;
    return mine;
}

// a key bits(d) << 32 | j, or all ones where nothing was drawn
__device__ __forceinline__ uint64_t raster_key(float d, uint32_t j) { return ((uint64_t)__float_as_uint(d) << 32) | j; }
__device__ __forceinline__ uint32_t raster_key_id(uint64_t key) { return key == ~0ull ? 0xFFFFFFFFu : (uint32_t)key; }
__device__ __forceinline__ float raster_key_depth(uint64_t key) { return key == ~0ull ? 1.0f : __uint_as_float((uint32_t)(key >> 32)); }

// the sRGB byte of a linear value: the number of thresholds T[1..255] that are <= c (T strictly increasing; a NaN gives 0)
__device__ __forceinline__ uint32_t eye_srgb_byte(const float *T, float c)
{
    uint32_t b = 0;
#pragma unroll
    for (uint32_t step = 128; step; step >>= 1)
        if (T[b + step] <= c) b += step;     // b + step <= 255
    return b;
}

// step 11: the word whose bytes in memory are B, G, R, A; alpha byte 255
__device__ __forceinline__ uint32_t raster_bgra8(const float *T, float4 px)
{
    return eye_srgb_byte(T, px.z) | eye_srgb_byte(T, px.y) << 8 | eye_srgb_byte(T, px.x) << 16 | 0xFF000000u;
}

#define NB_SRGB_TABLE static __device__ const
#include "nb_srgb_tables.h"
#undef NB_SRGB_TABLE

// one lane's value to its whole wave
__device__ __forceinline__ float eye_bcast(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
__device__ __forceinline__ uint32_t eye_bcast(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }

// M1, FM1: the 8 samples' offsets in sixteenths, nibble k = 16 o_k: Vulkan's standard 8-sample pattern.  nb_eyes.h / nb_frame.h list
// the same sixteenths for the C ABI; nb_kernels.hip holds the static_assert that ties the two.
static constexpr uint32_t kMsaaSamples = 8;
static constexpr uint32_t kMsaaOffsets16 = 0xFB135D79u;         // x: (9, 7, 13, 5, 3, 1, 11, 15) / 16
static constexpr uint32_t kFrameMsaaOffsetsY16 = 0x1F7D39B5u;   // y: (5, 11, 9, 3, 13, 7, 15, 1) / 16

__device__ __forceinline__ float eye_msaa_offset(uint32_t k) { return (float)((kMsaaOffsets16 >> (4u * k)) & 15u) * 0.0625f; }   // exact
__device__ __forceinline__ float frame_msaa_offset_y(uint32_t k) { return (float)((kFrameMsaaOffsetsY16 >> (4u * k)) & 15u) * 0.0625f; }   // exact
