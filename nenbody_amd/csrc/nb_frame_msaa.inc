// nb_frame_msaa.inc -- the scene camera's frame through 8 samples per pixel, resolved (DESIGN.md section 11.1, steps FM1-FM5): what
// the reference's display pass leaves in its target with msaa_samples = 8 (src/main.rs:652; the display target, :685-690; its pass
// resolving into the swapchain image, :545-548, :948-960).
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit after nb_eyes_msaa.inc.  nb_eyes.inc, nb_frame.inc and
// nb_eyes_msaa.inc are used as they are (frame_edge, FrameSeg, FrameTex, frame_key_load, frame_clear_kernel; eye_bcast, eye_srgb_byte,
// kSrgbEncodeT; eye_msaa_offset, eye_msaa_fragment) and not edited.  Launcher: nb_frame.h.
//
// The rule continues section 11's F1-F6, one binary32 operation per step in the order written (-ffp-contract=off, IEEE '/');
// tests/frame_msaa_restatement.py states it again in numpy and the GPU tests compare every bit:
//   FM1  samples     sample k of pixel (c, r) at (c + ox_k, r + oy_k), ox = (9, 7, 13, 5, 3, 1, 11, 15) / 16 (the eye rows' offsets),
//                    oy = (5, 11, 9, 3, 13, 7, 15, 1) / 16: Vulkan's standard 8-sample pattern (sums exact for c, r < 4096)
//   FM2  per sample  F1-F4's clip, projection and major axis; with (oa, ob) = (ox, oy) on an x-major edge and (oy, ox) on a y-major
//                    one, for every step m and every k: a_k = m + oa_k, tried iff min(a0, a1) <= a_k < max(a0, a1);
//                    t_k = (a_k - a0) / da, o_k = b0 + t_k db, e_k = o_k + q_k with q_k = 0.5 - ob_k (exact); sample k of the pixel
//                    (m, floor(e_k)) iff 0 <= e_k < the minor extent; d_k = d0 + t_k (d1 - d0), a candidate iff d_k < 1, then
//                    !(d_k > 0) -> +0; the minimum of bits(d_k) << 32 | j
//   FM3  edge        per sample the first of the winner's edges 0, 1, 2 that produces this sample, is a candidate and gives the key's bits
//   FM4  fragment    one per (pixel, body, edge), shaded at the pixel centre whether or not the centre is covered: section 10 steps
//                    7-10 with t = (mc - a0) / da, mc = m + 0.5, m the pixel's index along that edge's major axis
//   FM5  resolve     a_k = the fragment colour of sample k's (body, edge), or the clear colour; per channel, alpha included,
//                    (((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7))) * 0.125; bgra8 through T, alpha byte 255
//
// Shape: the frame's three kernels over a plane of W x H x 8 keys, sample-minor (key (pixel p, k) at 8 p + k; 133 MB at 1920 x 1080:
// device memory, where an eye's 8 W keys fit in LDS).  frame_clear_kernel sets the 8 W H keys.  frame_msaa_edges_kernel takes one body
// per lane as frame_edges_kernel does; a lane walks the first kFrameMsaaOwnSteps major-axis steps x 8 samples of an edge itself and
// hands the rest to its whole wave, 8 steps x 8 samples at a time (lane 8 i + k: step lo + i, sample k).  Keys resolve with one relaxed
// agent-scope 64-bit atomic minimum behind frame_cover's read-before-write cull.  frame_msaa_resolve_kernel takes one pixel per lane:
// ids8 / depth8 go out as the keys lie, a workgroup's 2048 keys in coalesced rows; then each distinct body among the pixel's samples
// has its edges rebuilt once through frame_edge, each distinct (body, edge) is shaded once at the pixel centre.

static constexpr uint32_t kFrameMsaaOwnSteps = 2;            // major-axis steps of an edge its own lane walks (x 8 samples each)
static constexpr uint32_t kFrameMsaaOffsetsY16 = 0x1F7D39B5u;   // nibble k = 16 oy_k (ox: kMsaaOffsets16)

__device__ __forceinline__ float frame_msaa_offset_y(uint32_t k) { return (float)((kFrameMsaaOffsetsY16 >> (4u * k)) & 15u) * 0.0625f; }   // exact

// Sample k of step m of segment s (FM2): its parameter, the pixel it belongs to (an index into the H x W plane), its depth.
// false: no pixel, or no candidate.
__device__ __forceinline__ bool frame_msaa_step(const FrameSeg &s, uint32_t m, uint32_t k, uint32_t width, float &t, uint32_t &pixel, float &d)
{
    const float ox = eye_msaa_offset(k), oy = frame_msaa_offset_y(k);
    const float oa = s.xmajor ? ox : oy, ob = s.xmajor ? oy : ox;
    const float a = (float)m + oa;                                              // exact
    if (!(s.amin <= a && a < s.amax)) return false;
    t = (a - s.a0) / s.da;
    const float qb = t * s.db;
    const float o = s.b0 + qb;
    const float q = 0.5f - ob;                                                  // exact
    const float e = o + q;
    if (!(e >= 0.0f && e < s.blim)) return false;                               // a NaN covers nothing
    const float qd = t * s.dd;
    d = s.d0 + qd;
    if (!(d < 1.0f)) return false;                                              // Less against the clear value; NaN never passes
    if (!(d > 0.0f)) d = 0.0f;
    const uint32_t f = (uint32_t)e;                                             // floor(e): 0 <= e < blim <= 2048
    pixel = s.xmajor ? f * width + m : m * width + f;                           // m < hi <= the major extent: inside the plane
    return true;
}

// keys: the plane, sample-minor.  As frame_cover: a stale key read here is never below the key in place, so it never culls a winner.
__device__ __forceinline__ void frame_msaa_cover(uint64_t *keys, uint32_t m, uint32_t k, const FrameSeg &s, uint32_t j, uint32_t width)
{
    float t, d;
    uint32_t pixel;
    if (!frame_msaa_step(s, m, k, width, t, pixel, d)) return;
    uint64_t *slot = keys + ((size_t)pixel * kMsaaSamples + k);
    const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | j;
    if (key < frame_key_load(slot)) __hip_atomic_fetch_min(slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// FM3-FM5 for pixel (col, row), its eight keys resolved (every array index below is a constant after unrolling: no scratch)
__device__ __forceinline__ float4 frame_msaa_shade(const uint64_t *keys8, uint32_t col, uint32_t row, const float *C,
                                                   const float4 *__restrict__ inst, uint32_t width, uint32_t height,
                                                   const float4 *__restrict__ skin, uint32_t tw, uint32_t th)
{
    uint32_t id[kMsaaSamples], db[kMsaaSamples];
    float ar[kMsaaSamples], ag[kMsaaSamples], ab[kMsaaSamples], aa[kMsaaSamples];
    uint32_t todo = 0;                                           // samples that hold a body and have no fragment yet
#pragma unroll
    for (uint32_t k = 0; k < kMsaaSamples; ++k) {
        const uint64_t key = keys8[k];
        id[k] = (uint32_t)key, db[k] = (uint32_t)(key >> 32);
        if (key != ~0ull) todo |= 1u << k;
        ar[k] = 0.1f, ag[k] = 0.2f, ab[k] = 0.3f, aa[k] = 1.0f;  // the clear colour
    }
    const float h = (float)width * 0.5f, g = (float)height * 0.5f;
    const uint32_t here = row * width + col;
    const float ax[3] = {-1.0f, 1.0f, -1.0f}, ay[3] = {-1.0f, 0.0f, 1.0f};
    while (todo) {
        uint32_t j = 0;                                          // the body of the lowest sample left
#pragma unroll
        for (int k = kMsaaSamples - 1; k >= 0; --k)
            if (todo >> k & 1u) j = id[k];
        uint32_t mine = 0;                                       // its samples
#pragma unroll
        for (uint32_t k = 0; k < kMsaaSamples; ++k)
            if ((todo >> k & 1u) && id[k] == j) mine |= 1u << k;
        todo &= ~mine;
        float M[16], P[3][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 v = inst[(size_t)j * 4 + k];
            M[4 * k] = v.x, M[4 * k + 1] = v.y, M[4 * k + 2] = v.z, M[4 * k + 3] = v.w;
        }
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            float w[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float t0 = M[r] * ax[v], t1 = M[4 + r] * ay[v], t2 = M[8 + r] * 0.0f, t3 = M[12 + r] * 1.0f;
                w[r] = ((t0 + t1) + t2) + t3;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float t0 = C[r] * w[0], t1 = C[4 + r] * w[1], t2 = C[8 + r] * w[2], t3 = C[12 + r] * w[3];
                P[v][r] = ((t0 + t1) + t2) + t3;
            }
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) {                            // FM3: the first edge in draw order
            FrameSeg s{};
            FrameTex x{};
            if (!mine || !frame_edge(P[e], P[e == 2 ? 0 : e + 1], h, g, width, height, s, &x)) continue;
            const uint32_t m = s.xmajor ? col : row;
            uint32_t hit = 0;
#pragma unroll
            for (uint32_t k = 0; k < kMsaaSamples; ++k) {
                if (!(mine >> k & 1u)) continue;
                float t, d;
                uint32_t pixel;
                if (!frame_msaa_step(s, m, k, width, t, pixel, d)) continue;
                if (pixel == here && __float_as_uint(d) == db[k]) hit |= 1u << k;
            }
            if (!hit) continue;
            mine &= ~hit;
            EyeSeg cs{};                                         // FM4: once per (pixel, body, edge), at the centre of step m
            EyeTex cx{};
            cs.xs0 = s.a0, cs.dx = s.da;
            cx.t_in = x.t_in, cx.t_out = x.t_out, cx.w0 = x.w0, cx.w1 = x.w1;
            const float4 px = eye_msaa_fragment(cs, cx, e, (float)m + 0.5f, skin, tw, th);
#pragma unroll
            for (uint32_t k = 0; k < kMsaaSamples; ++k)
                if (hit >> k & 1u) ar[k] = px.x, ag[k] = px.y, ab[k] = px.z, aa[k] = px.w;
        }
        // (a sample left in `mine` keeps the clear colour: its key came from one of the three edges, so this is not reached)
    }
    float4 o;                                                    // FM5
    o.x = (((ar[0] + ar[1]) + (ar[2] + ar[3])) + ((ar[4] + ar[5]) + (ar[6] + ar[7]))) * 0.125f;
    o.y = (((ag[0] + ag[1]) + (ag[2] + ag[3])) + ((ag[4] + ag[5]) + (ag[6] + ag[7]))) * 0.125f;
    o.z = (((ab[0] + ab[1]) + (ab[2] + ab[3])) + ((ab[4] + ab[5]) + (ab[6] + ab[7]))) * 0.125f;
    o.w = (((aa[0] + aa[1]) + (aa[2] + aa[3])) + ((aa[4] + aa[5]) + (aa[6] + aa[7]))) * 0.125f;
    return o;
}

__global__ __launch_bounds__(kFrameBlock) void frame_msaa_edges_kernel(uint32_t n_total, const float4 *__restrict__ cam,
                                                                       const float4 *__restrict__ inst, uint32_t width, uint32_t height,
                                                                       uint64_t *__restrict__ keys)
{
    const uint32_t lane = threadIdx.x & 63u;
    const float h = (float)width * 0.5f, g = (float)height * 0.5f;   // exact
    const float ax[3] = {-1.0f, 1.0f, -1.0f}, ay[3] = {-1.0f, 0.0f, 1.0f};
    float C[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 v = cam[k];
        C[4 * k] = v.x, C[4 * k + 1] = v.y, C[4 * k + 2] = v.z, C[4 * k + 3] = v.w;
    }
    const uint32_t j = blockIdx.x * (uint32_t)kFrameBlock + threadIdx.x;
    float P[3][4] = {};
    bool live = j < n_total;   // (no lane leaves early: every lane of a wave runs the wave loops below)
    if (live) {
        float M[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 v = inst[(size_t)j * 4 + k];
            M[4 * k] = v.x, M[4 * k + 1] = v.y, M[4 * k + 2] = v.z, M[4 * k + 3] = v.w;
        }
        float w[3][4];
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float t0 = M[r] * ax[v], t1 = M[4 + r] * ay[v], t2 = M[8 + r] * 0.0f, t3 = M[12 + r] * 1.0f;
                w[v][r] = ((t0 + t1) + t2) + t3;
            }
#pragma unroll
        for (int v = 0; v < 3; ++v) {   // the near plane's row first: a body wholly behind the camera stops here
            const float t0 = C[2] * w[v][0], t1 = C[6] * w[v][1], t2 = C[10] * w[v][2], t3 = C[14] * w[v][3];
            P[v][2] = ((t0 + t1) + t2) + t3;
        }
        live = !(P[0][2] < 0.0f && P[1][2] < 0.0f && P[2][2] < 0.0f);
        if (live) {
#pragma unroll
            for (int v = 0; v < 3; ++v)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (r == 2) continue;
                    const float t0 = C[r] * w[v][0], t1 = C[4 + r] * w[v][1], t2 = C[8 + r] * w[v][2], t3 = C[12 + r] * w[v][3];
                    P[v][r] = ((t0 + t1) + t2) + t3;
                }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        FrameSeg s{};
        const bool has = live && frame_edge(P[k], P[k == 2 ? 0 : k + 1], h, g, width, height, s);   // [s.lo, s.hi) holds every sample's step too
        uint32_t rest = 0;   // first step left to the wave
        if (has) {
            const uint32_t own = s.hi - s.lo < kFrameMsaaOwnSteps ? s.hi : s.lo + kFrameMsaaOwnSteps;
            for (uint32_t m = s.lo; m < own; ++m)
#pragma unroll
                for (uint32_t q = 0; q < kMsaaSamples; ++q) frame_msaa_cover(keys, m, q, s, j, width);
            rest = own;
        }
        uint64_t wide = __ballot(has && rest < s.hi);
        while (wide) {
            const int src = __ffsll((unsigned long long)wide) - 1;
            wide &= wide - 1;
            FrameSeg b;
            b.a0 = eye_bcast(s.a0, src), b.da = eye_bcast(s.da, src), b.b0 = eye_bcast(s.b0, src), b.db = eye_bcast(s.db, src);
            b.d0 = eye_bcast(s.d0, src), b.dd = eye_bcast(s.dd, src), b.amin = eye_bcast(s.amin, src), b.amax = eye_bcast(s.amax, src);
            b.blim = eye_bcast(s.blim, src), b.lo = eye_bcast(rest, src), b.hi = eye_bcast(s.hi, src), b.xmajor = eye_bcast(s.xmajor, src);
            const uint32_t bj = eye_bcast(j, src);
            for (uint32_t m = b.lo + (lane >> 3); m < b.hi; m += 8u) frame_msaa_cover(keys, m, lane & 7u, b, bj, width);   // m < the major extent
        }
    }
}

__global__ __launch_bounds__(kFrameBlock) void frame_msaa_resolve_kernel(const float4 *__restrict__ cam, const float4 *__restrict__ inst,
                                                                         uint32_t width, uint32_t height, const uint64_t *__restrict__ keys,
                                                                         const float4 *__restrict__ skin, uint32_t tw, uint32_t th,
                                                                         uint32_t *__restrict__ ids8, float *__restrict__ depth8,
                                                                         float4 *__restrict__ rgba, uint32_t *__restrict__ bgra8)
{
    static_assert(kFrameBlock == 256, "one lane copies one entry of T");
    __shared__ float enc[256];
    enc[threadIdx.x] = kSrgbEncodeT[threadIdx.x];
    __syncthreads();
    const uint32_t pixels = width * height;            // <= 2^22
    const uint32_t cells = pixels * kMsaaSamples;      // <= 2^25
    if (ids8 || depth8) {                              // the keys as they lie, (r * width + c) * 8 + k: this workgroup's 2048, coalesced
        const uint32_t base = blockIdx.x * (uint32_t)kFrameBlock * kMsaaSamples;
#pragma unroll
        for (uint32_t q = 0; q < kMsaaSamples; ++q) {
            const uint32_t i = base + q * (uint32_t)kFrameBlock + threadIdx.x;
            if (i < cells) {
                const uint64_t key = keys[i];
                const bool none = key == ~0ull;
                if (ids8) ids8[i] = none ? 0xFFFFFFFFu : (uint32_t)key;
                if (depth8) depth8[i] = none ? 1.0f : __uint_as_float((uint32_t)(key >> 32));
            }
        }
    }
    const uint32_t p = blockIdx.x * (uint32_t)kFrameBlock + threadIdx.x;
    if (p >= pixels || (!rgba && !bgra8)) return;
    uint64_t k8[kMsaaSamples];                          // the pixel's 64 contiguous bytes
#pragma unroll
    for (uint32_t k = 0; k < kMsaaSamples; ++k) k8[k] = keys[(size_t)p * kMsaaSamples + k];
    float C[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 v = cam[k];
        C[4 * k] = v.x, C[4 * k + 1] = v.y, C[4 * k + 2] = v.z, C[4 * k + 3] = v.w;
    }
    const uint32_t row = p / width, col = p - row * width;
    const float4 px = frame_msaa_shade(k8, col, row, C, inst, width, height, skin, tw, th);
    if (rgba) rgba[p] = px;
    if (bgra8)   // bytes in memory B, G, R, A
        bgra8[p] = eye_srgb_byte(enc, px.z) | eye_srgb_byte(enc, px.y) << 8 | eye_srgb_byte(enc, px.x) << 16 | 0xFF000000u;
}

hipError_t launch_frame_msaa(uint32_t n_total, const float *cam, const float *inst, uint32_t width, uint32_t height, const float *skin,
                             uint32_t tw, uint32_t th, uint64_t *keys, uint32_t *ids8, float *depth8, float *rgba, uint32_t *bgra8,
                             hipStream_t s)
{
    const uint32_t pixels = width * height, cells = pixels * kMsaaSamples;
    hipLaunchKernelGGL(frame_clear_kernel, dim3(ceil_div_u(cells, kFrameBlock)), dim3(kFrameBlock), 0, s, keys, cells);
    if (n_total)
        hipLaunchKernelGGL(frame_msaa_edges_kernel, dim3(ceil_div_u(n_total, kFrameBlock)), dim3(kFrameBlock), 0, s, n_total,
                           (const float4 *)cam, (const float4 *)inst, width, height, keys);
    hipLaunchKernelGGL(frame_msaa_resolve_kernel, dim3(ceil_div_u(pixels, kFrameBlock)), dim3(kFrameBlock), 0, s, (const float4 *)cam,
                       (const float4 *)inst, width, height, (const uint64_t *)keys, (const float4 *)skin, tw, th, ids8, depth8,
                       (float4 *)rgba, bgra8);
    return hipGetLastError();
}
