// nb_frame_msaa.inc -- the scene camera's frame through 8 samples per pixel, resolved (DESIGN.md section 11.1, steps FM1-FM5): what
// the reference's display pass leaves in its target with msaa_samples = 8 (src/main.rs:652; the display target, :685-690; its pass
// resolving into the swapchain image, :545-548, :948-960).
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit after nb_eyes_msaa.inc.  The edge and the clear pass are
// nb_frame.inc's (frame_edge, FrameSeg, frame_key_load, frame_seg_bcast, frame_clear_kernel); the vertex products, the depth of a
// parameter, the fragment, the mean, the sample offsets and the sRGB bytes are nb_raster.inc's; this file adds the step and the cover
// of a sample, the 8-sample shade and the two kernels.  Launcher: nb_frame.h.
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
    if (!raster_depth(s.d0, s.dd, t, d)) return false;
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
    const uint64_t key = raster_key(d, j);
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
    while (todo) {
        uint32_t j;                                              // the body of the lowest sample left, and its samples
        uint32_t mine = raster_lowest_body(todo, id, j);
        todo &= ~mine;
        float P[3][4];
        raster_vertices(C, inst, j, P);
#pragma unroll
        for (int e = 0; e < 3; ++e) {                            // FM3: the first edge in draw order
            FrameSeg s{};
            Tex x{};
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
            const float mc = (float)m + 0.5f;                    // FM4: once per (pixel, body, edge), at the centre of step m
            const float4 px = raster_fragment(x, e, (mc - s.a0) / s.da, skin, tw, th);
#pragma unroll
            for (uint32_t k = 0; k < kMsaaSamples; ++k)
                if (hit >> k & 1u) ar[k] = px.x, ag[k] = px.y, ab[k] = px.z, aa[k] = px.w;
        }
        // (a sample left in `mine` keeps the clear colour: its key came from one of the three edges, so this is not reached)
    }
    return make_float4(raster_mean8(ar), raster_mean8(ag), raster_mean8(ab), raster_mean8(aa));   // FM5
}

#ifdef __HIPCC__
__global__ __launch_bounds__(kFrameBlock) void frame_msaa_edges_kernel(uint32_t n_total, const float4 *__restrict__ cam,
                                                                       const float4 *__restrict__ inst, uint32_t width, uint32_t height,
                                                                       uint64_t *__restrict__ keys)
{
    const uint32_t lane = threadIdx.x & 63u;
    const float h = (float)width * 0.5f, g = (float)height * 0.5f;   // exact
    float C[16];
    raster_load16(cam, C);
    const uint32_t j = blockIdx.x * (uint32_t)kFrameBlock + threadIdx.x;
    float P[3][4] = {};
    bool live = j < n_total;   // (no lane leaves early: every lane of a wave runs the wave loops below)
    if (live) live = raster_vertices_culled(C, inst, j, P);   // a body wholly behind the camera stops at its z rows
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
            const FrameSeg b = frame_seg_bcast(s, rest, src);
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
                if (ids8) ids8[i] = raster_key_id(key);
                if (depth8) depth8[i] = raster_key_depth(key);
            }
        }
    }
    const uint32_t p = blockIdx.x * (uint32_t)kFrameBlock + threadIdx.x;
    if (p >= pixels || (!rgba && !bgra8)) return;
    uint64_t k8[kMsaaSamples];                          // the pixel's 64 contiguous bytes
#pragma unroll
    for (uint32_t k = 0; k < kMsaaSamples; ++k) k8[k] = keys[(size_t)p * kMsaaSamples + k];
    float C[16];
    raster_load16(cam, C);
    const uint32_t row = p / width, col = p - row * width;
    const float4 px = frame_msaa_shade(k8, col, row, C, inst, width, height, skin, tw, th);
    if (rgba) rgba[p] = px;
    if (bgra8) bgra8[p] = raster_bgra8(enc, px);
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
#endif   // __HIPCC__
