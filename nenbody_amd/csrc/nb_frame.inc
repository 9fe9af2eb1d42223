// nb_frame.inc -- the scene camera's frame (DESIGN.md section 11): what the reference's display pass leaves in its W x H target
// (src/main.rs:948-960: every instance's LineStrip triangle through the one scene camera, depth test Less against a clear of 1.0,
// the skin under the vignette, the clear colour (0.1, 0.2, 0.3, 1), a Bgra8UnormSrgb target), and which instance wrote each pixel.
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit after nb_eyes.inc.  The vertex products, the clip, the depth of
// a parameter, the fragment and the sRGB bytes are nb_raster.inc's, shared with the eye rows; this file adds the projection onto the
// plane, the major axis and its range, the step, the cover, the shade and the three kernels.  Launcher: nb_frame.h.
//
// The rule continues section 10's, one binary32 operation per step in the order written (-ffp-contract=off, IEEE '/');
// tests/frame_restatement.py states it again in numpy and the GPU tests compare every bit:
//   F1, F2       clip vertices and clipping as section 10 steps 1 and 2
//   F3           h = W/2, xs = (x / w) * h + h, d = z / w; g = H/2, ys = g - (y / w) * g (row 0 is the top)
//   F4           dx = xs1 - xs0, dy = ys1 - ys0; x-major iff |dx| >= |dy| (a NaN: y-major).  Along the major axis a, minor axis b:
//                every step m of the extent with min(a0, a1) <= mc < max(a0, a1), mc = m + 0.5; t = (mc - a0) / da, o = b0 + t * db;
//                the pixel is (m, floor(o)) iff 0 <= o < the minor extent
//   F5           d = d0 + t (d1 - d0); a candidate iff d < 1, then !(d > 0) -> +0; per pixel the minimum of bits(d) << 32 | j
//   F6           section 10 steps 6-11 with "covers column c" read as "has this pixel as one of its F4 pixels", and F4's t
//
// Shape: three kernels on the caller's stream over a caller-supplied plane of W x H 64-bit keys (a 1920 x 1080 plane is 16.6 MB: it
// does not fit in LDS as an eye's row does).  frame_clear_kernel sets the keys to all ones.  frame_edges_kernel takes one body per
// lane: the clip z row first (a body wholly behind the camera stops there), then the three edges; a lane walks the first
// kFrameOwnSteps major-axis steps of an edge itself and hands the rest to its whole wave, 64 steps at a time, as eyes_kernel does.
// Keys are resolved with a 64-bit atomic minimum at agent scope (one global_atomic_umin_x2; the eight XCDs' L2s do not see each
// other's plain stores within a kernel), so the result is the minimum of a set: the same bits from run to run.
// frame_resolve_kernel takes one pixel per lane, coalesced rows: ids and depth from the key, and for a non-empty key the winner's
// three edges again with frame_edge's own arithmetic, the edge of F6, the shade, the sRGB bytes (T in LDS).
// Of eye_cover's two culls one carries over: the atomic only goes out when the key is below the key read just before.  The other
// (a lower bound of the segment's depth against the key in place, before the divide) has nothing to test against here: which
// pixel a step writes is only known from the divide's t.

static constexpr int kFrameBlock = 256;
static constexpr uint32_t kFrameOwnSteps = 8;   // major-axis steps of an edge its own lane walks; the rest goes to the whole wave

struct FrameSeg {
    float a0, da;        // the major axis: the first end, a1 - a0
    float b0, db;        // the minor axis likewise
    float d0, dd;        // depth likewise
    float amin, amax;    // min / max of a0, a1
    float blim;          // the extent along the minor axis
    uint32_t lo, hi;     // a superset of the covered major-axis steps, [lo, hi)
    uint32_t xmajor;     // 1: a = x, b = y; 0: a = y, b = x
};

// One edge P0 -> P1 of clip-space vertices (x, y, z, w): clipped (F2), projected (F3), its major axis and range (F4).
// false: dropped, or covers no step.  tx: what the colour needs of the clipped edge beyond FrameSeg.
__device__ __forceinline__ bool frame_edge(const float *P0, const float *P1, float h, float g, uint32_t width, uint32_t height, FrameSeg &s,
                                           Tex *tx = nullptr)
{
    float Q0[4], Q1[4];
    Tex x;
    if (!raster_clip(P0, P1, Q0, Q1, x)) return false;
    if (tx) *tx = x;
    const float u0 = Q0[0] / Q0[3], u1 = Q1[0] / Q1[3];
    const float v0 = Q0[1] / Q0[3], v1 = Q1[1] / Q1[3];
    const float p0 = u0 * h, p1 = u1 * h, q0 = v0 * g, q1 = v1 * g;
    const float xs0 = p0 + h, xs1 = p1 + h;
    const float ys0 = g - q0, ys1 = g - q1;                                     // NDC y points up, row 0 is the top
    const float dx = xs1 - xs0, dy = ys1 - ys0;
    const bool xm = fabsf(dx) >= fabsf(dy);                                     // a NaN on either side: y-major
    const float a1 = xm ? xs1 : ys1;
    s.xmajor = xm ? 1u : 0u;
    s.a0 = xm ? xs0 : ys0;
    s.da = xm ? dx : dy;
    s.b0 = xm ? ys0 : xs0;
    s.db = xm ? dy : dx;
    s.blim = (float)(xm ? height : width);
    const float alim = (float)(xm ? width : height);
    s.amin = (s.a0 <= a1) ? s.a0 : a1;
    s.amax = (s.a0 <= a1) ? a1 : s.a0;
    if (!(s.amin <= s.amax)) return false;                                      // a NaN end covers nothing
    // m covered => amin <= m + 0.5 < amax => floor(amin) - 1 < m < ceil(amax): a superset, clamped in float first (the ends may be
    // infinite)
    const float lo = floorf(fmaxf(s.amin, -4.0f)) - 1.0f;
    const float hi = ceilf(fminf(s.amax, alim + 4.0f)) + 1.0f;
    s.lo = (uint32_t)fminf(fmaxf(lo, 0.0f), alim);
    s.hi = (uint32_t)fminf(fmaxf(hi, 0.0f), alim);
    if (s.lo >= s.hi) return false;
    s.d0 = Q0[2] / Q0[3];
    const float d1 = Q1[2] / Q1[3];
    s.dd = d1 - s.d0;
    return true;
}

// Step m of segment s (F4, F5): its parameter, its pixel (an index into the H x W plane), its depth.  false: no pixel, or no candidate.
__device__ __forceinline__ bool frame_step(const FrameSeg &s, uint32_t m, uint32_t width, float &t, uint32_t &pixel, float &d)
{
    const float mc = (float)m + 0.5f;                                           // exact
    if (!(s.amin <= mc && mc < s.amax)) return false;
    t = (mc - s.a0) / s.da;
    const float qb = t * s.db;
    const float o = s.b0 + qb;
    if (!(o >= 0.0f && o < s.blim)) return false;                               // a NaN covers nothing
    if (!raster_depth(s.d0, s.dd, t, d)) return false;
    const uint32_t f = (uint32_t)o;                                             // floor(o): 0 <= o < blim <= 4096
    pixel = s.xmajor ? f * width + m : m * width + f;                           // m < hi <= the major extent: inside the plane
    return true;
}

// Keys only ever decrease while the edges kernel runs, so a stale value read here is never below the key in place: it can only fail
// to cull, never cull a key that would have won.
__device__ __forceinline__ uint64_t frame_key_load(uint64_t *k) { return __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ void frame_cover(uint64_t *keys, uint32_t m, const FrameSeg &s, uint32_t j, uint32_t width)
{
    float t, d;
    uint32_t pixel;
    if (!frame_step(s, m, width, t, pixel, d)) return;
    const uint64_t key = raster_key(d, j);
    if (key < frame_key_load(keys + pixel)) __hip_atomic_fetch_min(keys + pixel, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// segment s of lane src for its whole wave, its range starting at that lane's `rest`
__device__ __forceinline__ FrameSeg frame_seg_bcast(const FrameSeg &s, uint32_t rest, int src)
{
    FrameSeg b;
    b.a0 = eye_bcast(s.a0, src), b.da = eye_bcast(s.da, src), b.b0 = eye_bcast(s.b0, src), b.db = eye_bcast(s.db, src);
    b.d0 = eye_bcast(s.d0, src), b.dd = eye_bcast(s.dd, src), b.amin = eye_bcast(s.amin, src), b.amax = eye_bcast(s.amax, src);
    b.blim = eye_bcast(s.blim, src), b.lo = eye_bcast(rest, src), b.hi = eye_bcast(s.hi, src), b.xmajor = eye_bcast(s.xmajor, src);
    return b;
}

// The colour of pixel (col, row), its key resolved (F6): the winner's three edges again with frame_edge's own arithmetic, the first
// that has this pixel among its F4 pixels, is a candidate and gives the key's depth bits, then section 10 steps 7-10.
__device__ __forceinline__ float4 frame_shade(uint64_t key, uint32_t col, uint32_t row, const float *C, const float4 *__restrict__ inst,
                                              uint32_t width, uint32_t height, const float4 *__restrict__ skin, uint32_t tw, uint32_t th)
{
    if (key == ~0ull) return raster_clear();
    const uint32_t j = (uint32_t)key, dbits = (uint32_t)(key >> 32);
    const float h = (float)width * 0.5f, g = (float)height * 0.5f;
    float P[3][4];
    raster_vertices(C, inst, j, P);
    const uint32_t here = row * width + col;
    int edge = -1;
    float t_at = 0.0f;
    Tex at{};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        FrameSeg e{};
        Tex x{};
        if (edge >= 0 || !frame_edge(P[k], P[k == 2 ? 0 : k + 1], h, g, width, height, e, &x)) continue;
        float t, d;
        uint32_t pixel;
        if (!frame_step(e, e.xmajor ? col : row, width, t, pixel, d)) continue;
        if (pixel != here || __float_as_uint(d) != dbits) continue;
        edge = k, t_at = t, at = x;
    }
    if (edge < 0) return raster_clear();   // (the key came from one of the three: not reached)
    return raster_fragment(at, edge, t_at, skin, tw, th);
}

#ifdef __HIPCC__
__global__ __launch_bounds__(kFrameBlock) void frame_clear_kernel(uint64_t *__restrict__ keys, uint32_t pixels)
{
    const uint32_t p = blockIdx.x * (uint32_t)kFrameBlock + threadIdx.x;
    if (p < pixels) keys[p] = ~0ull;
}

__global__ __launch_bounds__(kFrameBlock) void frame_edges_kernel(uint32_t n_total, const float4 *__restrict__ cam,
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
        const bool has = live && frame_edge(P[k], P[k == 2 ? 0 : k + 1], h, g, width, height, s);
        uint32_t rest = 0;   // first step left to the wave
        if (has) {
            const uint32_t own = s.hi - s.lo < kFrameOwnSteps ? s.hi : s.lo + kFrameOwnSteps;
            for (uint32_t m = s.lo; m < own; ++m) frame_cover(keys, m, s, j, width);
            rest = own;
        }
        uint64_t wide = __ballot(has && rest < s.hi);
        while (wide) {
            const int src = __ffsll((unsigned long long)wide) - 1;
            wide &= wide - 1;
            const FrameSeg b = frame_seg_bcast(s, rest, src);
            const uint32_t bj = eye_bcast(j, src);
            for (uint32_t m = b.lo + lane; m < b.hi; m += 64u) frame_cover(keys, m, b, bj, width);
        }
    }
}

__global__ __launch_bounds__(kFrameBlock) void frame_resolve_kernel(const float4 *__restrict__ cam, const float4 *__restrict__ inst,
                                                                    uint32_t width, uint32_t height, const uint64_t *__restrict__ keys,
                                                                    const float4 *__restrict__ skin, uint32_t tw, uint32_t th,
                                                                    uint32_t *__restrict__ ids, float *__restrict__ depth,
                                                                    float4 *__restrict__ rgba, uint32_t *__restrict__ bgra8)
{
    static_assert(kFrameBlock == 256, "one lane copies one entry of T");
    __shared__ float enc[256];
    enc[threadIdx.x] = kSrgbEncodeT[threadIdx.x];
    __syncthreads();
    const uint32_t pixels = width * height;   // <= 2^24
    const uint32_t p = blockIdx.x * (uint32_t)kFrameBlock + threadIdx.x;
    if (p >= pixels) return;
    const uint64_t key = keys[p];
    if (ids) ids[p] = raster_key_id(key);
    if (depth) depth[p] = raster_key_depth(key);
    if (!rgba && !bgra8) return;
    float C[16];
    raster_load16(cam, C);
    const uint32_t row = p / width, col = p - row * width;
    const float4 px = frame_shade(key, col, row, C, inst, width, height, skin, tw, th);
    if (rgba) rgba[p] = px;
    if (bgra8) bgra8[p] = raster_bgra8(enc, px);
}

hipError_t launch_frame(uint32_t n_total, const float *cam, const float *inst, uint32_t width, uint32_t height, const float *skin,
                        uint32_t tw, uint32_t th, uint64_t *keys, uint32_t *ids, float *depth, float *rgba, uint32_t *bgra8, hipStream_t s)
{
    const uint32_t pixels = width * height;
    const uint32_t grid = ceil_div_u(pixels, kFrameBlock);
    hipLaunchKernelGGL(frame_clear_kernel, dim3(grid), dim3(kFrameBlock), 0, s, keys, pixels);
    if (n_total)
        hipLaunchKernelGGL(frame_edges_kernel, dim3(ceil_div_u(n_total, kFrameBlock)), dim3(kFrameBlock), 0, s, n_total,
                           (const float4 *)cam, (const float4 *)inst, width, height, keys);
    hipLaunchKernelGGL(frame_resolve_kernel, dim3(grid), dim3(kFrameBlock), 0, s, (const float4 *)cam, (const float4 *)inst, width, height,
                       (const uint64_t *)keys, (const float4 *)skin, tw, th, ids, depth, (float4 *)rgba, bgra8);
    return hipGetLastError();
}
#endif   // __HIPCC__
