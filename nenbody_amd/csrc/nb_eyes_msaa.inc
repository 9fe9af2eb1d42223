// nb_eyes_msaa.inc -- every entity's eye view through 8 samples per column, resolved (DESIGN.md section 10, steps M1-M5): what the
// reference's eye targets hold with msaa_samples = 8 (src/main.rs:652; sample_count, :263; resolve_target, :547, :611).
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit after nb_frame.inc.  The edge is nb_eyes.inc's (eye_edge,
// EyeSeg, eye_key_load) and so is the loop over the bodies (eye_row_fill, with this file's EyeCover8); the vertex products, the depth
// of a parameter, the fragment, the mean, the sample offsets and the sRGB bytes are nb_raster.inc's; this file adds the cover of a
// sample, the 8-sample shade and the kernel.  Launcher: nb_eyes.h.
//
// The rule continues section 10's steps 1-11, one binary32 operation per step in the order written (-ffp-contract=off, IEEE '/');
// tests/eyes_msaa_restatement.py states it again in numpy and the GPU tests compare every bit:
//   M1  samples     sample k of column c at x_k = c + o_k, o = (9, 7, 13, 5, 3, 1, 11, 15) / 16 (exact for c < 4096)
//   M2  per sample  steps 3-5 with xc replaced by x_k: covered iff min(xs) <= x_k < max(xs); t_k = (x_k - xs0) / (xs1 - xs0),
//                   d_k = d0 + t_k (d1 - d0); a candidate iff d_k < 1, then !(d_k > 0) -> +0; the minimum of bits(d_k) << 32 | j
//   M3  edge        per sample the first of the winner's edges 0, 1, 2 that covers the sample, is a candidate and gives the key's bits
//   M4  fragment    one per (column, body, edge), shaded at the column centre whether or not the centre is covered: steps 7-10 with
//                   t = (xc - xs0) / (xs1 - xs0), xc = c + 0.5
//   M5  resolve     a_k = the fragment colour of sample k's (body, edge), or the clear colour; per channel, alpha included,
//                   (((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7))) * 0.125; bgra8 through T, alpha byte 255
//
// Shape: eyes_kernel's -- one workgroup of 256 lanes per eye, a grid-stride loop over the eyes -- with the eye's 8 W keys in LDS,
// sample-minor (key (c, k) at 8 c + k), T behind them: 64 W + 1024 bytes.  A lane takes one body per pass, clips its three edges,
// walks the first kMsaaOwnCols columns of each span itself and hands the rest to its whole wave, 8 columns x 8 samples at a time:
// 64 consecutive keys.  eye_cover's culls carry over (eye_edge's klow bounds every d_k as it bounds every d: x_k lies between the
// ends wherever the sample is covered).  Then ids8 / depth8 go out as the keys lie, and a lane per column shades: each distinct body
// among the column's samples has its edges rebuilt once, each distinct (body, edge) is shaded once.

static constexpr uint32_t kMsaaOwnCols = 4;               // columns of a span its own lane walks; the rest goes to the whole wave

// sample k of column c of segment s of body j; keys: the eye's, sample-minor
__device__ __forceinline__ void eye_msaa_cover(uint64_t *keys, uint32_t c, uint32_t k, const EyeSeg &s, uint32_t j)
{
    const float x = (float)c + eye_msaa_offset(k);                              // exact
    if (!(s.xa <= x && x < s.xb)) return;
    uint64_t *slot = keys + (c * kMsaaSamples + k);
    if ((((uint64_t)s.klow << 32) | j) >= eye_key_load(slot)) return;           // nothing this segment writes here can win
    const float t = (x - s.xs0) / s.dx;
    float d;
    if (!raster_depth(s.d0, s.dd, t, d)) return;
    const uint64_t key = raster_key(d, j);
    if (key < eye_key_load(slot)) __hip_atomic_fetch_min(slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// M3-M5 for column c of one eye, its eight keys resolved (every array index below is a constant after unrolling: no scratch)
__device__ __forceinline__ float4 eye_msaa_shade(const uint64_t *keys, uint32_t c, const float *C, const float4 *__restrict__ inst, float h,
                                                 uint32_t width, const float4 *__restrict__ skin, uint32_t tw, uint32_t th)
{
    uint32_t id[kMsaaSamples], db[kMsaaSamples];
    float ar[kMsaaSamples], ag[kMsaaSamples], ab[kMsaaSamples], aa[kMsaaSamples];
    uint32_t todo = 0;                                           // samples that hold a body and have no fragment yet
#pragma unroll
    for (uint32_t k = 0; k < kMsaaSamples; ++k) {
        const uint64_t key = keys[c * kMsaaSamples + k];
        id[k] = (uint32_t)key, db[k] = (uint32_t)(key >> 32);
        if (key != ~0ull) todo |= 1u << k;
        ar[k] = 0.1f, ag[k] = 0.2f, ab[k] = 0.3f, aa[k] = 1.0f;  // the clear colour
    }
    const float xc = (float)c + 0.5f;
    while (todo) {
        uint32_t j;                                              // the body of the lowest sample left, and its samples
        uint32_t mine = raster_lowest_body(todo, id, j);
        todo &= ~mine;
        float P[3][4];
        raster_vertices(C, inst, j, P);
#pragma unroll
        for (int e = 0; e < 3; ++e) {                            // M3: the first edge in draw order
            EyeSeg g{};
            Tex x{};
            if (!mine || !eye_edge(P[e], P[e == 2 ? 0 : e + 1], h, width, g, &x)) continue;
            uint32_t hit = 0;
#pragma unroll
            for (uint32_t k = 0; k < kMsaaSamples; ++k) {
                if (!(mine >> k & 1u)) continue;
                const float xk = (float)c + eye_msaa_offset(k);
                if (!(g.xa <= xk && xk < g.xb)) continue;
                const float t = (xk - g.xs0) / g.dx;
                float d;
                if (raster_depth(g.d0, g.dd, t, d) && __float_as_uint(d) == db[k]) hit |= 1u << k;
            }
            if (!hit) continue;
            mine &= ~hit;
            const float4 px = raster_fragment(x, e, (xc - g.xs0) / g.dx, skin, tw, th);   // M4: once per (column, body, edge)
#pragma unroll
            for (uint32_t k = 0; k < kMsaaSamples; ++k)
                if (hit >> k & 1u) ar[k] = px.x, ag[k] = px.y, ab[k] = px.z, aa[k] = px.w;
        }
        // (a sample left in `mine` keeps the clear colour: its key came from one of the three edges, so this is not reached)
    }
    return make_float4(raster_mean8(ar), raster_mean8(ag), raster_mean8(ab), raster_mean8(aa));   // M5
}

#ifdef __HIPCC__
// eye_row_fill's cover for 8 samples per column: the owning lane takes a column's eight samples, the wave 8 columns x 8 samples
struct EyeCover8 {
    static constexpr uint32_t kOwnCols = kMsaaOwnCols;
    static __device__ __forceinline__ void own(uint64_t *keys, uint32_t c, const EyeSeg &s, uint32_t j)
    {
#pragma unroll
        for (uint32_t m = 0; m < kMsaaSamples; ++m) eye_msaa_cover(keys, c, m, s, j);
    }
    static __device__ __forceinline__ void wave(uint64_t *keys, uint32_t lane, const EyeSeg &b, uint32_t bj)
    {
        for (uint32_t c = b.lo + (lane >> 3); c < b.hi; c += 8u) eye_msaa_cover(keys, c, lane & 7u, b, bj);   // c < width
    }
};

__global__ __launch_bounds__(kEyeBlock) void eyes_msaa_kernel(uint32_t n_total, uint32_t first, uint32_t count,
                                                             const float4 *__restrict__ cams, const float4 *__restrict__ inst,
                                                             uint32_t width, uint32_t see_self, const float4 *__restrict__ skin,
                                                             uint32_t tw, uint32_t th, uint32_t *__restrict__ ids8,
                                                             float *__restrict__ depth8, float4 *__restrict__ rgba,
                                                             uint32_t *__restrict__ bgra8)
{
    extern __shared__ uint64_t msaa_keys[];   // 8 * width entries, then T
    static_assert(kEyeBlock == 256, "one lane copies one entry of T");
    const uint32_t cells = width * kMsaaSamples;
    float *enc = reinterpret_cast<float *>(msaa_keys + cells);
    enc[threadIdx.x] = kSrgbEncodeT[threadIdx.x];   // (the first barrier below orders it)
    const uint32_t tid = threadIdx.x;
    const float h = (float)width * 0.5f;      // exact
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        for (uint32_t i = tid; i < cells; i += kEyeBlock) msaa_keys[i] = ~0ull;
        __syncthreads();
        float C[16];
        raster_load16(cams + (size_t)e * 4, C);
        eye_row_fill<kEyeBlock, EyeCover8>(msaa_keys, C, inst, n_total, first + e, see_self, h, width);
        __syncthreads();
        const size_t row = (size_t)e * cells;
        if (ids8 || depth8)
            for (uint32_t i = tid; i < cells; i += kEyeBlock) {   // the keys as they lie: (e * width + c) * 8 + k
                const uint64_t key = msaa_keys[i];
                if (ids8) ids8[row + i] = raster_key_id(key);
                if (depth8) depth8[row + i] = raster_key_depth(key);
            }
        if (rgba || bgra8)
            for (uint32_t c = tid; c < width; c += kEyeBlock) {
                const float4 px = eye_msaa_shade(msaa_keys, c, C, inst, h, width, skin, tw, th);
                const size_t o = (size_t)e * width + c;
                if (rgba) rgba[o] = px;
                if (bgra8) bgra8[o] = raster_bgra8(enc, px);
            }
        __syncthreads();   // the next eye re-initialises the keys
    }
}

// Up to 64 KiB of dynamic LDS a kernel may ask for as it is; above that (width > 1008) the runtime wants to be told once per device,
// and telling it again costs nothing that matters beside the launch.
hipError_t launch_eyes_msaa(uint32_t n_total, uint32_t first, uint32_t count, const float *cams, const float *inst, uint32_t width,
                            uint32_t flags, const float *skin, uint32_t tw, uint32_t th, uint32_t *ids8, float *depth8, float *rgba,
                            uint32_t *bgra8, hipStream_t s)
{
    const uint32_t grid = count < kEyeMaxGrid ? count : kEyeMaxGrid;
    const size_t lds = (size_t)width * kMsaaSamples * sizeof(uint64_t) + 256 * sizeof(float);
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute((const void *)eyes_msaa_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(eyes_msaa_kernel, dim3(grid), dim3(kEyeBlock), lds, s, n_total, first, count, (const float4 *)cams,
                       (const float4 *)inst, width, flags & 1u, (const float4 *)skin, tw, th, ids8, depth8, (float4 *)rgba, bgra8);
    return hipGetLastError();
}
#endif   // __HIPCC__
