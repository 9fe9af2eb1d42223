// nb_eyes.inc -- every entity's eye view (DESIGN.md section 10): what the reference's depth attachment holds after its eye pass
// (src/main.rs:585-647, 962-998: one 1 x W layer per entity, the camera on the entity looking along its velocity, every instance drawn
// as the LineStrip 0-1-2-0 of its triangle, src/main.rs:130-138, 249, with depth test Less against a clear of 1.0, :256-260, 626),
// and which instance wrote each pixel.
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit: NOT in the two units whose device code kernel_code_sha()
// hashes (nenbody_amd/_lib.py), so the stamp of profiles/hbm_traffic.json stays that of the benchmarked kernels.  Launcher: nb_eyes.h.
// The vertex products, the clip, the depth of a parameter, the fragment and the sRGB bytes are nb_raster.inc's, shared with the
// frame; this file adds the projection onto a row, the column range and its lower depth bound, the cover, the shade and the kernel.
//
// The rule, one binary32 operation per step in the order written (-ffp-contract=off, IEEE '/'); tests/eyes_restatement.py states it
// again in numpy and the GPU tests compare every bit:
//   clip vertex  C (M a) for a = (-1,-1,0,1), (1,0,0,1), (-1,1,0,1); each row of each product ((m0 x + m1 y) + m2 z) + m3 w
//   edges        (a0,a1), (a1,a2), (a2,a0), clipped (Liang-Barsky) to z >= 0, w - z >= 0, w + y >= 0, w - y >= 0; no x planes
//   projection   xs = (x / w) * (W/2) + W/2, d = z / w; column c, centre xc = c + 0.5, covered iff min(xs) <= xc < max(xs)
//   depth        t = (xc - xs0) / (xs1 - xs0), d = d0 + t (d1 - d0); a candidate iff d < 1, then !(d > 0) -> +0
//   resolve      the minimum over bodies and edges of bits(d) << 32 | j: the nearest, ties to the lower index
// and, for the colour row (nb_eyes_colour; tests/eyes_colour_restatement.py), per resolved column:
//   edge         the first of the winner's edges 0, 1, 2 that covers the column, is a candidate and gives the key's depth bits
//   parameter    s0 = max(t_in, 0), s1 = min(t_out, 1), i = 1 / w of the clipped ends; s = (s0 i0 + t (s1 i1 - s0 i0)) / (i0 + t (i1 - i0))
//   coordinate   (u, v) = (0, s), (s, 1), (1 - s, 1 - s) for edge 0, 1, 2; texel (min(tw - 1, floor(u tw)), min(th - 1, floor(v th)))
//   colour       texel * (1 - ((u - 0.5)^2 + (v - 0.5)^2)), alpha 1; no winner: the clear colour (0.1, 0.2, 0.3, 1)
//   bgra8        per channel the number of thresholds T[1..255] <= c (nb_srgb_tables.h): the exact sRGB byte
//
// Shape: one workgroup of 256 lanes per eye (a grid-stride loop over the eyes); the eye's W keys in LDS (W <= 4096: 32 KB), resolved
// with ds_min_u64 -- the minimum does not depend on the order the candidates arrive in, so the result is deterministic.  A lane takes
// one body per pass: it clips the three edges, walks the first kEyeOwnCols columns of each span itself and hands the rest of a wide
// span to its whole wave (a near body covers hundreds of columns: one lane per body would leave the wave waiting on its widest span).
// Culls, none of which can change a bit: an edge whose ends are both outside one boundary is dropped before any divide (a body behind
// the eye costs its clip z rows only); a column is skipped before its divide when a lower bound of every key the segment can write
// there (klow, eye_edge) is not below the key in place; and the atomic only goes out when the key is below the key read just before.

static constexpr int kEyeBlock = 256;
static constexpr uint32_t kEyeOwnCols = 8;    // columns of a span its own lane walks; the rest goes to the whole wave
static constexpr uint32_t kEyeMaxGrid = 1u << 20;

struct EyeSeg {
    float xs0, xs1, d0, d1;  // projected ends
    float dx, dd;            // xs1 - xs0, d1 - d0
    float xa, xb;            // min / max of xs0, xs1
    uint32_t klow;           // bits of a lower bound of every depth this segment writes (the key's upper half)
    uint32_t lo, hi;         // a superset of the covered columns, [lo, hi)
};

// One edge P0 -> P1 of clip-space vertices (x, y, z, w): clipped, projected, its column range.  false: dropped, or covers no column.
// tx: what the colour row needs of the clipped edge beyond EyeSeg.
__device__ __forceinline__ bool eye_edge(const float *P0, const float *P1, float h, uint32_t width, EyeSeg &s, Tex *tx = nullptr)
{
    float Q0[4], Q1[4];
    Tex x;
    if (!raster_clip(P0, P1, Q0, Q1, x)) return false;
    if (tx) *tx = x;
    const float u0 = Q0[0] / Q0[3], u1 = Q1[0] / Q1[3];
    const float p0 = u0 * h, p1 = u1 * h;
    s.xs0 = p0 + h;
    s.xs1 = p1 + h;
    s.xa = (s.xs0 <= s.xs1) ? s.xs0 : s.xs1;
    s.xb = (s.xs0 <= s.xs1) ? s.xs1 : s.xs0;
    if (!(s.xa <= s.xb)) return false;                                          // a NaN end covers nothing
    // c covered => xa <= c + 0.5 < xb => floor(xa) - 1 < c < ceil(xb): a superset, clamped in float first (the ends may be infinite)
    const float lo = floorf(fmaxf(s.xa, -4.0f)) - 1.0f;
    const float hi = ceilf(fminf(s.xb, (float)width + 4.0f)) + 1.0f;
    s.lo = (uint32_t)fminf(fmaxf(lo, 0.0f), (float)width);
    s.hi = (uint32_t)fminf(fmaxf(hi, 0.0f), (float)width);
    if (s.lo >= s.hi) return false;
    s.d0 = Q0[2] / Q0[3];
    s.d1 = Q1[2] / Q1[3];
    s.dx = s.xs1 - s.xs0;
    s.dd = s.d1 - s.d0;
    // A lower bound of d = d0 + t * dd over the covered columns.  There 0 <= t <= 1 or t is NaN (xc lies between the ends and
    // rounding is monotone), so with dd >= 0 the product is >= 0 and d >= d0, and with dd < 0 the product is >= dd and
    // d >= fl(d0 + dd).  A NaN bound becomes 0 (no cull); a NaN d is never a candidate anyway.
    const float dlow = (s.d1 >= s.d0) ? s.d0 : s.d0 + s.dd;
    s.klow = __float_as_uint(dlow > 0.0f ? dlow : 0.0f);
    return true;
}

__device__ __forceinline__ uint64_t eye_key_load(uint64_t *k) { return __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// column c of segment s of body j
__device__ __forceinline__ void eye_cover(uint64_t *keys, uint32_t c, const EyeSeg &s, uint32_t j)
{
    const float xc = (float)c + 0.5f;                                           // exact
    if (!(s.xa <= xc && xc < s.xb)) return;
    if ((((uint64_t)s.klow << 32) | j) >= eye_key_load(keys + c)) return;       // nothing this segment writes here can win
    const float t = (xc - s.xs0) / s.dx;
    float d;
    if (!raster_depth(s.d0, s.dd, t, d)) return;
    const uint64_t key = raster_key(d, j);
    if (key < eye_key_load(keys + c)) __hip_atomic_fetch_min(keys + c, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// segment s of lane src for its whole wave, its range starting at that lane's `rest`
__device__ __forceinline__ EyeSeg eye_seg_bcast(const EyeSeg &s, uint32_t rest, int src)
{
    EyeSeg b;
    b.xs0 = eye_bcast(s.xs0, src), b.xs1 = eye_bcast(s.xs1, src), b.d0 = eye_bcast(s.d0, src), b.d1 = eye_bcast(s.d1, src);
    b.dx = eye_bcast(s.dx, src), b.dd = eye_bcast(s.dd, src), b.xa = eye_bcast(s.xa, src), b.xb = eye_bcast(s.xb, src);
    b.klow = eye_bcast(s.klow, src), b.lo = eye_bcast(rest, src), b.hi = eye_bcast(s.hi, src);
    return b;
}

// The colour of column c of one eye (rule steps 6-11), its key resolved: the winner's three edges again with eye_edge's own arithmetic,
// the first that covers c, is a candidate and gives the key's depth bits, then the texture coordinate, one texel, the vignette.
__device__ __forceinline__ float4 eye_shade(uint64_t key, uint32_t c, const float *C, const float4 *__restrict__ inst, float h,
                                            uint32_t width, const float4 *__restrict__ skin, uint32_t tw, uint32_t th)
{
    if (key == ~0ull) return raster_clear();
    const uint32_t j = (uint32_t)key, dbits = (uint32_t)(key >> 32);
    float P[3][4];
    raster_vertices(C, inst, j, P);
    const float xc = (float)c + 0.5f;
    int edge = -1;
    float t_at = 0.0f;
    Tex at{};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        EyeSeg g{};
        Tex x{};
        if (edge >= 0 || !eye_edge(P[k], P[k == 2 ? 0 : k + 1], h, width, g, &x)) continue;
        if (!(g.xa <= xc && xc < g.xb)) continue;
        const float t = (xc - g.xs0) / g.dx;
        float d;
        if (!raster_depth(g.d0, g.dd, t, d) || __float_as_uint(d) != dbits) continue;
        edge = k, t_at = t, at = x;
    }
    if (edge < 0) return raster_clear();   // (the key came from one of the three: not reached)
    return raster_fragment(at, edge, t_at, skin, tw, th);
}

#ifdef __HIPCC__
// What eye_row_fill leaves to the kind of row: how many columns of a span its own lane walks, that lane's call at one of them, and
// the wave's walk over a span handed to it (b.lo: the first column left).  Here one sample per column, a column per lane.
struct EyeCover1 {
    static constexpr uint32_t kOwnCols = kEyeOwnCols;
    static __device__ __forceinline__ void own(uint64_t *keys, uint32_t c, const EyeSeg &s, uint32_t j) { eye_cover(keys, c, s, j); }
    static __device__ __forceinline__ void wave(uint64_t *keys, uint32_t lane, const EyeSeg &b, uint32_t bj)
    {
        for (uint32_t c = b.lo + lane; c < b.hi; c += 64u) eye_cover(keys, c, b, bj);
    }
};

// The row of one eye, its keys cleared and a barrier behind the clearing: every body j < n_total of `inst` but `self` (unless
// see_self) into `keys`.  The ONE copy of the loop: eyes_kernel, eyes_msaa_kernel and the two scenes kernels (nb_scenes_seen.inc,
// nb_scenes_located.inc: see_self a literal 0u, inst the scene's) call it from workgroups of LANES lanes, all lanes together.
template <int LANES, class Cover>
__device__ __forceinline__ void eye_row_fill(uint64_t *keys, const float *C, const float4 *__restrict__ inst, uint32_t n_total, uint32_t self,
                                             uint32_t see_self, float h, uint32_t width)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t j0 = 0; j0 < n_total; j0 += LANES) {   // every lane of the workgroup runs every pass (the wave loops below)
        const uint32_t j = j0 + tid;
        float P[3][4] = {};
        bool live = j < n_total && (see_self || j != self);
        if (live) live = raster_vertices_culled(C, inst, j, P);   // a body wholly behind the eye stops at its z rows
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            EyeSeg s{};
            const bool has = live && eye_edge(P[k], P[k == 2 ? 0 : k + 1], h, width, s);   // [s.lo, s.hi) holds every covered sample's column too
            uint32_t rest = 0;   // first column left to the wave (rest < s.hi: some are)
            if (has) {
                const uint32_t own = s.hi - s.lo < Cover::kOwnCols ? s.hi : s.lo + Cover::kOwnCols;
                for (uint32_t c = s.lo; c < own; ++c) Cover::own(keys, c, s, j);
                rest = own;
            }
            uint64_t wide = __ballot(has && rest < s.hi);
            while (wide) {
                const int src = __ffsll((unsigned long long)wide) - 1;
                wide &= wide - 1;
                const EyeSeg b = eye_seg_bcast(s, rest, src);
                Cover::wave(keys, lane, b, eye_bcast(j, src));
            }
        }
    }
}

// kColour = false: ids / depth alone (nb_eyes, nb_launch_eyes).  kColour = true: the shading pass too, while the eye's keys are still
// in LDS -- a lane per column -- with T behind the keys in LDS (width * 8 + 1024 bytes); rgba is a float4 row, bgra8 a uint32 row.
template <bool kColour>
__global__ __launch_bounds__(kEyeBlock) void eyes_kernel(uint32_t n_total, uint32_t first, uint32_t count, const float4 *__restrict__ cams,
                                                        const float4 *__restrict__ inst, uint32_t width, uint32_t see_self,
                                                        uint32_t *__restrict__ ids, float *__restrict__ depth,
                                                        const float4 *__restrict__ skin, uint32_t tw, uint32_t th,
                                                        float4 *__restrict__ rgba, uint32_t *__restrict__ bgra8)
{
    extern __shared__ uint64_t eye_keys[];   // width entries
    float *enc = nullptr;                    // kColour: T behind the keys, 256 entries
    if constexpr (kColour) {
        static_assert(kEyeBlock == 256, "one lane copies one entry of T");
        enc = reinterpret_cast<float *>(eye_keys + width);
        enc[threadIdx.x] = kSrgbEncodeT[threadIdx.x];   // (the first barrier below orders it)
    }
    const uint32_t tid = threadIdx.x;
    const float h = (float)width * 0.5f;     // exact
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        for (uint32_t c = tid; c < width; c += kEyeBlock) eye_keys[c] = ~0ull;
        __syncthreads();
        float C[16];
        raster_load16(cams + (size_t)e * 4, C);
        eye_row_fill<kEyeBlock, EyeCover1>(eye_keys, C, inst, n_total, first + e, see_self, h, width);
        __syncthreads();
        for (uint32_t c = tid; c < width; c += kEyeBlock) {   // coalesced rows of ids and depths
            const uint64_t key = eye_keys[c];
            const size_t o = (size_t)e * width + c;
            if (ids) ids[o] = raster_key_id(key);
            if (depth) depth[o] = raster_key_depth(key);
            if constexpr (kColour) {
                const float4 px = eye_shade(key, c, C, inst, h, width, skin, tw, th);
                if (rgba) rgba[o] = px;
                if (bgra8) bgra8[o] = raster_bgra8(enc, px);
            }
        }
        __syncthreads();   // the next eye re-initialises the keys
    }
}

hipError_t launch_eyes(uint32_t n_total, uint32_t first, uint32_t count, const float *cams, const float *inst, uint32_t width,
                       uint32_t flags, uint32_t *ids, float *depth, hipStream_t s)
{
    const uint32_t grid = count < kEyeMaxGrid ? count : kEyeMaxGrid;
    hipLaunchKernelGGL(eyes_kernel<false>, dim3(grid), dim3(kEyeBlock), (size_t)width * sizeof(uint64_t), s, n_total, first, count,
                       (const float4 *)cams, (const float4 *)inst, width, flags & 1u, ids, depth, (const float4 *)nullptr, 0u, 0u,
                       (float4 *)nullptr, (uint32_t *)nullptr);
    return hipGetLastError();
}

hipError_t launch_eyes_colour(uint32_t n_total, uint32_t first, uint32_t count, const float *cams, const float *inst, uint32_t width,
                              uint32_t flags, const float *skin, uint32_t tw, uint32_t th, uint32_t *ids, float *depth, float *rgba,
                              uint32_t *bgra8, hipStream_t s)
{
    const uint32_t grid = count < kEyeMaxGrid ? count : kEyeMaxGrid;
    hipLaunchKernelGGL(eyes_kernel<true>, dim3(grid), dim3(kEyeBlock), (size_t)width * sizeof(uint64_t) + 256 * sizeof(float), s, n_total,
                       first, count, (const float4 *)cams, (const float4 *)inst, width, flags & 1u, ids, depth, (const float4 *)skin, tw,
                       th, (float4 *)rgba, bgra8);
    return hipGetLastError();
}
#endif   // __HIPCC__
