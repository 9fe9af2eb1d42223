// nb_eyes_msaa.inc -- every entity's eye view through 8 samples per column, resolved (DESIGN.md section 10, steps M1-M5): what the
// reference's eye targets hold with msaa_samples = 8 (src/main.rs:652; sample_count, :263; resolve_target, :547, :611).
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit after nb_frame.inc; nb_eyes.inc is used as it is (eye_edge,
// eye_key_load, eye_bcast, eye_srgb_byte, kSrgbEncodeT) and not edited.  Launcher: nb_eyes.h.
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

static constexpr uint32_t kMsaaSamples = 8;
static constexpr uint32_t kMsaaOwnCols = 4;               // columns of a span its own lane walks; the rest goes to the whole wave
static constexpr uint32_t kMsaaOffsets16 = 0xFB135D79u;   // nibble k = 16 o_k

__device__ __forceinline__ float eye_msaa_offset(uint32_t k) { return (float)((kMsaaOffsets16 >> (4u * k)) & 15u) * 0.0625f; }   // exact

// sample k of column c of segment s of body j; keys: the eye's, sample-minor
__device__ __forceinline__ void eye_msaa_cover(uint64_t *keys, uint32_t c, uint32_t k, const EyeSeg &s, uint32_t j)
{
    const float x = (float)c + eye_msaa_offset(k);                              // exact
    if (!(s.xa <= x && x < s.xb)) return;
    uint64_t *slot = keys + (c * kMsaaSamples + k);
    if ((((uint64_t)s.klow << 32) | j) >= eye_key_load(slot)) return;           // nothing this segment writes here can win
    const float t = (x - s.xs0) / s.dx;
    const float q = t * s.dd;
    float d = s.d0 + q;
    if (!(d < 1.0f)) return;                                                    // Less against the clear value; NaN never passes
    if (!(d > 0.0f)) d = 0.0f;
    const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | j;
    if (key < eye_key_load(slot)) __hip_atomic_fetch_min(slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// M4: the fragment of edge `edge` (clipped: g, x) in the column whose centre is xc -- steps 7-10
__device__ __forceinline__ float4 eye_msaa_fragment(const EyeSeg &g, const EyeTex &x, int edge, float xc, const float4 *__restrict__ skin,
                                                    uint32_t tw, uint32_t th)
{
    const float t = (xc - g.xs0) / g.dx;
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
        for (int e = 0; e < 3; ++e) {                            // M3: the first edge in draw order
            EyeSeg g{};
            EyeTex x{};
            if (!mine || !eye_edge(P[e], P[e == 2 ? 0 : e + 1], h, width, g, &x)) continue;
            uint32_t hit = 0;
#pragma unroll
            for (uint32_t k = 0; k < kMsaaSamples; ++k) {
                if (!(mine >> k & 1u)) continue;
                const float xk = (float)c + eye_msaa_offset(k);
                if (!(g.xa <= xk && xk < g.xb)) continue;
                const float t = (xk - g.xs0) / g.dx;
                const float q = t * g.dd;
                float d = g.d0 + q;
                if (!(d < 1.0f)) continue;
                if (!(d > 0.0f)) d = 0.0f;
                if (__float_as_uint(d) == db[k]) hit |= 1u << k;
            }
            if (!hit) continue;
            mine &= ~hit;
            const float4 px = eye_msaa_fragment(g, x, e, xc, skin, tw, th);   // M4: once per (column, body, edge)
#pragma unroll
            for (uint32_t k = 0; k < kMsaaSamples; ++k)
                if (hit >> k & 1u) ar[k] = px.x, ag[k] = px.y, ab[k] = px.z, aa[k] = px.w;
        }
        // (a sample left in `mine` keeps the clear colour: its key came from one of the three edges, so this is not reached)
    }
    float4 o;                                                    // M5
    o.x = (((ar[0] + ar[1]) + (ar[2] + ar[3])) + ((ar[4] + ar[5]) + (ar[6] + ar[7]))) * 0.125f;
    o.y = (((ag[0] + ag[1]) + (ag[2] + ag[3])) + ((ag[4] + ag[5]) + (ag[6] + ag[7]))) * 0.125f;
    o.z = (((ab[0] + ab[1]) + (ab[2] + ab[3])) + ((ab[4] + ab[5]) + (ab[6] + ab[7]))) * 0.125f;
    o.w = (((aa[0] + aa[1]) + (aa[2] + aa[3])) + ((aa[4] + aa[5]) + (aa[6] + aa[7]))) * 0.125f;
    return o;
}

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
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const float h = (float)width * 0.5f;      // exact
    const float ax[3] = {-1.0f, 1.0f, -1.0f}, ay[3] = {-1.0f, 0.0f, 1.0f};
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        for (uint32_t i = tid; i < cells; i += kEyeBlock) msaa_keys[i] = ~0ull;
        __syncthreads();
        float C[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 v = cams[(size_t)e * 4 + k];
            C[4 * k] = v.x, C[4 * k + 1] = v.y, C[4 * k + 2] = v.z, C[4 * k + 3] = v.w;
        }
        const uint32_t self = first + e;
        for (uint32_t j0 = 0; j0 < n_total; j0 += kEyeBlock) {   // every lane of the workgroup runs every pass (the wave loops below)
            const uint32_t j = j0 + tid;
            float P[3][4] = {};
            bool live = j < n_total && (see_self || j != self);
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
                for (int v = 0; v < 3; ++v) {   // the near plane's row first: a body wholly behind the eye stops here
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
                EyeSeg s{};
                const bool has = live && eye_edge(P[k], P[k == 2 ? 0 : k + 1], h, width, s);   // [s.lo, s.hi) holds every covered sample's column too
                uint32_t rest = 0;   // first column left to the wave (rest < s.hi: some are)
                if (has) {
                    const uint32_t own = s.hi - s.lo < kMsaaOwnCols ? s.hi : s.lo + kMsaaOwnCols;
                    for (uint32_t c = s.lo; c < own; ++c)
#pragma unroll
                        for (uint32_t m = 0; m < kMsaaSamples; ++m) eye_msaa_cover(msaa_keys, c, m, s, j);
                    rest = own;
                }
                uint64_t wide = __ballot(has && rest < s.hi);
                while (wide) {
                    const int src = __ffsll((unsigned long long)wide) - 1;
                    wide &= wide - 1;
                    EyeSeg b;
                    b.xs0 = eye_bcast(s.xs0, src), b.xs1 = eye_bcast(s.xs1, src), b.d0 = eye_bcast(s.d0, src), b.d1 = eye_bcast(s.d1, src);
                    b.dx = eye_bcast(s.dx, src), b.dd = eye_bcast(s.dd, src), b.xa = eye_bcast(s.xa, src), b.xb = eye_bcast(s.xb, src);
                    b.klow = eye_bcast(s.klow, src), b.lo = eye_bcast(rest, src), b.hi = eye_bcast(s.hi, src);
                    const uint32_t bj = eye_bcast(j, src);
                    for (uint32_t c = b.lo + (lane >> 3); c < b.hi; c += 8u) eye_msaa_cover(msaa_keys, c, lane & 7u, b, bj);   // c < width
                }
            }
        }
        __syncthreads();
        const size_t row = (size_t)e * cells;
        if (ids8 || depth8)
            for (uint32_t i = tid; i < cells; i += kEyeBlock) {   // the keys as they lie: (e * width + c) * 8 + k
                const uint64_t key = msaa_keys[i];
                const bool none = key == ~0ull;
                if (ids8) ids8[row + i] = none ? 0xFFFFFFFFu : (uint32_t)key;
                if (depth8) depth8[row + i] = none ? 1.0f : __uint_as_float((uint32_t)(key >> 32));
            }
        if (rgba || bgra8)
            for (uint32_t c = tid; c < width; c += kEyeBlock) {
                const float4 px = eye_msaa_shade(msaa_keys, c, C, inst, h, width, skin, tw, th);
                const size_t o = (size_t)e * width + c;
                if (rgba) rgba[o] = px;
                if (bgra8)   // bytes in memory B, G, R, A
                    bgra8[o] = eye_srgb_byte(enc, px.z) | eye_srgb_byte(enc, px.y) << 8 | eye_srgb_byte(enc, px.x) << 16 | 0xFF000000u;
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
