// nb_scenes.inc -- scene batches (DESIGN.md section 14): B independent scenes of n <= 2 048 bodies, stepped k times by ONE launch, one
// workgroup per scene, the scene's state in LDS and registers between the steps.  Every scene follows the reference's law exactly as
// step_strict_kernel / boids_step_kernel apply it to a set of n bodies: the same device functions fold the same records in the same
// order, so the bits are theirs.
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit behind nb_located.inc: NOT in the two units whose device code
// kernel_code_sha() hashes.  Launchers: nb_scenes.h.
//
// Shape of both kernels.  The workgroup is the smallest of 64 / 128 / 256 / 512 / 1024 lanes that holds n; lane t owns body t and, in a
// scene of more than 1 024 bodies, body t + 1024 (TWO).  A scene's records are read from global memory once, live in two LDS buffers
// that the steps alternate between, and are written back after step k: a workgroup holds its whole scene on chip before it writes
// anything, so the update is in place (B4), and no workgroup ever touches another scene's records (B3).  Per step a lane folds
// j = 0 .. n-1 in index order from the current buffer, integrates, writes its new record into the other buffer and waits at ONE
// barrier: whoever passes barrier s has seen every wave finish the reads of step s, so step s + 1 may overwrite the buffer step s read.
// More scenes than kScenesMaxGrid workgroups are walked by a grid-stride loop; after the last barrier of a scene nothing reads LDS
// (the final records leave from registers), so the next scene may be staged at once.
//
// Gravity: the divide guard and the planar shortcut are decided per scene and per step from the records that step reads -- every lane
// flags its own record as it writes it (coord_oor, nonzero_bits), the wave ORs (wave_or), one LDS word per wave and buffer -- as
// step_strict_kernel decides them per tile.  A coarser decision than per tile of 1 024 records, and as exact: every path gives the
// reference's bits wherever the guard admits it.
// Boids: boids_pair's select form (3-D, i != n tested, a skipped sum untouched whatever the record holds), valid for any record, so
// no flags; the epilogue is boids_finish_records, the arithmetic of boids_finish.  The buffers hold (px, py, vx, vy) and (pz, vz) as
// the boids tiles do: 24 n bytes each, 96 KiB for two at n = 2 048.

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t scenes_record_flags(const float4 p, uint32_t lo, uint32_t span)
{
    return coord_oor(p.x, lo, span) | coord_oor(p.y, lo, span) | coord_oor(p.z, lo, span) | nonzero_bits(p.z);
}

template <int LANES, bool TWO>
__global__ __launch_bounds__(LANES) void scenes_nbody_kernel(ScenesNbodyArgs a)
{
    extern __shared__ float4 scenes_lds[];   // [2][n] records (x, y, z, bias) in tile_store's form, then [2][W] flag words
    constexpr int W = LANES / 64;
    constexpr int U = LANES == 1024 ? 4 : 8;  // pairs in flight per lane: 1 024 lanes leave each 128 registers
    const uint32_t t = threadIdx.x, wave = t >> 6, n = a.n;
    uint32_t *flag_words = reinterpret_cast<uint32_t *>(scenes_lds + 2u * n);
    const uint32_t lo = a.lo_bits, span = a.hi_bits - a.lo_bits;
    const uint32_t forced = a.force_ieee | a.force_3d;
    const bool live0 = t < n, live1 = TWO && t + (uint32_t)LANES < n;
    for (uint32_t s = blockIdx.x; s < a.scenes; s += gridDim.x) {
        float4 *pos = a.pos + (size_t)s * n, *vel = a.vel + (size_t)s * n;
        float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), v0 = p0, p1 = p0, v1 = p0;
        uint32_t f = 0;
        if (live0) {
            p0 = pos[t], v0 = vel[t];
            scenes_lds[t] = make_float4(p0.x, p0.y, p0.z, a.bias);
            f |= scenes_record_flags(p0, lo, span);
        }
        if (TWO && live1) {
            p1 = pos[t + LANES], v1 = vel[t + LANES];
            scenes_lds[t + LANES] = make_float4(p1.x, p1.y, p1.z, a.bias);
            f |= scenes_record_flags(p1, lo, span);
        }
        f = wave_or(f);
        if ((t & 63u) == 0u) flag_words[wave] = f;
        __syncthreads();
        uint32_t cur = 0;
        for (uint32_t step = 0; step < a.k; ++step) {
            const float4 *tile = scenes_lds + cur * n;
            float4 *next = scenes_lds + (cur ^ 1u) * n;
            uint32_t sf = forced;
#pragma unroll
            for (int w = 0; w < W; ++w) sf |= flag_words[cur * W + w];
            sf = (uint32_t)__builtin_amdgcn_readfirstlane((int)sf);
            uint32_t nf = 0;
            auto body = [&](float4 &p, float4 &v, uint32_t b) {
                float sx = 0.f, sy = 0.f, sz = 0.f;  // main.rs:426
                if (sf == 0u)
                    fold_tile_strict<false, true, U, 1>(tile, (int)n, 0, p.x, p.y, p.z, a.G, sx, sy, sz);
                else if ((sf & kFlagIeee) == 0u)
                    fold_tile_strict<false, false, U, 1>(tile, (int)n, 0, p.x, p.y, p.z, a.G, sx, sy, sz);
                else
                    fold_tile_strict<true, false, 2, 1>(tile, (int)n, 0, p.x, p.y, p.z, a.G, sx, sy, sz);
                integrate(p, v, sx, sy, sz, a.dt);
                next[b] = make_float4(p.x, p.y, p.z, a.bias);
                nf |= scenes_record_flags(p, lo, span);
            };
            if (live0) body(p0, v0, t);
            if (TWO && live1) body(p1, v1, t + LANES);
            nf = wave_or(nf);
            if ((t & 63u) == 0u) flag_words[(cur ^ 1u) * W + wave] = nf;
            __syncthreads();
            cur ^= 1u;
        }
        if (live0) pos[t] = p0, vel[t] = v0;
        if (TWO && live1) pos[t + LANES] = p1, vel[t + LANES] = v1;
    }
}

template <int LANES, bool TWO>
__global__ __launch_bounds__(LANES) void scenes_boids_kernel(BoidsArgs a, float4 *pos_all, float4 *vel_all, uint32_t scenes, uint32_t k)
{
    extern __shared__ float4 scenes_lds[];   // [2][n] records (px, py, vx, vy), then [2][n] records (pz, vz)
    const uint32_t t = threadIdx.x, n = a.n_total;
    float2 *z_lds = reinterpret_cast<float2 *>(scenes_lds + 2u * n);
    const bool live0 = t < n, live1 = TWO && t + (uint32_t)LANES < n;
    for (uint32_t s = blockIdx.x; s < scenes; s += gridDim.x) {
        float4 *pos = pos_all + (size_t)s * n, *vel = vel_all + (size_t)s * n;
        float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), v0 = p0, p1 = p0, v1 = p0;
        if (live0) {
            p0 = pos[t], v0 = vel[t];
            scenes_lds[t] = make_float4(p0.x, p0.y, v0.x, v0.y);
            z_lds[t] = make_float2(p0.z, v0.z);
        }
        if (TWO && live1) {
            p1 = pos[t + LANES], v1 = vel[t + LANES];
            scenes_lds[t + LANES] = make_float4(p1.x, p1.y, v1.x, v1.y);
            z_lds[t + LANES] = make_float2(p1.z, v1.z);
        }
        __syncthreads();
        uint32_t cur = 0;
        for (uint32_t step = 0; step < k; ++step) {
            const float4 *tpv = scenes_lds + cur * n;
            const float2 *tz = z_lds + cur * n;
            float4 *npv = scenes_lds + (cur ^ 1u) * n;
            float2 *nz = z_lds + (cur ^ 1u) * n;
            auto body = [&](float4 &p, float4 &v, uint32_t b) {
                BoidsAcc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // main.rs:472, 483, 495
                if (LANES < 1024) {  // two register sets of eight records, one read ahead of the other
                    boids_fold_tile<true, false, false, false, false, 0>(acc, tpv, tz, (int)n, 0u, b, p, v, a.r1, a.t2, a.t3, a.mk);
                } else {  // 1 024 lanes leave each 128 registers, and four waves a SIMD to hide the reads behind
#pragma unroll 4
                    for (uint32_t j = 0; j < n; ++j)
                        boids_pair<true, false, false, false, 0>(acc, tpv[j], tz[j], j, b, p, v, a.r1, a.t2, a.t3, a.mk);
                }
                float4 pn, vn;
                boids_finish_records(a, acc, p, pn, vn);
                p = pn, v = vn;
                npv[b] = make_float4(p.x, p.y, v.x, v.y);
                nz[b] = make_float2(p.z, v.z);
            };
            if (live0) body(p0, v0, t);
            if (TWO && live1) body(p1, v1, t + LANES);
            __syncthreads();
            cur ^= 1u;
        }
        if (live0) pos[t] = p0, vel[t] = v0;
        if (TWO && live1) pos[t + LANES] = p1, vel[t + LANES] = v1;
    }
}

// the workgroup a scene of n bodies takes: f.template operator()<LANES, TWO>()
template <typename F>
static hipError_t scenes_by_size(uint32_t n, F f)
{
    if (n <= 64u) return f.template operator()<64, false>();
    if (n <= 128u) return f.template operator()<128, false>();
    if (n <= 256u) return f.template operator()<256, false>();
    if (n <= 512u) return f.template operator()<512, false>();
    if (n <= 1024u) return f.template operator()<1024, false>();
    return f.template operator()<1024, true>();
}

// The launch of a one-workgroup-per-scene kernel of LANES lanes: above 64 KiB of LDS the function's dynamic limit is raised first (as
// nb_eyes_msaa.inc's launcher does); more scenes than kScenesMaxGrid are the kernel's grid-stride loop's
template <int LANES, class K, class... A>
static hipError_t launch_scenes_scene(K kernel, uint32_t scenes, size_t lds, hipStream_t s, A... args)
{
    if (lds > 65536u) {
        const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const uint32_t grid = scenes < kScenesMaxGrid ? scenes : kScenesMaxGrid;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(LANES), lds, s, args...);
    return hipGetLastError();
}

struct ScenesNbodyLaunch {
    const ScenesNbodyArgs &a;
    hipStream_t s;
    template <int LANES, bool TWO>
    hipError_t operator()() const
    {
        const size_t lds = (size_t)a.n * 2u * sizeof(float4) + 2u * (LANES / 64) * sizeof(uint32_t);   // 64 KiB + 128 B at n = 2 048
        return launch_scenes_scene<LANES>(scenes_nbody_kernel<LANES, TWO>, a.scenes, lds, s, a);
    }
};
hipError_t launch_scenes_nbody(const ScenesNbodyArgs &a, hipStream_t s) { return scenes_by_size(a.n, ScenesNbodyLaunch{a, s}); }

struct ScenesBoidsLaunch {
    const BoidsArgs &c;
    float4 *pos, *vel;
    uint32_t scenes, k;
    hipStream_t s;
    template <int LANES, bool TWO>
    hipError_t operator()() const
    {
        const size_t lds = (size_t)c.n_total * 2u * (sizeof(float4) + sizeof(float2));   // 96 KiB at n = 2 048
        return launch_scenes_scene<LANES>(scenes_boids_kernel<LANES, TWO>, scenes, lds, s, c, pos, vel, scenes, k);
    }
};
hipError_t launch_scenes_boids(const BoidsArgs &c, float4 *pos, float4 *vel, uint32_t scenes, uint32_t k, hipStream_t s)
{
    return scenes_by_size(c.n_total, ScenesBoidsLaunch{c, pos, vel, scenes, k, s});
}
#endif   // __HIPCC__
