// nb_scenes_seen.inc -- the seen boids step for scene batches (DESIGN.md section 14.1): every body of every scene folds over what its
// own eye sees of its own scene, in ONE kernel per step for the whole batch.  The eye's row is resolved in LDS as eyes_kernel resolves
// it, reduced there to a membership bitmap, and the fold walks the set bits in ascending order: no row and no list reaches device
// memory.  Every scene gets the bits nb_step_boids_seen gives a context of its n bodies (SV1): the raster is nb_raster.inc's and
// nb_eyes.inc's, unchanged; the fold is boids_seen_kernel's pair code, repeated here, and nb_boids.inc's boids_finish.
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit behind nb_eyes.inc, nb_seen.inc and nb_scenes.inc: NOT in the
// two units whose device code kernel_code_sha() hashes.  Launchers: nb_scenes.h.
//
// Why the bits are the chain's.  The row is an order-independent 64-bit minimum, so neither the workgroup's shape nor the order the
// candidates arrive in can change a key.  The seen list (S1-S3) is the set of ids in the row, ascending, without duplicates and with
// no entry >= n; V2 folds it in that order, which is the order a bitmap's set bits are walked in, lowest word and lowest bit first.
// With flags = 0 the eye does not draw its own body, so the self entry never occurs, and V2's `i == n` test stays anyway.
//
// Shape: one workgroup per eye b = s n + i (a grid-stride loop over the eyes, eyes_kernel's cap), 64 lanes where n <= 128 -- one wave
// per eye, two passes over the bodies at most, a barrier that costs nothing -- and 256 lanes above.  Dynamic LDS: width keys of 8 bytes
// and 256 bytes of bitmap (kScenesMaxBodies bits).  Per eye:
//   1  clear the keys and the bitmap; barrier
//   2  eyes_kernel<false>'s loop body over bodies j = 0 .. n-1 of scene s, j = i skipped, the matrices read at inst + s n; keys carry j
//   3  barrier; every column whose id is not NB_EYES_NONE ORs its bit into the bitmap (an LDS atomic)
//   4  barrier; kEmit = false: lane 0 folds body i over the set bits, gathers the 16-byte records of scene s, runs the epilogue and
//      writes record b.  kEmit = true (SV3): a member's slot is the number of set bits below it -- popcounts of the lower words and of
//      the lower bits of its own --; the list is staged in the keys' LDS and leaves coalesced, NB_EYES_NONE behind the count
//   5  barrier before the next eye re-initialises LDS

static constexpr uint32_t kScenesSeenWords = kScenesMaxBodies / 32u;   // the bitmap: one bit per body of a scene, 256 bytes

#ifdef __HIPCC__
template <int LANES, bool kEmit>
__global__ __launch_bounds__(LANES) void scenes_boids_seen_kernel(BoidsArgs a, uint32_t n, uint32_t first_eye, uint32_t count,
                                                                 const float4 *__restrict__ cams, const float4 *__restrict__ inst,
                                                                 uint32_t width, uint32_t *__restrict__ seen_count,
                                                                 uint32_t *__restrict__ seen_ids)
{
    extern __shared__ uint64_t scenes_seen_keys[];                                     // width entries
    uint32_t *bitmap = reinterpret_cast<uint32_t *>(scenes_seen_keys + width);         // kScenesSeenWords words
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t words = (n + 31u) >> 5;
    const float h = (float)width * 0.5f;     // exact
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const uint32_t b = first_eye + e, s = b / n, self = b - s * n;
        const float4 *__restrict__ inst_s = inst + (size_t)s * n * 4;
        for (uint32_t c = tid; c < width; c += LANES) scenes_seen_keys[c] = ~0ull;
        for (uint32_t w = tid; w < kScenesSeenWords; w += LANES) bitmap[w] = 0u;
        __syncthreads();
        float C[16];
        raster_load16(cams + (size_t)b * 4, C);
        for (uint32_t j0 = 0; j0 < n; j0 += LANES) {   // every lane of the workgroup runs every pass (the wave loops below)
            const uint32_t j = j0 + tid;
            float P[3][4] = {};
            bool live = j < n && j != self;
            if (live) live = raster_vertices_culled(C, inst_s, j, P);   // a body wholly behind the eye stops at its z rows
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                EyeSeg g{};
                const bool has = live && eye_edge(P[k], P[k == 2 ? 0 : k + 1], h, width, g);
                uint32_t rest = 0;   // first column left to the wave (rest < g.hi: some are)
                if (has) {
                    const uint32_t own = g.hi - g.lo < kEyeOwnCols ? g.hi : g.lo + kEyeOwnCols;
                    for (uint32_t c = g.lo; c < own; ++c) eye_cover(scenes_seen_keys, c, g, j);
                    rest = own;
                }
                uint64_t wide = __ballot(has && rest < g.hi);
                while (wide) {
                    const int src = __ffsll((unsigned long long)wide) - 1;
                    wide &= wide - 1;
                    const EyeSeg bg = eye_seg_bcast(g, rest, src);
                    const uint32_t bj = eye_bcast(j, src);
                    for (uint32_t c = bg.lo + lane; c < bg.hi; c += 64u) eye_cover(scenes_seen_keys, c, bg, bj);
                }
            }
        }
        __syncthreads();
        for (uint32_t c = tid; c < width; c += LANES) {
            const uint32_t id = raster_key_id(scenes_seen_keys[c]);
            if (id != kSeenNone && id < n) atomicOr(bitmap + (id >> 5), 1u << (id & 31u));   // (a key's id is a j < n: the test keeps the OR inside the bitmap)
        }
        __syncthreads();
        if constexpr (!kEmit) {
            if (tid == 0) {
                const float4 *__restrict__ pos_s = a.pos_in + (size_t)s * n, *__restrict__ vel_s = a.vel_in + (size_t)s * n;
                const float4 pn = pos_s[self], vn = vel_s[self];
                BoidsAcc acc{};                                                        // main.rs:472, 483, 495
                for (uint32_t w = 0; w < words; ++w) {
                    uint32_t m = bitmap[w];
                    while (m) {
                        const uint32_t i = (w << 5) + (uint32_t)(__ffs((int)m) - 1);
                        m &= m - 1u;
                        if (i == self || i >= n) continue;                             // main.rs:475 n != i; an entry outside the scene is not read
                        // boids_seen_kernel's pair code, repeated (nb_seen.inc keeps its text, and its kernel its instructions)
                        const float4 pj = pos_s[i], vj = vel_s[i];
                        const float dx = pj.x - pn.x, dy = pj.y - pn.y, dz = pj.z - pn.z;     // distance2: (other - self)
                        const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
                        const float ex = vj.x - vn.x, ey = vj.y - vn.y, ez = vj.z - vn.z;
                        const float e2 = ((ex * ex) + (ey * ey)) + (ez * ez);
                        if (d2 < a.r1) {                                                      // main.rs:474-476
                            acc.cx = acc.cx + pj.x, acc.cy = acc.cy + pj.y, acc.cz = acc.cz + pj.z;
                            acc.cnt = acc.cnt + 1.f;
                        }
                        if (d2 <= a.t2) acc.rx = acc.rx - dx, acc.ry = acc.ry - dy, acc.rz = acc.rz - dz;   // main.rs:485-487  sqrt(d2) < rule_2_distance
                        if (e2 <= a.t3) {                                                     // main.rs:497-499  sqrt(e2) < rule_3_distance
                            acc.mx = acc.mx + vj.x, acc.my = acc.my + vj.y, acc.mz = acc.mz + vj.z;
                            acc.vcnt = acc.vcnt + 1.f;
                        }
                    }
                }
                boids_finish(a, acc, b, pn);                                           // a.first = 0: record b of the batch
            }
        } else {
            uint32_t *list = reinterpret_cast<uint32_t *>(scenes_seen_keys);           // the keys are spent: width slots of the list
            uint32_t total = 0;
            for (uint32_t w = 0; w < words; ++w) total += (uint32_t)__popc(bitmap[w]);
            for (uint32_t i = tid; i < n; i += LANES) {
                const uint32_t w = i >> 5, bit = i & 31u, m = bitmap[w];
                if (!(m >> bit & 1u)) continue;
                uint32_t rank = (uint32_t)__popc(m & ((1u << bit) - 1u));
                for (uint32_t v = 0; v < w; ++v) rank += (uint32_t)__popc(bitmap[v]);
                list[rank] = i;                                                        // rank < total <= width: a column holds one id
            }
            __syncthreads();
            if (seen_count && tid == 0) seen_count[e] = total;
            if (seen_ids)
                for (uint32_t k = tid; k < width; k += LANES) seen_ids[(size_t)e * width + k] = k < total ? list[k] : kSeenNone;
        }
        __syncthreads();   // the next eye re-initialises the keys and the bitmap
    }
}

template <bool kEmit>
static hipError_t launch_scenes_seen_form(const BoidsArgs &a, uint32_t n, uint32_t first_eye, uint32_t count, const float *cams,
                                          const float *inst, uint32_t width, uint32_t *seen_count, uint32_t *seen_ids, hipStream_t s)
{
    const size_t lds = (size_t)width * sizeof(uint64_t) + kScenesSeenWords * sizeof(uint32_t);   // 32 KiB + 256 B at width 4096
    const uint32_t grid = count < kEyeMaxGrid ? count : kEyeMaxGrid;
    if (n <= kScenesSeenWaveBodies)
        hipLaunchKernelGGL((scenes_boids_seen_kernel<64, kEmit>), dim3(grid), dim3(64), lds, s, a, n, first_eye, count, (const float4 *)cams,
                           (const float4 *)inst, width, seen_count, seen_ids);
    else
        hipLaunchKernelGGL((scenes_boids_seen_kernel<256, kEmit>), dim3(grid), dim3(256), lds, s, a, n, first_eye, count, (const float4 *)cams,
                           (const float4 *)inst, width, seen_count, seen_ids);
    return hipGetLastError();
}

hipError_t launch_scenes_boids_seen(const BoidsArgs &c, uint32_t scenes, const float *cams, const float *inst, uint32_t width, hipStream_t s)
{
    return launch_scenes_seen_form<false>(c, c.n_total, 0u, scenes * c.n_total, cams, inst, width, nullptr, nullptr, s);
}

hipError_t launch_scenes_seen(uint32_t n, uint32_t first_eye, uint32_t count, const float *cams, const float *inst, uint32_t width,
                              uint32_t *seen_count, uint32_t *seen_ids, hipStream_t s)
{
    return launch_scenes_seen_form<true>(BoidsArgs{}, n, first_eye, count, cams, inst, width, seen_count, seen_ids, s);
}
#endif   // __HIPCC__
