// nb_scenes_located.inc -- gravity from located vision for scene batches (DESIGN.md section 14.2): every body of every scene folds
// the reference's gravity law over WHERE its own eye sees the bodies of its own scene, in ONE kernel per step for the whole batch.
// The eye's row is resolved in LDS as eyes_kernel resolves it and reduced there to one 64-bit word per body of the scene -- the
// member's nearest depth and the least column holding it --; the located points and the quotients are formed from those words and the
// fold walks the members in ascending order: no row, no list and no located point reaches device memory.  Every scene gets the bits
// nb_step_nbody_located gives a context of its n bodies (SL1): the raster is nb_raster.inc's and nb_eyes.inc's, unchanged; L2-L4 are
// located_kernel's text and G2 is nbody_located_kernel's, repeated here, with nb_nbody_strict.inc's integrate.
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit behind nb_scenes_seen.inc: NOT in the two units whose device
// code kernel_code_sha() hashes.  Launchers: nb_scenes.h.
//
// Why the bits are the chain's.
//   - The row is an order-independent 64-bit minimum of keys depth << 32 | id (nb_raster.inc), so neither the workgroup's shape nor
//     the order the candidates arrive in can change a key.
//   - seen_kernel sorts id << 32 | depth, so a member's seen_depth is the unsigned minimum of the depth bits over its columns (S5).
//   - L1 picks the least column holding exactly those bits.
//   - Both are therefore the two halves of ONE unsigned 64-bit minimum per member m: over the columns c with ids[c] == m, of
//     depth_bits(c) << 32 | c.  A minimum does not depend on the order of arrival either.
//   - The seen list is ascending in id, without duplicates, with no entry >= n (S1-S3); G2 walks it in that order, which is the order
//     the per-body slots 0 .. n-1 are walked in.  With flags = 0 the eye does not draw its own body: no self entry.
//   - L2-L4 and the three quotients of G2 are pure functions of (column, depth bits, the eye's velocity record, up, cp, G, bias): any
//     lane may compute them, the same operations on the same operands give the same bits.  Only the three chains of additions
//     sum = sum + q are ordered, and one lane carries them out in slot order.
//
// Shape: one workgroup per eye b = s n + i (a grid-stride loop over the eyes, eyes_kernel's cap), 64 lanes where
// n <= kScenesSeenWaveBodies and 256 above, as nb_scenes_seen.inc.  Dynamic LDS, sized from (width, n):
//   keys    width x 8 bytes   the row
//   slots   n x 8 bytes       per body of the scene: min over its columns of depth_bits << 32 | column, all ones = not seen; the
//                             step then keeps two quotients in a member's slot (qx low, qy high)
//   plane   n x 4 bytes       the third quotient (step) or the member list (emit)
//   bitmap  256 bytes         kScenesMaxBodies membership bits
// together 8 width + 12 n + 256 bytes: 9.7 KiB at n = 100, width = 1024; 56.25 KiB at n = 2 048, width = 4 096, the largest -- never
// above 64 KiB, so the dynamic limit is not raised.  Per eye:
//   1  clear the keys and the slots to all ones; barrier
//   2  eyes_kernel<false>'s loop body over bodies j = 0 .. n-1 of scene s, j = i skipped, the matrices read at inst + s n; keys carry
//      j.  The text is repeated, as nb_scenes_seen.inc repeats it: nb_eyes.inc keeps its text and eyes_kernel its instructions
//   3  barrier; every column whose key is not all ones takes the LDS minimum (ds_min_u64) of (key >> 32) << 32 | c into slot id
//   4  barrier; lanes take bodies j = t, t + LANES, ...; a __ballot per 64 bodies gives two bitmap words without an atomic.
//      kEmit = false, the step: a lane whose slot is set forms L2-L4 and G2's three quotients and leaves them in the slot and the
//      plane; after a barrier lane 0 walks the set bits ascending, adds the quotients, integrates and writes record b.
//      kEmit = true (SL3): a member's rank is the number of set bits below it; the member list goes into the plane, and after a
//      barrier lanes take slots k = t, t + LANES, ... of the outputs: ids, depth bits, col and rel leave coalesced, padding included
//   5  barrier before the next eye re-initialises LDS

#ifdef __HIPCC__
// L2-L4 for one member, located_kernel's text: column col, depth bits dbits, f and s of the eye
__device__ __forceinline__ float4 scenes_located_rel(const ScenesLocatedArgs &a, float h, uint32_t col, uint32_t dbits, float fx, float fy,
                                                     float fz, float sx, float sy, float sz)
{
    const float xc = (float)col + 0.5f;                                   // L2
    const float xn = (xc - h) / h;
    const float r = a.cp14 / (__uint_as_float(dbits) + a.cp10);
    const float xv = (xn * r) / a.cp0;
    const float p0 = r * fx, p1 = r * fy, p2 = r * fz, q0 = xv * sx, q1 = xv * sy, q2 = xv * sz;
    return make_float4(p0 + q0, p1 + q1, p2 + q2, r);                     // L4
}

template <int LANES, bool kEmit>
__global__ __launch_bounds__(LANES) void scenes_nbody_located_kernel(ScenesLocatedArgs a)
{
    extern __shared__ uint64_t scenes_loc_keys[];                                      // a.width entries
    uint64_t *slots = scenes_loc_keys + a.width;                                       // n entries
    uint32_t *plane = reinterpret_cast<uint32_t *>(slots + a.n);                       // n words
    uint32_t *bitmap = plane + a.n;                                                    // kScenesSeenWords words
    const uint32_t n = a.n, width = a.width;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t words = (n + 31u) >> 5;
    const float h = (float)width * 0.5f;     // exact
    for (uint32_t e = blockIdx.x; e < a.count; e += gridDim.x) {
        const uint32_t b = a.first_eye + e, s = b / n, self = b - s * n;
        const float4 *__restrict__ inst_s = a.inst + (size_t)s * n * 4;
        for (uint32_t c = tid; c < width; c += LANES) scenes_loc_keys[c] = ~0ull;
        for (uint32_t j = tid; j < n; j += LANES) slots[j] = ~0ull;
        __syncthreads();
        float C[16];
        raster_load16(a.cams + (size_t)b * 4, C);
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
                    for (uint32_t c = g.lo; c < own; ++c) eye_cover(scenes_loc_keys, c, g, j);
                    rest = own;
                }
                uint64_t wide = __ballot(has && rest < g.hi);
                while (wide) {
                    const int src = __ffsll((unsigned long long)wide) - 1;
                    wide &= wide - 1;
                    const EyeSeg bg = eye_seg_bcast(g, rest, src);
                    const uint32_t bj = eye_bcast(j, src);
                    for (uint32_t c = bg.lo + lane; c < bg.hi; c += 64u) eye_cover(scenes_loc_keys, c, bg, bj);
                }
            }
        }
        __syncthreads();
        for (uint32_t c = tid; c < width; c += LANES) {
            const uint64_t key = scenes_loc_keys[c];
            const uint32_t id = (uint32_t)key;
            if (key != ~0ull && id < n)   // (a key's id is a j < n: the test keeps the minimum inside the slots)
                __hip_atomic_fetch_min(slots + id, (key & 0xFFFFFFFF00000000ull) | c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        const float4 d = a.vel_in[b];
        float fx = d.x, fy = d.y, fz = d.z;
        loc_normalize3(fx, fy, fz);                                                   // L3: f = dir.normalize()
        const float a0 = fy * a.uz, a1 = fz * a.uy, b0 = fz * a.ux, b1 = fx * a.uz, c0 = fx * a.uy, c1 = fy * a.ux;
        float sx = a0 - a1, sy = b0 - b1, sz = c0 - c1;                               // s = f.cross(up)
        loc_normalize3(sx, sy, sz);
        for (uint32_t j0 = 0; j0 < n; j0 += LANES) {   // every lane runs every pass: the ballot is the wave's
            const uint32_t j = j0 + tid;
            const uint64_t slot = j < n ? slots[j] : ~0ull;
            const bool member = slot != ~0ull;
            if constexpr (!kEmit) {
                if (member) {
                    const float4 vec = scenes_located_rel(a, h, (uint32_t)slot, (uint32_t)(slot >> 32), fx, fy, fz, sx, sy, sz);
                    // nbody_located_kernel's pair code, repeated (nb_located.inc keeps its text, and its kernel its instructions)
                    const float xx = vec.x * vec.x, yy = vec.y * vec.y, zz = vec.z * vec.z;
                    const float dist = ((xx + yy) + zz) + a.bias;                     // main.rs:429
                    const float nx = vec.x * a.G, ny = vec.y * a.G, nz = vec.z * a.G;
                    const float qx = nx / dist, qy = ny / dist, qz = nz / dist;       // main.rs:430
                    slots[j] = (uint64_t)__float_as_uint(qy) << 32 | __float_as_uint(qx);   // the slot is spent: this lane alone read it
                    plane[j] = __float_as_uint(qz);
                }
            }
            const uint64_t m = __ballot(member);
            if (lane == 0u) {   // bodies j0 + 64 wave .. + 63: two words, inside the bitmap (j0 + LANES <= kScenesMaxBodies)
                const uint32_t w = (j0 + tid) >> 5;
                bitmap[w] = (uint32_t)m;
                bitmap[w + 1u] = (uint32_t)(m >> 32);
            }
        }
        __syncthreads();
        if constexpr (!kEmit) {
            if (tid == 0) {
                float4 p = a.pos_in[b], v = d;
                float ax = 0.f, ay = 0.f, az = 0.f;                                   // main.rs:425
                for (uint32_t w = 0; w < words; ++w) {
                    uint32_t m = bitmap[w];
                    while (m) {
                        const uint32_t i = (w << 5) + (uint32_t)(__ffs((int)m) - 1);
                        m &= m - 1u;
                        const uint64_t q = slots[i];
                        ax = ax + __uint_as_float((uint32_t)q);                       // main.rs:430, in slot order
                        ay = ay + __uint_as_float((uint32_t)(q >> 32));
                        az = az + __uint_as_float(plane[i]);
                    }
                }
                integrate(p, v, ax, ay, az, a.dt);                                    // main.rs:434, 436
                a.pos_out[b] = p;
                a.vel_out[b] = v;
            }
        } else {
            uint32_t total = 0;
            for (uint32_t w = 0; w < words; ++w) total += (uint32_t)__popc(bitmap[w]);
            for (uint32_t i = tid; i < n; i += LANES) {
                const uint32_t w = i >> 5, bit = i & 31u, m = bitmap[w];
                if (!(m >> bit & 1u)) continue;
                uint32_t rank = (uint32_t)__popc(m & ((1u << bit) - 1u));
                for (uint32_t v = 0; v < w; ++v) rank += (uint32_t)__popc(bitmap[v]);
                plane[rank] = i;                                                      // rank < total <= n
            }
            __syncthreads();
            if (a.seen_count && tid == 0) a.seen_count[e] = total;
            for (uint32_t k = tid; k < width; k += LANES) {                           // total <= width: a column holds one id
                uint32_t id = kSeenNone, dbits = 0x3F800000u, col = kSeenNone;        // S3, S5's 1.0f, L5
                float4 rel = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k < total) {
                    id = plane[k];
                    const uint64_t slot = slots[id];
                    dbits = (uint32_t)(slot >> 32), col = (uint32_t)slot;
                    rel = scenes_located_rel(a, h, col, dbits, fx, fy, fz, sx, sy, sz);
                }
                const size_t o = (size_t)e * width + k;
                if (a.seen_ids) a.seen_ids[o] = id;
                if (a.seen_depth) a.seen_depth[o] = dbits;
                if (a.seen_col) a.seen_col[o] = col;
                if (a.seen_rel) a.seen_rel[o] = rel;
            }
        }
        __syncthreads();   // the next eye re-initialises the keys and the slots
    }
}

// Dynamic LDS: 8 width + 12 n + 256 bytes (keys, slots, plane, bitmap): 57 600 bytes at the limits, below the 64 KiB default
template <bool kEmit>
static hipError_t launch_scenes_located_form(const ScenesLocatedArgs &a, hipStream_t s)
{
    static_assert((size_t)4096 * 8u + (size_t)kScenesMaxBodies * 12u + kScenesSeenWords * 4u <= 65536u, "the dynamic limit is the default");
    const size_t lds = (size_t)a.width * sizeof(uint64_t) + (size_t)a.n * (sizeof(uint64_t) + sizeof(uint32_t)) + kScenesSeenWords * sizeof(uint32_t);
    const uint32_t grid = a.count < kEyeMaxGrid ? a.count : kEyeMaxGrid;
    if (a.n <= kScenesSeenWaveBodies)
        hipLaunchKernelGGL((scenes_nbody_located_kernel<64, kEmit>), dim3(grid), dim3(64), lds, s, a);
    else
        hipLaunchKernelGGL((scenes_nbody_located_kernel<256, kEmit>), dim3(grid), dim3(256), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_scenes_nbody_located(const ScenesLocatedArgs &a, hipStream_t s) { return launch_scenes_located_form<false>(a, s); }

hipError_t launch_scenes_located(const ScenesLocatedArgs &a, hipStream_t s) { return launch_scenes_located_form<true>(a, s); }
#endif   // __HIPCC__
