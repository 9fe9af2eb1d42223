// nb_scenes_located.inc -- gravity from located vision for scene batches (DESIGN.md section 14.2): every body of every scene folds
// the reference's gravity law over WHERE its own eye sees the bodies of its own scene, in ONE kernel per step for the whole batch.
// The eye's row is resolved in LDS as eyes_kernel resolves it and reduced there to one 64-bit word per body of the scene -- the
// member's nearest depth and the least column holding it --; the located points and the quotients are formed from those words and the
// fold walks the members in ascending order: no row, no list and no located point reaches device memory.  Every scene gets the bits
// nb_step_nbody_located gives a context of its n bodies (SL1): the row is nb_eyes.inc's eye_row_fill, L2-L4 and G2 are
// nb_located.inc's located_basis, located_rel and located_quotients, each the one copy the single-scene chain runs, with
// nb_nbody_strict.inc's integrate; the bitmap helpers and the launch shape are nb_scenes_seen.inc's.
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
//   1  clear the slots to all ones
//   2  scenes_eye_begin (nb_scenes_seen.inc, the one copy the three per-eye scenes kernels share): the keys cleared, a barrier, the
//      row of eye b over the bodies of scene s, a barrier; keys carry j
//   3  every column whose key is not all ones takes the LDS minimum (ds_min_u64) of (key >> 32) << 32 | c into slot id
//   4  barrier; lanes take bodies j = t, t + LANES, ...; a __ballot per 64 bodies gives two bitmap words without an atomic.
//      kEmit = false, the step: a lane whose slot is set forms L2-L4 and G2's three quotients and leaves them in the slot and the
//      plane; after a barrier lane 0 walks the set bits ascending, adds the quotients, integrates and writes record b.
//      kEmit = true (SL3): a member's rank is the number of set bits below it; the member list goes into the plane, and after a
//      barrier lanes take slots k = t, t + LANES, ... of the outputs: ids, depth bits, col and rel leave coalesced, padding included
//   5  barrier before the next eye re-initialises LDS

#ifdef __HIPCC__
template <int LANES, bool kEmit>
__global__ __launch_bounds__(LANES) void scenes_nbody_located_kernel(ScenesLocatedArgs a)
{
    extern __shared__ uint64_t scenes_loc_keys[];                                      // width entries
    const uint32_t n = a.eye.n, width = a.eye.width;
    uint64_t *slots = scenes_loc_keys + width;                                         // n entries
    uint32_t *plane = reinterpret_cast<uint32_t *>(slots + n);                         // n words
    uint32_t *bitmap = plane + n;                                                      // kScenesSeenWords words
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t words = (n + 31u) >> 5;
    const float h = (float)width * 0.5f;     // exact
    for (uint32_t e = blockIdx.x; e < a.eye.count; e += gridDim.x) {
        for (uint32_t j = tid; j < n; j += LANES) slots[j] = ~0ull;
        uint32_t b, s, self;
        scenes_eye_begin<LANES>(a.eye, scenes_loc_keys, e, b, s, self);
        for (uint32_t c = tid; c < width; c += LANES) {
            const uint64_t key = scenes_loc_keys[c];
            const uint32_t id = (uint32_t)key;
            if (key != ~0ull && id < n)   // (a key's id is a j < n: the test keeps the minimum inside the slots)
                __hip_atomic_fetch_min(slots + id, (key & 0xFFFFFFFF00000000ull) | c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        const float4 d = a.vel_in[b];
        float fx, fy, fz, sx, sy, sz;
        located_basis(a, d, fx, fy, fz, sx, sy, sz);
        for (uint32_t j0 = 0; j0 < n; j0 += LANES) {   // every lane runs every pass: the ballot is the wave's
            const uint32_t j = j0 + tid;
            const uint64_t slot = j < n ? slots[j] : ~0ull;
            const bool member = slot != ~0ull;
            if constexpr (!kEmit) {
                if (member) {
                    float qx, qy, qz;
                    located_quotients(a, located_rel(a, h, (uint32_t)slot, (uint32_t)(slot >> 32), fx, fy, fz, sx, sy, sz), qx, qy, qz);
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
                for_each_member(bitmap, words, [&](uint32_t i) {
                    const uint64_t q = slots[i];
                    ax = ax + __uint_as_float((uint32_t)q);                           // main.rs:430, in slot order
                    ay = ay + __uint_as_float((uint32_t)(q >> 32));
                    az = az + __uint_as_float(plane[i]);
                });
                integrate(p, v, ax, ay, az, a.dt);                                    // main.rs:434, 436
                a.pos_out[b] = p;
                a.vel_out[b] = v;
            }
        } else {
            const uint32_t total = members_stage<LANES>(bitmap, n, words, plane);     // total <= n
            __syncthreads();
            if (a.seen_count && tid == 0) a.seen_count[e] = total;
            for (uint32_t k = tid; k < width; k += LANES) {                           // total <= width: a column holds one id
                uint32_t id = kSeenNone, dbits = 0x3F800000u, col = kSeenNone;        // S3, S5's 1.0f, L5
                float4 rel = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k < total) {
                    id = plane[k];
                    const uint64_t slot = slots[id];
                    dbits = (uint32_t)(slot >> 32), col = (uint32_t)slot;
                    rel = located_rel(a, h, col, dbits, fx, fy, fz, sx, sy, sz);
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
    const size_t lds = (size_t)a.eye.width * sizeof(uint64_t) + (size_t)a.eye.n * (sizeof(uint64_t) + sizeof(uint32_t)) + kScenesSeenWords * sizeof(uint32_t);
    return launch_scenes_eyes(scenes_nbody_located_kernel<64, kEmit>, scenes_nbody_located_kernel<256, kEmit>, a.eye.n, a.eye.count, lds, s, a);
}

hipError_t launch_scenes_nbody_located(const ScenesLocatedArgs &a, hipStream_t s) { return launch_scenes_located_form<false>(a, s); }

hipError_t launch_scenes_located(const ScenesLocatedArgs &a, hipStream_t s) { return launch_scenes_located_form<true>(a, s); }
#endif   // __HIPCC__
