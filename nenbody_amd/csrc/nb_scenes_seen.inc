// nb_scenes_seen.inc -- the seen boids step for scene batches (DESIGN.md section 14.1): every body of every scene folds over what its
// own eye sees of its own scene, in ONE kernel per step for the whole batch.  The eye's row is resolved in LDS as eyes_kernel resolves
// it, reduced there to a membership bitmap, and the fold walks the set bits in ascending order: no row and no list reaches device
// memory.  Every scene gets the bits nb_step_boids_seen gives a context of its n bodies (SV1): the row is nb_eyes.inc's eye_row_fill,
// the pair nb_seen.inc's boids_seen_pair and the epilogue nb_boids.inc's boids_finish, each the one copy the single-scene chain runs.
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit behind nb_eyes.inc, nb_seen.inc and nb_scenes.inc: NOT in the
// two units whose device code kernel_code_sha() hashes.  Launchers: nb_scenes.h.  The bitmap helpers below are nb_scenes_located.inc's
// too, the launch shape and the eye prologue (scenes_eye_begin) that file's and nb_scenes_policy.inc's; this file's kernel spells the
// prologue out and takes loose parameters, the form in which it was measured (DESIGN.md section 14.7).
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
//   2  eye_row_fill over bodies j = 0 .. n-1 of scene s, j = i skipped (see_self = 0), the matrices read at inst + s n; keys carry j
//   3  barrier; every column whose id is not NB_EYES_NONE ORs its bit into the bitmap (an LDS atomic)
//   4  barrier; kEmit = false: lane 0 folds body i over the set bits, gathers the 16-byte records of scene s, runs the epilogue and
//      writes record b.  kEmit = true (SV3): a member's slot is the number of set bits below it -- popcounts of the lower words and of
//      the lower bits of its own --; the list is staged in the keys' LDS and leaves coalesced, NB_EYES_NONE behind the count
//   5  barrier before the next eye re-initialises LDS

static constexpr uint32_t kScenesSeenWords = kScenesMaxBodies / 32u;   // the bitmap: one bit per body of a scene, 256 bytes

#ifdef __HIPCC__
// ---- a scene's membership bitmap, one bit per body, `words` = ceil(n / 32) words of it in use -------------------------------------------
__device__ __forceinline__ uint32_t members_total(const uint32_t *bitmap, uint32_t words)
{
    uint32_t total = 0;
    for (uint32_t w = 0; w < words; ++w) total += (uint32_t)__popc(bitmap[w]);
    return total;
}

// f(i) for every member i, ascending: lowest word and lowest bit first
template <class F>
__device__ __forceinline__ void for_each_member(const uint32_t *bitmap, uint32_t words, F f)
{
    for (uint32_t w = 0; w < words; ++w) {
        uint32_t m = bitmap[w];
        while (m) {
            const uint32_t i = (w << 5) + (uint32_t)(__ffs((int)m) - 1);
            m &= m - 1u;
            f(i);
        }
    }
}

// The members ascending into list[0 .. total), all LANES lanes together: a member's rank is the number of set bits below it -- the
// popcounts of the lower words and of the lower bits of its own.  Returns total; a barrier orders the list.
template <int LANES>
__device__ __forceinline__ uint32_t members_stage(const uint32_t *bitmap, uint32_t n, uint32_t words, uint32_t *list)
{
    const uint32_t total = members_total(bitmap, words);
    for (uint32_t i = threadIdx.x; i < n; i += LANES) {
        const uint32_t w = i >> 5, bit = i & 31u, m = bitmap[w];
        if (!(m >> bit & 1u)) continue;
        uint32_t rank = (uint32_t)__popc(m & ((1u << bit) - 1u));
        for (uint32_t v = 0; v < w; ++v) rank += (uint32_t)__popc(bitmap[v]);
        list[rank] = i;                                                            // rank < total
    }
    return total;
}

// The launch of a one-workgroup-per-eye scenes kernel: k64 where a scene has at most kScenesSeenWaveBodies bodies, k256 above
template <class K, class... A>
static hipError_t launch_scenes_eyes(K k64, K k256, uint32_t n, uint32_t count, size_t lds, hipStream_t s, A... args)
{
    const uint32_t grid = count < kEyeMaxGrid ? count : kEyeMaxGrid;
    if (n <= kScenesSeenWaveBodies)
        hipLaunchKernelGGL(k64, dim3(grid), dim3(64), lds, s, args...);
    else
        hipLaunchKernelGGL(k256, dim3(grid), dim3(256), lds, s, args...);
    return hipGetLastError();
}

// The head of every pass of a one-workgroup-per-eye scenes kernel over the eyes of `y`: eye e of the launch is body `self` of scene s,
// record b of the batch; its row is resolved into `keys` (y.width entries of LDS) as eyes_kernel resolves it, the eye's own body not
// drawn.  The kernel has issued the clears of its other LDS; the first barrier here orders them with the keys', the second the row.
// scenes_boids_seen_kernel below holds the same statements itself.
template <int LANES>
__device__ __forceinline__ void scenes_eye_begin(const ScenesEyes &y, uint64_t *keys, uint32_t e, uint32_t &b, uint32_t &s, uint32_t &self)
{
    b = y.first_eye + e, s = b / y.n, self = b - s * y.n;
    for (uint32_t c = threadIdx.x; c < y.width; c += LANES) keys[c] = ~0ull;
    __syncthreads();
    float C[16];
    raster_load16(y.cams + (size_t)b * 4, C);
    eye_row_fill<LANES, EyeCover1>(keys, C, y.inst + (size_t)s * y.n * 4, y.n, self, 0u, (float)y.width * 0.5f /* exact */, y.width);
    __syncthreads();
}

template <int LANES, bool kEmit>
__global__ __launch_bounds__(LANES) void scenes_boids_seen_kernel(BoidsArgs a, uint32_t n, uint32_t first_eye, uint32_t count,
                                                                 const float4 *__restrict__ cams, const float4 *__restrict__ inst,
                                                                 uint32_t width, uint32_t *__restrict__ seen_count,
                                                                 uint32_t *__restrict__ seen_ids)
{
    extern __shared__ uint64_t scenes_seen_keys[];                                     // width entries
    uint32_t *bitmap = reinterpret_cast<uint32_t *>(scenes_seen_keys + width);         // kScenesSeenWords words
    const uint32_t tid = threadIdx.x;
    const uint32_t words = (n + 31u) >> 5;
    const float h = (float)width * 0.5f;     // exact
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const uint32_t b = first_eye + e, s = b / n, self = b - s * n;
        for (uint32_t c = tid; c < width; c += LANES) scenes_seen_keys[c] = ~0ull;
        for (uint32_t w = tid; w < kScenesSeenWords; w += LANES) bitmap[w] = 0u;
        __syncthreads();
        float C[16];
        raster_load16(cams + (size_t)b * 4, C);
        eye_row_fill<LANES, EyeCover1>(scenes_seen_keys, C, inst + (size_t)s * n * 4, n, self, 0u, h, width);
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
                for_each_member(bitmap, words, [&](uint32_t i) {
                    if (i == self || i >= n) return;                                   // main.rs:475 n != i; an entry outside the scene is not read
                    boids_seen_pair(a, acc, pn, vn, pos_s[i], vel_s[i]);
                });
                boids_finish(a, acc, b, pn);                                           // a.first = 0: record b of the batch
            }
        } else {
            uint32_t *list = reinterpret_cast<uint32_t *>(scenes_seen_keys);           // the keys are spent: width slots of the list
            const uint32_t total = members_stage<LANES>(bitmap, n, words, list);       // total <= width: a column holds one id
            __syncthreads();
            if (seen_count && tid == 0) seen_count[e] = total;
            if (seen_ids)
                for (uint32_t k = tid; k < width; k += LANES) seen_ids[(size_t)e * width + k] = k < total ? list[k] : kSeenNone;
        }
        __syncthreads();   // the next eye re-initialises the keys and the bitmap
    }
}

template <bool kEmit>
static hipError_t launch_scenes_seen_form(const ScenesSeenArgs &a, hipStream_t s)
{
    const size_t lds = (size_t)a.eye.width * sizeof(uint64_t) + kScenesSeenWords * sizeof(uint32_t);   // 32 KiB + 256 B at width 4096
    return launch_scenes_eyes(scenes_boids_seen_kernel<64, kEmit>, scenes_boids_seen_kernel<256, kEmit>, a.eye.n, a.eye.count, lds, s, a.c,
                              a.eye.n, a.eye.first_eye, a.eye.count, a.eye.cams, a.eye.inst, a.eye.width, a.seen_count, a.seen_ids);
}

hipError_t launch_scenes_boids_seen(const ScenesSeenArgs &a, hipStream_t s) { return launch_scenes_seen_form<false>(a, s); }

hipError_t launch_scenes_seen(const ScenesSeenArgs &a, hipStream_t s) { return launch_scenes_seen_form<true>(a, s); }
#endif   // __HIPCC__
