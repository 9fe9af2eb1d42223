// nb_seen.inc -- what a controller makes of the eye rows (DESIGN.md section 12): the seen set of every eye, and the boids step folded
// over what each body sees instead of over every body by index (the reference's own caveat at its flocking demo: "this controller
// has access to the location of each entity, and is not using the visual data").
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit behind nb_raster.inc and nb_eyes.inc: NOT in the two units
// whose device code kernel_code_sha() hashes.  Launchers: nb_seen.h.
//
// Seen set of eye e from its resolved row ids[0..W), depth[0..W) (tests/seen_restatement.py states it again through np.unique):
//   S1  S(e) = the values other than NB_EYES_NONE in ids, compared as unsigned 32-bit numbers
//   S2  seen_count[e] = |S(e)|
//   S3  seen_ids[e W + k], k < count: the members ascending; the other slots NB_EYES_NONE
//   S4  seen_cols[e W + k]: the number of columns holding that member; the other slots 0
//   S5  seen_depth[e W + k]: the value whose bits are the unsigned minimum of the bits of depth[c] over those columns; the others 1.0f
// Shape: one workgroup of 256 lanes per eye (a grid-stride loop over the eyes).  The row goes into LDS as keys id << 32 | bits(depth),
// padded with all-ones keys to the next power of two P, and is sorted there by a bitonic network (P <= 4096: 32 KB): equal ids are
// then neighbours with their least depth first, empty columns (id = NB_EYES_NONE) and the padding last.  A position is a HEAD where
// its id is not NB_EYES_NONE and differs from its predecessor's; a workgroup prefix sum over the head flags gives each head its slot k,
// the head's low half is S5's minimum and the distance to the next head (or to the first empty column) S4's count.  The three list rows
// leave coalesced, padding included.  Nothing depends on the order anything arrives in: the result is a function of the row.
//
// Seen boids step (V2-V3): boids_pair's select form -- the reference's operations, operand order and predicates, valid for any
// record -- over the entries of the body's list in list order; an entry equal to the body or >= n_total is skipped unread.  One lane
// per body: its nine sums form the reference's chains of additions, its loads are gathers of 16-byte records.  The epilogue is
// boids_finish, unchanged.

static constexpr int kSeenBlock = 256;
static constexpr uint32_t kSeenMaxGrid = 2048;   // 256 compute units x 8 workgroups of four waves
static constexpr uint32_t kSeenNone = 0xFFFFFFFFu;

#ifdef __HIPCC__
__global__ __launch_bounds__(kSeenBlock) void seen_kernel(uint32_t count, uint32_t width, uint32_t pow2, const uint32_t *__restrict__ ids_rows,
                                                         const uint32_t *__restrict__ depth_rows, uint32_t *__restrict__ seen_count,
                                                         uint32_t *__restrict__ seen_ids, uint32_t *__restrict__ seen_depth,
                                                         uint32_t *__restrict__ seen_cols)
{
    extern __shared__ uint64_t seen_keys[];                                   // pow2 keys
    uint32_t *heads = reinterpret_cast<uint32_t *>(seen_keys + pow2);         // pow2 + 1 positions: head k, then the end of the last run
    uint32_t *misc = heads + pow2 + 1;                                        // [0..3] the waves' head counts, [4] the first empty position
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // the positions a lane flags and ranks: a contiguous share, so that one prefix sum over the lanes orders every head
    const uint32_t per = pow2 > (uint32_t)kSeenBlock ? pow2 / kSeenBlock : 1u;
    const uint32_t lo = tid * per < pow2 ? tid * per : pow2, hi = lo + per < pow2 ? lo + per : pow2;
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const size_t row = (size_t)e * width;
        for (uint32_t c = tid; c < pow2; c += kSeenBlock) {
            uint64_t key = ~0ull;
            if (c < width) key = ((uint64_t)ids_rows[row + c] << 32) | (depth_rows ? depth_rows[row + c] : 0u);
            seen_keys[c] = key;
        }
        if (tid == 0) misc[4] = 0u;
        __syncthreads();
        for (uint32_t k = 2; k <= pow2; k <<= 1)
            for (uint32_t j = k >> 1; j; j >>= 1) {
                for (uint32_t i = tid; i < pow2 / 2u; i += kSeenBlock) {
                    const uint32_t a = ((i & ~(j - 1u)) << 1) | (i & (j - 1u)), b = a | j;   // a < b < pow2
                    const uint64_t x = seen_keys[a], y = seen_keys[b];
                    if ((x > y) == ((a & k) == 0u)) seen_keys[a] = y, seen_keys[b] = x;
                }
                __syncthreads();
            }
        uint32_t mine = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            const uint32_t id = (uint32_t)(seen_keys[i] >> 32);
            if (id == kSeenNone) continue;
            if (i == 0u || (uint32_t)(seen_keys[i - 1u] >> 32) != id) ++mine;
            if (i + 1u == pow2 || (uint32_t)(seen_keys[i + 1u] >> 32) == kSeenNone) misc[4] = i + 1u;   // one position at most
        }
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t v = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += v;
        }
        if (lane == 63u) misc[wave] = incl;
        __syncthreads();
        uint32_t slot = incl - mine;
        for (uint32_t w = 0; w < wave; ++w) slot += misc[w];
        const uint32_t total = misc[0] + misc[1] + misc[2] + misc[3];                          // <= width
        for (uint32_t i = lo; i < hi; ++i) {
            const uint32_t id = (uint32_t)(seen_keys[i] >> 32);
            if (id != kSeenNone && (i == 0u || (uint32_t)(seen_keys[i - 1u] >> 32) != id)) heads[slot++] = i;
        }
        if (tid == 0) {
            heads[total] = misc[4];
            seen_count[e] = total;
        }
        __syncthreads();
        for (uint32_t k = tid; k < width; k += kSeenBlock) {
            uint32_t id = kSeenNone, dbits = 0x3F800000u, cols = 0u;
            if (k < total) {
                const uint32_t h = heads[k];
                const uint64_t key = seen_keys[h];
                id = (uint32_t)(key >> 32), dbits = (uint32_t)key, cols = heads[k + 1u] - h;
            }
            seen_ids[row + k] = id;
            if (seen_depth) seen_depth[row + k] = dbits;
            if (seen_cols) seen_cols[row + k] = cols;
        }
        __syncthreads();   // the next eye refills the keys
    }
}

// Rules 1-3 of body (pn, vn) on one neighbour (pj, vj): V2's pair, for boids_seen_kernel and scenes_boids_seen_kernel (nb_scenes_seen.inc)
__device__ __forceinline__ void boids_seen_pair(const BoidsArgs &a, BoidsAcc &s, const float4 &pn, const float4 &vn, const float4 &pj,
                                                const float4 &vj)
{
    const float dx = pj.x - pn.x, dy = pj.y - pn.y, dz = pj.z - pn.z;         // distance2: (other - self)
    const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
    const float ex = vj.x - vn.x, ey = vj.y - vn.y, ez = vj.z - vn.z;
    const float e2 = ((ex * ex) + (ey * ey)) + (ez * ez);
    if (d2 < a.r1) {                                                          // main.rs:474-476
        s.cx = s.cx + pj.x, s.cy = s.cy + pj.y, s.cz = s.cz + pj.z;
        s.cnt = s.cnt + 1.f;
    }
    if (d2 <= a.t2) s.rx = s.rx - dx, s.ry = s.ry - dy, s.rz = s.rz - dz;     // main.rs:485-487  sqrt(d2) < rule_2_distance
    if (e2 <= a.t3) {                                                         // main.rs:497-499  sqrt(e2) < rule_3_distance
        s.mx = s.mx + vj.x, s.my = s.my + vj.y, s.mz = s.mz + vj.z;
        s.vcnt = s.vcnt + 1.f;
    }
}

__global__ __launch_bounds__(kBlock) void boids_seen_kernel(BoidsArgs a, const uint32_t *__restrict__ seen_count,
                                                           const uint32_t *__restrict__ seen_ids, uint32_t stride)
{
    const uint32_t l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= a.count) return;
    const uint32_t n = a.first + l;
    const float4 pn = a.pos_in[n], vn = a.vel_in[n];
    const uint32_t *__restrict__ list = seen_ids + (size_t)l * stride;
    const uint32_t len = seen_count[l] < stride ? seen_count[l] : stride;
    BoidsAcc s{};                                                             // main.rs:472, 483, 495
    for (uint32_t k = 0; k < len; ++k) {
        const uint32_t i = list[k];
        if (i == n || i >= a.n_total) continue;                               // main.rs:475 n != i; an entry outside the set is not read
        boids_seen_pair(a, s, pn, vn, a.pos_in[i], a.vel_in[i]);
    }
    boids_finish(a, s, l, pn);
}

hipError_t launch_seen(uint32_t count, uint32_t width, const uint32_t *ids_rows, const float *depth_rows, uint32_t *seen_count,
                       uint32_t *seen_ids, float *seen_depth, uint32_t *seen_cols, hipStream_t s)
{
    uint32_t pow2 = 1;
    while (pow2 < width) pow2 <<= 1;
    const size_t lds = (size_t)pow2 * sizeof(uint64_t) + ((size_t)pow2 + 1u + 5u) * sizeof(uint32_t);   // 48 KB + 24 B at width 4096
    const uint32_t grid = count < kSeenMaxGrid ? count : kSeenMaxGrid;
    hipLaunchKernelGGL(seen_kernel, dim3(grid), dim3(kSeenBlock), lds, s, count, width, pow2, ids_rows, (const uint32_t *)depth_rows,
                       seen_count, seen_ids, (uint32_t *)seen_depth, seen_cols);
    return hipGetLastError();
}

hipError_t launch_boids_seen(const BoidsArgs &a, const uint32_t *seen_count, const uint32_t *seen_ids, uint32_t stride, hipStream_t s)
{
    hipLaunchKernelGGL(boids_seen_kernel, dim3(ceil_div_u(a.count, kBlock)), dim3(kBlock), 0, s, a, seen_count, seen_ids, stride);
    return hipGetLastError();
}
#endif   // __HIPCC__
