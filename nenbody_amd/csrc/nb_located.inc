// nb_located.inc -- where each eye sees what it sees (DESIGN.md section 13): the located seen set of every eye, and the gravity step
// folded over those relative positions alone -- the reference's own law (update_instance_nbody, src/main.rs:404-441) with the difference
// vector p_i - p_n supplied by the eye's row instead of by the positions of the two bodies.
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit behind nb_seen.inc: NOT in the two units whose device code
// kernel_code_sha() hashes.  Launchers: nb_located.h.
//
// Located seen set of eye e from its resolved row ids[0..W), depth[0..W), its seen list (count, seen_ids, seen_depth as seen_kernel
// leaves them: ascending, no duplicates), its direction record Dir, `up` and the eyes' camera constant cp
// (tests/located_restatement.py states it again in numpy); every step one binary32 operation in the order written:
//   L1  seen_col[k], k < count: the least column c with ids[c] == seen_ids[k] and bits(depth[c]) == bits(seen_depth[k]); no such
//       column (the list is not of this row; NB_EYES_NONE is no member): NB_EYES_NONE, and seen_rel[k] = four +0 words
//   L2  h = W 0.5; xc = c + 0.5; xn = (xc - h) / h; r = cp[14] / (d + cp[10]); xv = (xn r) / cp[0]
//   L3  f = normalize(Dir), s = normalize(f x up) as cameras_kernel forms them (nb_aux.inc)
//   L4  seen_rel[k] = (r f0 + xv s0, r f1 + xv s1, r f2 + xv s2, r)
//   L5  the slots k >= count: NB_EYES_NONE and four +0 words
// Shape: one workgroup of 256 lanes per eye (a grid-stride loop over the eyes, seen_kernel's cap).  The list goes into LDS -- ids,
// depth bits and one `col` word of all ones per slot, 12 bytes a slot: 48 KB at W = 4096 with a full list, three workgroups a compute
// unit there and thirteen at W = 1024 --; every lane takes columns c, c + 256, ..., finds its id's slot by binary search (at most 12
// probes of words that differ from lane to lane: no broadcast, conflicts as they fall) and, where the column's depth bits are the
// slot's, takes the unsigned minimum of c into the slot's col (ds_min_u32: the result does not depend on the order of arrival).  After
// the barrier lanes take slots: L2-L4, one 4-byte and one 16-byte store a slot, coalesced, padding included.  Three barriers an eye.
// f and s are recomputed by every lane: the same operations on the same operands, the same bits.
//
// Located gravity step (G2-G3): one lane per body, boids_seen_kernel's shape.  The lane walks the first min(count, stride) records of
// its own row -- 16-byte loads, no gather through an id --, forms dist and the three quotients as pair_strict<IEEE = true> does and adds
// them in slot order: the reference's chain of additions.  The epilogue is integrate(), unchanged.

static constexpr int kLocBlock = 256;

#ifdef __HIPCC__
// normalize3 of nb_aux.inc, which lives in a hashed unit: written again
__device__ __forceinline__ void loc_normalize3(float &x, float &y, float &z)
{
    const float q0 = x * x, q1 = y * y, q2 = z * z;
    const float mag = __builtin_sqrtf((q0 + q1) + q2);
    const float s = 1.0f / mag;
    x = x * s;
    y = y * s;
    z = z * s;
}

// The three below take any argument struct with the fields they read: LocatedArgs, LocatedStepArgs and nb_scenes.h's ScenesLocatedArgs.
// L3: f = normalize(d), s = normalize(f x up)
template <class Args>
__device__ __forceinline__ void located_basis(const Args &a, const float4 &d, float &fx, float &fy, float &fz, float &sx, float &sy, float &sz)
{
    float f0 = d.x, f1 = d.y, f2 = d.z;
    loc_normalize3(f0, f1, f2);                                                       // f = dir.normalize()
    const float a0 = f1 * a.uz, a1 = f2 * a.uy, b0 = f2 * a.ux, b1 = f0 * a.uz, c0 = f0 * a.uy, c1 = f1 * a.ux;
    float s0 = a0 - a1, s1 = b0 - b1, s2 = c0 - c1;                                   // s = f.cross(up)
    loc_normalize3(s0, s1, s2);
    fx = f0, fy = f1, fz = f2, sx = s0, sy = s1, sz = s2;
}

// L2 and L4 for one member: column col, depth bits dbits, f and s of the eye, h = width / 2
template <class Args>
__device__ __forceinline__ float4 located_rel(const Args &a, float h, uint32_t col, uint32_t dbits, float fx, float fy, float fz, float sx,
                                              float sy, float sz)
{
    const float xc = (float)col + 0.5f;                                               // L2
    const float xn = (xc - h) / h;
    const float r = a.cp14 / (__uint_as_float(dbits) + a.cp10);
    const float xv = (xn * r) / a.cp0;
    const float p0 = r * fx, p1 = r * fy, p2 = r * fz, q0 = xv * sx, q1 = xv * sy, q2 = xv * sz;
    return make_float4(p0 + q0, p1 + q1, p2 + q2, r);                                 // L4
}

// G2 for one located point: dist and the three quotients, as pair_strict<IEEE = true> forms them
template <class Args>
__device__ __forceinline__ void located_quotients(const Args &a, const float4 &vec, float &qx, float &qy, float &qz)
{
    const float xx = vec.x * vec.x, yy = vec.y * vec.y, zz = vec.z * vec.z;
    const float dist = ((xx + yy) + zz) + a.bias;                                     // main.rs:429
    const float nx = vec.x * a.G, ny = vec.y * a.G, nz = vec.z * a.G;
    qx = nx / dist, qy = ny / dist, qz = nz / dist;                                   // main.rs:430
}

__global__ __launch_bounds__(kLocBlock) void located_kernel(LocatedArgs a)
{
    extern __shared__ uint32_t loc_lds[];
    uint32_t *l_ids = loc_lds, *l_bits = loc_lds + a.width, *l_col = loc_lds + 2u * a.width;   // a.width slots each
    const uint32_t tid = threadIdx.x;
    const float h = (float)a.width * 0.5f;
    for (uint32_t e = blockIdx.x; e < a.count; e += gridDim.x) {
        const size_t row = (size_t)e * a.width;
        const uint32_t cnt = a.seen_count[e] < a.width ? a.seen_count[e] : a.width;   // a caller's count is clamped: nothing past the row is read
        for (uint32_t k = tid; k < cnt; k += kLocBlock) {
            l_ids[k] = a.seen_ids[row + k];
            l_bits[k] = a.seen_depth[row + k];
            l_col[k] = kSeenNone;
        }
        __syncthreads();
        for (uint32_t c = tid; c < a.width; c += kLocBlock) {                         // L1
            const uint32_t id = a.ids_rows[row + c];
            if (id == kSeenNone) continue;
            uint32_t lo = 0u, hi = cnt;                                               // the first slot whose id is not below `id`
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (l_ids[mid] < id)
                    lo = mid + 1u;
                else
                    hi = mid;
            }
            if (lo < cnt && l_ids[lo] == id && l_bits[lo] == a.depth_rows[row + c]) atomicMin(&l_col[lo], c);
        }
        __syncthreads();
        const float4 d = a.dirs[e];
        float fx, fy, fz, sx, sy, sz;
        located_basis(a, d, fx, fy, fz, sx, sy, sz);
        for (uint32_t k = tid; k < a.width; k += kLocBlock) {
            uint32_t col = kSeenNone;
            float4 rel = make_float4(0.f, 0.f, 0.f, 0.f);                             // L5, and L1's slot without a column
            if (k < cnt) col = l_col[k];
            if (col != kSeenNone) rel = located_rel(a, h, col, l_bits[k], fx, fy, fz, sx, sy, sz);
            if (a.seen_col) a.seen_col[row + k] = col;
            a.seen_rel[row + k] = rel;
        }
        __syncthreads();   // the next eye refills the list
    }
}

__global__ __launch_bounds__(kBlock) void nbody_located_kernel(LocatedStepArgs a, const uint32_t *__restrict__ seen_count,
                                                              const float4 *__restrict__ seen_rel, uint32_t stride)
{
    const uint32_t l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= a.count) return;
    const uint32_t n = a.first + l;
    float4 p = a.pos_in[n], v = a.vel_in[n];
    const float4 *__restrict__ list = seen_rel + (size_t)l * stride;
    const uint32_t len = seen_count[l] < stride ? seen_count[l] : stride;
    float sx = 0.f, sy = 0.f, sz = 0.f;                                               // main.rs:425
    for (uint32_t k = 0; k < len; ++k) {
        float qx, qy, qz;
        located_quotients(a, list[k], qx, qy, qz);                                    // main.rs:428-430, the vector from the row
        sx = sx + qx, sy = sy + qy, sz = sz + qz;                                     // in slot order
    }
    integrate(p, v, sx, sy, sz, a.dt);                                                // main.rs:434, 436
    a.pos_out[n] = p;
    a.vel_out[n] = v;
}

hipError_t launch_located(const LocatedArgs &a, hipStream_t s)
{
    const size_t lds = (size_t)a.width * 3u * sizeof(uint32_t);                       // 48 KB at width 4096
    const uint32_t grid = a.count < kSeenMaxGrid ? a.count : kSeenMaxGrid;
    hipLaunchKernelGGL(located_kernel, dim3(grid), dim3(kLocBlock), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_nbody_located(const LocatedStepArgs &a, const uint32_t *seen_count, const float4 *seen_rel, uint32_t stride, hipStream_t s)
{
    hipLaunchKernelGGL(nbody_located_kernel, dim3(ceil_div_u(a.count, kBlock)), dim3(kBlock), 0, s, a, seen_count, seen_rel, stride);
    return hipGetLastError();
}
#endif   // __HIPCC__
