// nb_scenes_policy.inc -- a neural policy over each body's eye row for scene batches (DESIGN.md section 14.4): every body of every
// scene pools the depths of its own eye's row into F features, runs them through a two-layer network of H hidden units -- one shared
// network or one per scene -- and is pushed along its eye's own forward and side axes by the two outputs, in ONE kernel per step for
// the whole batch.  The eye's row is resolved in LDS as eyes_kernel resolves it and reduced there to F words; no row, no feature and
// no hidden value reaches device memory.  The row is nb_eyes.inc's eye_row_fill, the axes nb_located.inc's located_basis and the
// epilogue nb_nbody_strict.inc's integrate, each the one copy the other steps run; the launch shape is nb_scenes_seen.inc's.
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit behind nb_scenes_located.inc: NOT in the two units whose device
// code kernel_code_sha() hashes.  Launchers: nb_scenes.h.
//
// The rule (include/nenbody.h P1-P8; tests/policy_restatement.py states it again in numpy), every step one binary32 operation in the
// order written, no contraction:
//   P2  bin f covers columns [f W/F, (f + 1) W/F); d_f = the value whose bits are the unsigned minimum of the depth bits over the bin's
//       non-empty columns, 1.0f where it has none; x_f = 1.0f - d_f
//   P3  t_j = b1[j]; f = 0 .. F-1 in order: t_j = t_j + (w1[f H + j] x_f); h_j = t_j > 0 ? t_j : +0
//   P4  o_k = b2[k]; j = 0 .. H-1 in order: o_k = o_k + (w2[k H + j] h_j); o_k = o_k < -L ? -L : (o_k > L ? L : o_k)
//   P5  f, s = located_basis(velocity record, up); one of the six components not finite: a = (+0, +0, +0); else a_c = (o_0 f_c) + (o_1 s_c)
//   P6  integrate(): v = v + a dt; p = v + p
//
// Why the bits do not depend on the shape.  A key is an order-independent 64-bit minimum (nb_raster.inc); a candidate's depth bits lie
// in [0, 0x3F800000), so the unsigned minimum into a bin cleared to 0x3F800000 is P2's d_f whatever order the columns arrive in.  P3's
// chain is one lane's, in the order of f; P4's is one lane's, in the order of j; P5 and P6 are one lane's.
//
// Shape: one workgroup per eye b = s n + i (a grid-stride loop over the eyes, eyes_kernel's cap), 64 lanes where
// n <= kScenesSeenWaveBodies and 256 above.  Dynamic LDS, sized from (width, F, H):
//   keys    width x 8 bytes   the row
//   bins    F x 4 bytes       the minimum of the depth bits of a bin's columns, 0x3F800000 = empty
//   hid     H x 4 bytes       the hidden layer
// together 8 width + 4 F + 4 H bytes: 8.4 KiB at width = 1024, (F, H) = (64, 32); 34 048 bytes at the limits -- the default dynamic
// limit holds.  Per eye:
//   1  clear the bins to 0x3F800000
//   2  scenes_eye_begin (nb_scenes_seen.inc, the one copy the three per-eye scenes kernels share): the keys cleared, a barrier, the
//      row of eye b over the bodies of scene s, a barrier
//   3  every column whose key is not all ones takes the LDS minimum (ds_min_u32) of its depth bits into bin c / (W/F)
//   4  barrier; lane j < H runs P3: the bins are broadcast reads, w1 is feature-major so that the lanes' loads of one f coalesce
//      (kEmit = true, P8: the F words of x leave coalesced here)
//   5  barrier; lanes 0 and 1 run P4.  kEmit = false, the step: lane 0 takes o_1 from lane 1, runs P5-P6 and writes record b.
//      kEmit = true: the two words of o leave
//   6  barrier before the next eye re-initialises LDS
// The weights are read from device memory: the n eyes of a scene share 4 policy_floats bytes (66 312 at the limits), which stay in L2.

#ifdef __HIPCC__
static constexpr uint32_t kPolicyEmptyBits = 0x3F800000u;   // 1.0f: above every candidate's depth bits

// P2, one column: its key into the bin of its column, `per` = W / F columns a bin
__device__ __forceinline__ void policy_pool(uint32_t *bins, uint32_t c, uint32_t per, uint64_t key)
{
    if (key != ~0ull) __hip_atomic_fetch_min(bins + c / per, (uint32_t)(key >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// P2, one bin resolved: x_f
__device__ __forceinline__ float policy_feature(uint32_t dbits) { return 1.0f - __uint_as_float(dbits); }

// P3 for hidden unit j: w1 and b1 of the eye's policy
__device__ __forceinline__ float policy_hidden(const float *__restrict__ w1, const float *__restrict__ b1, const uint32_t *bins,
                                               uint32_t features, uint32_t hidden, uint32_t j)
{
    float t = b1[j];
#pragma unroll 4
    for (uint32_t f = 0; f < features; ++f) {
        const float m = w1[f * hidden + j] * policy_feature(bins[f]);
        t = t + m;
    }
    return t > 0.0f ? t : 0.0f;                                                       // a NaN gives +0
}

// P4 for one output: its row of w2, its b2
__device__ __forceinline__ float policy_output(const float *__restrict__ w2, float b2, const float *hid, uint32_t hidden, float limit)
{
    float o = b2;
#pragma unroll 4
    for (uint32_t j = 0; j < hidden; ++j) {
        const float m = w2[j] * hid[j];
        o = o + m;
    }
    const float lo = -limit;
    return o < lo ? lo : (o > limit ? limit : o);                                     // a NaN passes through
}

__device__ __forceinline__ bool policy_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// P5: the acceleration of velocity record d under outputs (o0, o1)
template <class Args>
__device__ __forceinline__ void policy_accel(const Args &a, const float4 &d, float o0, float o1, float &ax, float &ay, float &az)
{
    float fx, fy, fz, sx, sy, sz;
    located_basis(a, d, fx, fy, fz, sx, sy, sz);
    ax = 0.f, ay = 0.f, az = 0.f;
    if (!(policy_finite(fx) && policy_finite(fy) && policy_finite(fz) && policy_finite(sx) && policy_finite(sy) && policy_finite(sz))) return;
    const float p0 = o0 * fx, p1 = o0 * fy, p2 = o0 * fz, q0 = o1 * sx, q1 = o1 * sy, q2 = o1 * sz;
    ax = p0 + q0, ay = p1 + q1, az = p2 + q2;
}

template <int LANES, bool kEmit>
__global__ __launch_bounds__(LANES) void scenes_policy_kernel(ScenesPolicyArgs a)
{
    static_assert(kPolicyMaxHidden <= (uint32_t)LANES, "one lane per hidden unit");
    extern __shared__ uint64_t scenes_pol_keys[];                                      // width entries
    const uint32_t width = a.eye.width, features = a.features, hidden = a.hidden;
    uint32_t *bins = reinterpret_cast<uint32_t *>(scenes_pol_keys + width);            // features words
    float *hid = reinterpret_cast<float *>(bins + features);                           // hidden words
    const uint32_t per = width / features;                                             // exact: F divides W
    const uint32_t tid = threadIdx.x;
    for (uint32_t e = blockIdx.x; e < a.eye.count; e += gridDim.x) {
        for (uint32_t f = tid; f < features; f += LANES) bins[f] = kPolicyEmptyBits;
        uint32_t b, s, self;
        scenes_eye_begin<LANES>(a.eye, scenes_pol_keys, e, b, s, self);
        for (uint32_t c = tid; c < width; c += LANES) policy_pool(bins, c, per, scenes_pol_keys[c]);   // c / per < F
        __syncthreads();
        const float *__restrict__ w1 = a.weights + (size_t)s * a.stride;               // the eye's policy: w1, b1, w2, b2
        const uint32_t fh = features * hidden;                                         // at most 16 384
        if (tid < hidden) hid[tid] = policy_hidden(w1, w1 + fh, bins, features, hidden, tid);
        if constexpr (kEmit) {
            if (a.feat_out)
                for (uint32_t f = tid; f < features; f += LANES) a.feat_out[(size_t)e * features + f] = __float_as_uint(policy_feature(bins[f]));
        }
        __syncthreads();
        if (tid < 2u) {                                                                // both lanes are of the first wave
            const float *__restrict__ w2 = w1 + fh + hidden;
            const float o = policy_output(w2 + tid * hidden, w2[2u * hidden + tid], hid, hidden, a.limit);
            if constexpr (!kEmit) {
                const float o0 = eye_bcast(o, 0), o1 = eye_bcast(o, 1);
                if (tid == 0) {
                    float4 p = a.pos_in[b], v = a.vel_in[b];
                    float ax, ay, az;
                    policy_accel(a, v, o0, o1, ax, ay, az);
                    integrate(p, v, ax, ay, az, a.dt);                                 // main.rs:434, 436
                    a.pos_out[b] = p;
                    a.vel_out[b] = v;
                }
            } else {
                if (a.act_out) a.act_out[(size_t)e * 2u + tid] = __float_as_uint(o);
            }
        }
        __syncthreads();   // the next eye re-initialises the keys and the bins
    }
}

// Dynamic LDS: 8 width + 4 F + 4 H bytes (keys, bins, hid): 34 048 bytes at the limits, below the 64 KiB default
template <bool kEmit>
static hipError_t launch_scenes_policy_form(const ScenesPolicyArgs &a, hipStream_t s)
{
    static_assert((size_t)4096 * 8u + (size_t)kPolicyMaxFeatures * 4u + (size_t)kPolicyMaxHidden * 4u <= 65536u, "the dynamic limit is the default");
    const size_t lds = (size_t)a.eye.width * sizeof(uint64_t) + ((size_t)a.features + a.hidden) * sizeof(uint32_t);
    return launch_scenes_eyes(scenes_policy_kernel<64, kEmit>, scenes_policy_kernel<256, kEmit>, a.eye.n, a.eye.count, lds, s, a);
}

hipError_t launch_scenes_policy(const ScenesPolicyArgs &a, hipStream_t s) { return launch_scenes_policy_form<false>(a, s); }

hipError_t launch_scenes_policy_observe(const ScenesPolicyArgs &a, hipStream_t s) { return launch_scenes_policy_form<true>(a, s); }
#endif   // __HIPCC__
