// nb_scenes_policy_recurrent.inc -- a recurrent policy with per-body memory for scene batches (DESIGN.md section 14.8): the policy of
// nb_scenes_policy.inc with a memory of H words per body kept in device memory between steps.  The hidden layer reads the pooled
// features AND the body's memory; the memory of the next step is the hidden layer, limited.  ONE kernel per step for the whole
// batch, as the feedforward policy's: the row, the features, the old memory and the hidden layer stay in LDS, and H words per body
// leave.  The pooling, the outputs, the actuation and the epilogue are nb_scenes_policy.inc's device functions, called as they are;
// the prologue and the launch shape are nb_scenes_seen.inc's.
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit behind nb_scenes_policy.inc: NOT in the two units whose device
// code kernel_code_sha() hashes.  Launchers: nb_scenes.h.
//
// The rule (include/nenbody.h R1-R8; tests/policy_recurrent_restatement.py states it again in numpy), every step one binary32
// operation in the order written, no contraction:
//   R3  t_j = b1[j]; f = 0 .. F-1 in order: t_j = t_j + (w1[f H + j] x_f); r = 0 .. H-1 in order: t_j = t_j + (wr[r H + j] m_r);
//       h_j = t_j > 0 ? t_j : +0
//   R4  m'_j = h_j > S ? S : h_j
//   R5  o_k from h as P4; P5-P6
//
// Shape: scenes_policy_kernel's, with a fourth LDS array.  Dynamic LDS, sized from (width, F, H):
//   keys    width x 8 bytes   the row
//   bins    F x 4 bytes       the minimum of the depth bits of a bin's columns
//   hid     H x 4 bytes       the hidden layer
//   mem     H x 4 bytes       the eye's memory as the step found it
// together 8 width + 4 F + 8 H bytes, 34 304 at the limits.  Per eye, beside scenes_policy_kernel's stages:
//   1  beside the bins' clear, lane j < H copies memory word j of body b from device memory into mem; scenes_eye_begin's first barrier
//      orders it.  Every read of the eye's memory is this one, so the memory may be updated in place
//   4  lane j < H continues its chain over mem[r] -- broadcast LDS reads; wr is source-major, so the lanes' loads of one r coalesce --,
//      writes h_j to hid and stores m'_j: the step to the memory output at b H + j, the observe form (kEmit) to its own output at
//      e H + j, where one is passed
// The weights of one policy are 4 policy_recurrent_floats bytes (82 696 at the limits); the n eyes of a scene share them in L2.

#ifdef __HIPCC__
// R3 for hidden unit j: the chain of P3 continued over the memory, the rectifier behind both
__device__ __forceinline__ float policy_recurrent_hidden(const float *__restrict__ w1, const float *__restrict__ wr, const float *__restrict__ b1,
                                                         const uint32_t *bins, const float *mem, uint32_t features, uint32_t hidden, uint32_t j)
{
    float t = b1[j];
#pragma unroll 4
    for (uint32_t f = 0; f < features; ++f) {
        const float m = w1[f * hidden + j] * policy_feature(bins[f]);
        t = t + m;
    }
#pragma unroll 4
    for (uint32_t r = 0; r < hidden; ++r) {
        const float m = wr[r * hidden + j] * mem[r];
        t = t + m;
    }
    return t > 0.0f ? t : 0.0f;                                                       // a NaN gives +0
}

// R4: h is never a NaN
__device__ __forceinline__ float policy_memory(float h, float limit) { return h > limit ? limit : h; }

template <int LANES, bool kEmit>
__global__ __launch_bounds__(LANES) void scenes_policy_recurrent_kernel(ScenesPolicyRecurrentArgs a)
{
    static_assert(kPolicyMaxHidden <= (uint32_t)LANES, "one lane per hidden unit and per memory word");
    extern __shared__ uint64_t scenes_rec_keys[];                                      // width entries
    const uint32_t width = a.p.eye.width, features = a.p.features, hidden = a.p.hidden;
    uint32_t *bins = reinterpret_cast<uint32_t *>(scenes_rec_keys + width);            // features words
    float *hid = reinterpret_cast<float *>(bins + features);                           // hidden words
    float *mem = hid + hidden;                                                         // hidden words
    const uint32_t per = width / features;                                             // exact: F divides W
    const uint32_t tid = threadIdx.x;
    for (uint32_t e = blockIdx.x; e < a.p.eye.count; e += gridDim.x) {
        for (uint32_t f = tid; f < features; f += LANES) bins[f] = kPolicyEmptyBits;
        if (tid < hidden) mem[tid] = a.mem_in[((size_t)a.p.eye.first_eye + e) * hidden + tid];   // body b's, of the WHOLE batch's
        uint32_t b, s, self;
        scenes_eye_begin<LANES>(a.p.eye, scenes_rec_keys, e, b, s, self);
        for (uint32_t c = tid; c < width; c += LANES) policy_pool(bins, c, per, scenes_rec_keys[c]);   // c / per < F
        __syncthreads();
        // H and the lane index behind an empty statement the compiler cannot see through: the offsets of wr, b1 and w2 and the three
        // lane masks below are then formed per eye (a handful of scalar operations) and not held in scalar registers across the row
        // fill, where the kernel has none to spare
        uint32_t hd = hidden, lane = tid;
        asm volatile("" : "+s"(hd), "+v"(lane));
        const float *__restrict__ w1 = a.p.weights + (size_t)s * a.p.stride;           // the eye's policy: w1, wr, b1, w2, b2
        const uint32_t fh = features * hd, hh = hd * hd;                               // at most 16 384 and 4 096
        if (lane < hd) {
            const float h = policy_recurrent_hidden(w1, w1 + fh, w1 + fh + hh, bins, mem, features, hd, lane);
            hid[lane] = h;
            const float m = policy_memory(h, a.mem_limit);
            if constexpr (!kEmit) {
                a.mem_out[(size_t)b * hd + lane] = m;                                  // the eye's own words, read into LDS above
            } else {
                if (a.mem_obs) a.mem_obs[(size_t)e * hd + lane] = __float_as_uint(m);
            }
        }
        if constexpr (kEmit) {
            if (a.p.feat_out)
                for (uint32_t f = tid; f < features; f += LANES) a.p.feat_out[(size_t)e * features + f] = __float_as_uint(policy_feature(bins[f]));
        }
        __syncthreads();
        if (lane < 2u) {                                                               // both lanes are of the first wave
            const float *__restrict__ w2 = w1 + fh + hh + hd;
            const float o = policy_output(w2 + lane * hd, w2[2u * hd + lane], hid, hd, a.p.limit);
            if constexpr (!kEmit) {
                const float o0 = eye_bcast(o, 0), o1 = eye_bcast(o, 1);
                if (lane == 0) {
                    float4 p = a.p.pos_in[b], v = a.p.vel_in[b];
                    float ax, ay, az;
                    policy_accel(a.p, v, o0, o1, ax, ay, az);
                    integrate(p, v, ax, ay, az, a.p.dt);                               // main.rs:434, 436
                    a.p.pos_out[b] = p;
                    a.p.vel_out[b] = v;
                }
            } else {
                if (a.p.act_out) a.p.act_out[(size_t)e * 2u + tid] = __float_as_uint(o);
            }
        }
        __syncthreads();   // the next eye re-initialises the keys, the bins and the memory
    }
}

// Dynamic LDS: 8 width + 4 F + 8 H bytes (keys, bins, hid, mem): 34 304 bytes at the limits, below the 64 KiB default
template <bool kEmit>
static hipError_t launch_scenes_policy_recurrent_form(const ScenesPolicyRecurrentArgs &a, hipStream_t s)
{
    static_assert((size_t)4096 * 8u + (size_t)kPolicyMaxFeatures * 4u + (size_t)kPolicyMaxHidden * 8u == 34304u, "the LDS at the limits");
    static_assert((size_t)4096 * 8u + (size_t)kPolicyMaxFeatures * 4u + (size_t)kPolicyMaxHidden * 8u <= 65536u, "the dynamic limit is the default");
    const size_t lds = (size_t)a.p.eye.width * sizeof(uint64_t) + ((size_t)a.p.features + 2u * (size_t)a.p.hidden) * sizeof(uint32_t);
    return launch_scenes_eyes(scenes_policy_recurrent_kernel<64, kEmit>, scenes_policy_recurrent_kernel<256, kEmit>, a.p.eye.n, a.p.eye.count, lds,
                              s, a);
}

hipError_t launch_scenes_policy_recurrent(const ScenesPolicyRecurrentArgs &a, hipStream_t s) { return launch_scenes_policy_recurrent_form<false>(a, s); }

hipError_t launch_scenes_policy_recurrent_observe(const ScenesPolicyRecurrentArgs &a, hipStream_t s)
{
    return launch_scenes_policy_recurrent_form<true>(a, s);
}
#endif   // __HIPCC__
