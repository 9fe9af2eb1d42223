// nb_scenes_es.inc -- one evolution-strategies generation over a scene batch (DESIGN.md section 14.6): the population drawn from a
// mean by a counter-based generator, the scenes' score records ranked, the mean updated.  Three kernels, every one asynchronous on
// the caller's stream; a search loop needs no transfer and no wait until the host wants the result.
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit behind nb_scenes_score.inc: NOT in the two units whose device
// code kernel_code_sha() hashes.  Launchers: nb_scenes.h.
//
// The rule (include/nenbody.h E1-E8; tests/es_restatement.py states it again in numpy), every float operation one binary32
// operation in the order written, no contraction, every sum of draws an exact integer:
//   E1  Philox4x32-10, counter (m >> 1, s >> 1, g, 0), key (seed low, seed high)
//   E2  k = the centred sum of the four 16-bit halves of (x0, x1) for even m, of (x2, x3) for odd m; scene 2q + 1 takes -k;
//       e = (float)k * C
//   E3  theta[s M + m] = mean[m] + (sigma * e)
//   E4  phi = +0, then phi = phi + (coef[i] * field_i) over the six fields, a zero coefficient skipped
//   E5  key64 = key32(phi) << 32 | s; r_s = the number of scenes with a smaller key
//   E6  u_s = 2 r_s - (B - 1)
//   E7  A_m = sum_s u_s k(s, m), exact; mean'[m] = mean[m] + (step * ((float)A_m * C))
//   E8  no word depends on B (theta), the grid, the workgroup shape or the split over launches
//
// es_philox, es_draw and the three float epilogues (es_theta, es_fitness, es_mean) are written once.  One Philox call serves a
// (scene pair, weight pair): words x0, x1 give k(2q, 2p), words x2, x3 give k(2q, 2p + 1), and scene 2q + 1 takes their negatives.
// The perturb kernel therefore writes four words of theta per call, and the update kernel folds a scene pair as (u_2q - u_2q+1) k.
//
// Why the rank counts.  E5 DEFINES r_s as a count, B is at most 4 096, and the keys are distinct, so a lane that owns scene s walks
// the B keys in LDS and counts the smaller ones: every lane of a wave reads the same key, which LDS broadcasts, there is no padding to
// a power of two, no barrier per stage and no scatter of ranks behind a sort.  The bitonic network of nb_seen.inc needs
// log2(P) (log2(P) + 1) / 2 barriers -- 78 at P = 4 096 -- and a second pass that turns places into ranks per scene.  At 512
// scenes and below the spare lanes of the workgroup split the walk into slices whose counts meet in an LDS add, so a population of 256 walks 64
// keys a lane.  Section 14.6 has the measured times at B = 256 and at the limit.

#ifdef __HIPCC__
constexpr uint32_t kEsKMax = 131070u;        // 2 (2^16 - 1): the centre of a sum of four 16-bit words
constexpr uint32_t kEsCBits = 0x37DDB3D7u;   // C = sqrt(3) 2^-16, one over the draw's standard deviation
constexpr uint32_t kEsRankLanes = 1024;
constexpr uint32_t kEsUpdateLanes = 256;     // four waves, a weight pair each
constexpr uint32_t kEsPerturbLanes = 256;

struct EsWords {
    uint32_t x0, x1, x2, x3;
};

// E1: Philox4x32-10 as published (Salmon et al., SC 2011)
__device__ __forceinline__ EsWords es_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0, c1 = l1, c2 = h0 ^ c3 ^ k1, c3 = l0;
    }
    return EsWords{c0, c1, c2, c3};
}

// E2's integer for an even scene: the centred sum of the four halves of (a, b)
__device__ __forceinline__ int32_t es_draw(uint32_t a, uint32_t b)
{
    return (int32_t)((a & 0xFFFFu) + (a >> 16) + (b & 0xFFFFu) + (b >> 16)) - (int32_t)kEsKMax;
}

// k(2q, 2p) and k(2q, 2p + 1) of generation g
__device__ __forceinline__ void es_draw_pair(uint64_t seed, uint32_t g, uint32_t q, uint32_t p, int32_t *k_even, int32_t *k_odd)
{
    const EsWords x = es_philox(p, q, g, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    *k_even = es_draw(x.x0, x.x1);
    *k_odd = es_draw(x.x2, x.x3);
}

// E3
__device__ __forceinline__ float es_theta(float mean, float sigma, int32_t k)
{
    const float e = (float)k * __uint_as_float(kEsCBits);   // (float)k is exact: |k| < 2^24
    const float se = sigma * e;
    return mean + se;
}

// E4
__device__ __forceinline__ float es_fitness(const SceneScore &r, const EsArgs &a)
{
    const float field[6] = {(float)r.near, r.spread, r.speed2, r.momentum2, r.goal2, (float)r.nonfinite};   // u64 -> f32 rounds once
    const float coef[6] = {a.c0, a.c1, a.c2, a.c3, a.c4, a.c5};
    float phi = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float term = coef[i] * field[i];
        if (coef[i] != 0.f) phi = phi + term;
    }
    return phi;
}

// E5's key32
__device__ __forceinline__ uint32_t es_key32(float phi)
{
    const uint32_t w = __float_as_uint(phi);
    if (phi != phi) return 0u;
    return (w & 0x80000000u) ? ~w : (w | 0x80000000u);
}

// E7's three float operations
__device__ __forceinline__ float es_mean(float mean, float step, long long A)
{
    const float d = (float)A * __uint_as_float(kEsCBits);   // i64 -> f32 rounds once
    const float sd = step * d;
    return mean + sd;
}

// One lane per (scene pair, weight pair) of scenes [first, first + count): pairs q0 .. q1 by weight pairs 0 .. mp - 1, the weight
// pair fastest, so a wave's stores run along m.
__global__ __launch_bounds__(kEsPerturbLanes) void es_perturb_kernel(EsArgs a, uint32_t first, uint32_t count, const float *__restrict__ mean,
                                                                     float *__restrict__ theta)
{
    const uint32_t mp = (a.m + 1u) >> 1, q0 = first >> 1;
    const uint32_t pairs = ((first + count - 1u) >> 1) - q0 + 1u;
    const uint32_t i = blockIdx.x * kEsPerturbLanes + threadIdx.x;   // below 2^25: pairs <= 2 048, mp <= 8 289
    if (i >= pairs * mp) return;
    const uint32_t q = q0 + i / mp, p = i % mp;
    int32_t k0, k1;
    es_draw_pair(a.seed, a.g, q, p, &k0, &k1);
    const uint32_t m = 2u * p;
    const bool odd_m = m + 1u < a.m;                                 // an odd last weight has no partner
    const float mu0 = mean[m], mu1 = odd_m ? mean[m + 1u] : 0.f;
    const uint32_t s0 = 2u * q, s1 = s0 + 1u;
    if (s0 >= first && s0 < first + count) {                         // a range may begin at an odd scene and end at an even one
        float *row = theta + (size_t)(s0 - first) * a.m;
        row[m] = es_theta(mu0, a.sigma, k0);
        if (odd_m) row[m + 1u] = es_theta(mu1, a.sigma, k1);
    }
    if (s1 >= first && s1 < first + count) {
        float *row = theta + (size_t)(s1 - first) * a.m;
        row[m] = es_theta(mu0, a.sigma, -k0);
        if (odd_m) row[m + 1u] = es_theta(mu1, a.sigma, -k1);
    }
}

// ONE workgroup of kEsRankLanes lanes.  Dynamic LDS: B keys of 64 bits, B counts, the NaN count: 12 B + 16 bytes, 49 168 at B = 4 096.
__global__ __launch_bounds__(kEsRankLanes) void es_rank_kernel(EsArgs a, const SceneScore *__restrict__ score, uint32_t *__restrict__ rank,
                                                               float *__restrict__ fitness, uint32_t *__restrict__ report)
{
    extern __shared__ unsigned long long es_lds[];                 // [B] key64
    const uint32_t t = threadIdx.x, B = a.scenes;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(es_lds + B);      // [B] the smaller keys, then the NaN count
    uint32_t nans = 0u;
    for (uint32_t s = t; s < B; s += kEsRankLanes) {
        const float phi = es_fitness(score[s], a);
        if (fitness) fitness[s] = phi;
        nans += (phi != phi) ? 1u : 0u;
        es_lds[s] = (unsigned long long)es_key32(phi) << 32 | s;
        cnt[s] = 0u;
    }
    if (t == 0u) cnt[B] = 0u;
    __syncthreads();
    nans = score_wave_sum(nans);
    if ((t & 63u) == 0u && nans) atomicAdd(cnt + B, nans);
    // P: the smallest power of two >= B.  P >= 1 024: lane t owns scenes t, t + 1 024, .. and walks every key.  P < 1 024: 1 024 / P
    // lanes share scene t % P, each walking a slice of the keys.
    uint32_t P = 1u;
    while (P < B) P <<= 1;
    if (P >= kEsRankLanes) {
        for (uint32_t s0 = t; s0 < B; s0 += 4u * kEsRankLanes) {   // four scenes a walk
            unsigned long long key[4];
            uint32_t c[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 4; ++j) key[j] = s0 + j * kEsRankLanes < B ? es_lds[s0 + j * kEsRankLanes] : 0ull;   // 0: nothing is smaller
            for (uint32_t o = 0; o < B; ++o) {
                const unsigned long long other = es_lds[o];
#pragma unroll
                for (int j = 0; j < 4; ++j) c[j] += other < key[j] ? 1u : 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (s0 + j * kEsRankLanes < B) cnt[s0 + j * kEsRankLanes] = c[j];
        }
    } else {
        const uint32_t s = t & (P - 1u), slice = t / P, slices = kEsRankLanes / P;
        const uint32_t per = (B + slices - 1u) / slices;
        const uint32_t lo = slice * per, hi = lo + per < B ? lo + per : B;
        if (s < B) {
            const unsigned long long key = es_lds[s];
            uint32_t c = 0u;
            for (uint32_t o = lo; o < hi; ++o) c += es_lds[o] < key ? 1u : 0u;
            if (c) atomicAdd(cnt + s, c);
        }
    }
    __syncthreads();
    for (uint32_t s = t; s < B; s += kEsRankLanes) {
        const uint32_t r = cnt[s];
        rank[s] = r;
        if (report && r == B - 1u) {                               // one scene holds the top rank
            report[0] = s;
            report[1] = __float_as_uint(es_fitness(score[s], a));
            report[2] = cnt[B];
            report[3] = a.g;
        }
    }
}

// One wave per weight pair, the scene pairs over its lanes; lane 0 runs E7 for the pair's two weights.  In place where mean_out is
// mean_in: a wave reads and writes its own two words only.
__global__ __launch_bounds__(kEsUpdateLanes) void es_update_kernel(EsArgs a, const uint32_t *__restrict__ rank, const float *mean_in, float *mean_out)
{
    const uint32_t lane = threadIdx.x & 63u, p = blockIdx.x * (kEsUpdateLanes / 64u) + (threadIdx.x >> 6);
    const uint32_t mp = (a.m + 1u) >> 1, B = a.scenes;
    if (p >= mp) return;                                           // the whole wave
    const int32_t centre = (int32_t)B - 1;
    long long A0 = 0, A1 = 0;
    for (uint32_t q = lane; 2u * q < B; q += 64u) {
        int32_t k0, k1;
        es_draw_pair(a.seed, a.g, q, p, &k0, &k1);
        int32_t u = 2 * (int32_t)rank[2u * q] - centre;            // E6
        if (2u * q + 1u < B) u -= 2 * (int32_t)rank[2u * q + 1u] - centre;   // the mirrored scene takes -k
        A0 += (long long)u * k0, A1 += (long long)u * k1;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) A0 += __shfl_down(A0, d, 64), A1 += __shfl_down(A1, d, 64);
    if (lane == 0u) {
        const uint32_t m = 2u * p;
        mean_out[m] = es_mean(mean_in[m], a.step, A0);
        if (m + 1u < a.m) mean_out[m + 1u] = es_mean(mean_in[m + 1u], a.step, A1);
    }
}

hipError_t launch_es_perturb(const EsArgs &a, uint32_t first, uint32_t count, const float *mean, float *theta, hipStream_t s)
{
    const uint32_t mp = (a.m + 1u) >> 1, pairs = ((first + count - 1u) >> 1) - (first >> 1) + 1u;
    const uint32_t grid = (pairs * mp + kEsPerturbLanes - 1u) / kEsPerturbLanes;
    hipLaunchKernelGGL(es_perturb_kernel, dim3(grid), dim3(kEsPerturbLanes), 0, s, a, first, count, mean, theta);
    return hipGetLastError();
}

hipError_t launch_es_rank(const EsArgs &a, const SceneScore *score, uint32_t *rank, float *fitness, uint32_t *report, hipStream_t s)
{
    static_assert(12u * kEsMaxPopulation + 16u == 49168u, "the LDS of the largest population: below the default limit");
    const size_t lds = 12u * (size_t)a.scenes + 16u;
    hipLaunchKernelGGL(es_rank_kernel, dim3(1), dim3(kEsRankLanes), lds, s, a, score, rank, fitness, report);
    return hipGetLastError();
}

hipError_t launch_es_update(const EsArgs &a, const uint32_t *rank, const float *mean_in, float *mean_out, hipStream_t s)
{
    const uint32_t mp = (a.m + 1u) >> 1, per = kEsUpdateLanes / 64u;
    hipLaunchKernelGGL(es_update_kernel, dim3((mp + per - 1u) / per), dim3(kEsUpdateLanes), 0, s, a, rank, mean_in, mean_out);
    return hipGetLastError();
}
#endif   // __HIPCC__
