// nb_scenes_score.inc -- the score of scene batches (DESIGN.md section 14.5): every scene's current snapshot reduced to one 32-byte
// record of metrics -- pairs within a radius, spread about the centroid, kinetic sum, squared momentum, squared distance to a goal,
// bodies with a non-finite component -- and added to the record the scene keeps in device memory, in ONE kernel for the whole batch.
// A rollout is scored where it runs; the host reads 32 bytes a scene when it ends.
// Included by nb_kernels.hip inside namespace nbk, in the SLP-off unit behind nb_scenes_policy.inc: NOT in the two units whose device
// code kernel_code_sha() hashes.  Launcher: nb_scenes.h.
//
// The rule (include/nenbody.h Q1-Q7; tests/score_restatement.py states it again in numpy), every float operation one binary32
// operation in the order written, no contraction:
//   Q1  T(u): P the smallest power of two >= n, u_i = +0 for i >= n; for stride = P/2 .. 1: u_i = u_i + u_{i + stride}, i < stride
//   Q2  near: unordered pairs with ((dx dx) + (dy dy)) + (dz dz) < radius_sq, a NaN comparing false
//   Q3  spread = T(|p - c|^2), c = T(p) / (float)n per component
//   Q4  speed2 = T(|v|^2); momentum2 = |T(v)|^2
//   Q5  goal2 = T(|p - goal|^2)
//   Q6  nonfinite: bodies with a non-finite component of (p, v)
//   Q7  the record takes one add per field
//
// Shape: scenes_nbody_kernel's.  One workgroup per scene, the smallest of 64 .. 1 024 lanes that holds n; lane t owns body t and, in a
// scene of more than 1 024 bodies, body t + 1024 (TWO); more scenes than kScenesMaxGrid are walked by a grid-stride loop.  Dynamic
// LDS: the scene's position records (16 n bytes), the dump of the partial sums (8 x LANES words), the centroid and two counters:
// 16 n + 32 LANES + 32 bytes, 65 568 at n = 2 048.
//
// Why the bits do not depend on the shape.  Q2 and Q6 are integer counts: every lane counts its own hits, the wave sums them, the
// wave's first lane adds the sum to an LDS word, and integer addition is order-free.  Q1's stride order IS the shape: stride 1 024 pairs
// body t with body t + 1024, one lane's two bodies; strides 512 .. 64 pair lane t with lane t + stride, the same lane of another
// wave, so lane l of wave 0 folds the W words the waves left at l in the order of the strides (score_tree); strides 32 .. 1 are
// ds_bpermute reads inside wave 0.  A lane without a body holds +0, and a workgroup wider than P -- 64 lanes over a scene of 5 --
// runs strides above P/2 whose right operands are all padding: x + (+0) = x for every x but -0, so at most the sign of a zero sum
// differs from the rule's, which no field can observe (Q1; tests/test_scenes_score_cpu.py runs the tree both ways on every case).
//
// Q2 walks the upper triangle: the lanes of a wave read record j as ONE broadcast LDS read, j from the wave's first body + 1, and lane
// i counts j > i.  d2 is bitwise symmetric, so each unordered pair is met once and nothing is halved (section 14.5 has the measurement
// against the full walk).

#ifdef __HIPCC__
// Q2 for body i at p: lane i's hits among j > i.  The wave reads record j as one broadcast, so j starts behind the wave's first body.
__device__ __forceinline__ uint32_t score_near(const float4 *tile, uint32_t n, uint32_t i, const float4 p, float radius_sq)
{
    uint32_t c = 0;
#pragma unroll 8
    for (uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)i) + 1u; j < n; ++j) {
        const float4 q = tile[j];
        const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
        const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
        const float d2 = (xx + yy) + zz;
        c += (j > i && d2 < radius_sq) ? 1u : 0u;
    }
    return c;
}

// the sum of v over the wave, in lane 0 of the wave
__device__ __forceinline__ uint32_t score_wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_down((int)v, d, 64);
    return v;
}

// |p - o|^2 in Q3's form
__device__ __forceinline__ float score_dist2(const float4 p, float ox, float oy, float oz)
{
    const float ex = p.x - ox, ey = p.y - oy, ez = p.z - oz;
    const float xx = ex * ex, yy = ey * ey, zz = ez * ez;
    return (xx + yy) + zz;
}

// round one's eight leaves of one body: p.x, p.y, p.z, |v|^2, v.x, v.y, v.z, |p - goal|^2
__device__ __forceinline__ void score_leaves(const ScenesScoreArgs &a, const float4 p, const float4 v, float (&u)[8])
{
    u[0] = p.x, u[1] = p.y, u[2] = p.z;
    const float xx = v.x * v.x, yy = v.y * v.y, zz = v.z * v.z;
    u[3] = (xx + yy) + zz;
    u[4] = v.x, u[5] = v.y, u[6] = v.z;
    u[7] = score_dist2(p, a.gx, a.gy, a.gz);
}

__device__ __forceinline__ bool score_finite(const float4 p, const float4 v)
{
    return policy_finite(p.x) && policy_finite(p.y) && policy_finite(p.z) && policy_finite(v.x) && policy_finite(v.y) && policy_finite(v.z);
}

// Q1 below stride 1 024 for Q sums at once: u holds lane t's leaves; afterwards lane 0 holds the Q tree sums.  One dump, one barrier,
// then lane l of wave 0 folds the words of lanes l, l + 64, ... by strides LANES/2 .. 64 and the wave folds strides 32 .. 1.
template <int LANES, int Q>
__device__ __forceinline__ void score_tree(float *part, uint32_t t, float (&u)[Q])
{
    constexpr int W = LANES / 64;
#pragma unroll
    for (int q = 0; q < Q; ++q) part[q * LANES + t] = u[q];
    __syncthreads();
    if (t < 64u) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            float r[W];
#pragma unroll
            for (int w = 0; w < W; ++w) r[w] = part[q * LANES + w * 64 + t];
#pragma unroll
            for (int h = W / 2; h >= 1; h >>= 1)
#pragma unroll
                for (int w = 0; w < h; ++w) r[w] = r[w] + r[w + h];
            float x = r[0];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) x = x + __shfl_down(x, d, 64);
            u[q] = x;
        }
    }
}

template <int LANES, bool TWO>
__global__ __launch_bounds__(LANES) void scenes_score_kernel(ScenesScoreArgs a)
{
    extern __shared__ float4 score_lds[];                          // [n] position records
    const uint32_t t = threadIdx.x, n = a.n;
    float *part = reinterpret_cast<float *>(score_lds + n);        // [8][LANES] the dump of score_tree
    float *cen = part + 8 * LANES;                                 // the centroid, 3 words of 4
    uint32_t *counts = reinterpret_cast<uint32_t *>(cen + 4);      // near, nonfinite
    const bool live0 = t < n, live1 = TWO && t + (uint32_t)LANES < n;
    const float fn = (float)n;                                     // exact: n <= 2 048
    for (uint32_t s = blockIdx.x; s < a.scenes; s += gridDim.x) {
        const float4 *pos = a.pos + (size_t)s * n, *vel = a.vel + (size_t)s * n;
        float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), v0 = p0, p1 = p0, v1 = p0;
        if (live0) {
            p0 = pos[t], v0 = vel[t];
            score_lds[t] = p0;
        }
        if (TWO && live1) {
            p1 = pos[t + LANES], v1 = vel[t + LANES];
            score_lds[t + LANES] = p1;
        }
        if (t < 2u) counts[t] = 0u;
        __syncthreads();
        // Q2 and Q6: every lane's counts summed over its wave, then added to the scene's by the wave's first lane
        uint32_t near = 0u;
        if (live0) near += score_near(score_lds, n, t, p0, a.radius_sq);
        if (TWO && live1) near += score_near(score_lds, n, t + LANES, p1, a.radius_sq);
        uint32_t bad = (live0 && !score_finite(p0, v0)) ? 1u : 0u;
        if (TWO) bad += (live1 && !score_finite(p1, v1)) ? 1u : 0u;
        near = score_wave_sum(near), bad = score_wave_sum(bad);
        if ((t & 63u) == 0u) {
            if (near) atomicAdd(counts + 0, near);
            if (bad) atomicAdd(counts + 1, bad);
        }
        // round one: the eight sums; stride 1 024 is the lane's own second body
        float u[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (live0) score_leaves(a, p0, v0, u);
        if (TWO) {
            float w[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (live1) score_leaves(a, p1, v1, w);
#pragma unroll
            for (int q = 0; q < 8; ++q) u[q] = u[q] + w[q];
        }
        score_tree<LANES, 8>(part, t, u);
        if (t == 0u) cen[0] = u[0] / fn, cen[1] = u[1] / fn, cen[2] = u[2] / fn;   // Q3: the IEEE quotient
        __syncthreads();                                           // the centroid is there; wave 0 has read the dump
        // round two: spread
        const float cx = cen[0], cy = cen[1], cz = cen[2];
        float e[1] = {live0 ? score_dist2(p0, cx, cy, cz) : 0.f};
        if (TWO) {
            const float e1 = live1 ? score_dist2(p1, cx, cy, cz) : 0.f;
            e[0] = e[0] + e1;
        }
        score_tree<LANES, 1>(part, t, e);
        if (t == 0u) {                                             // Q7: one lane reads, updates and writes the record
            const float mx = u[4] * u[4], my = u[5] * u[5], mz = u[6] * u[6];
            SceneScore r = a.score[s];
            r.near += counts[0];
            r.spread = r.spread + e[0];
            r.speed2 = r.speed2 + u[3];
            r.momentum2 = r.momentum2 + ((mx + my) + mz);
            r.goal2 = r.goal2 + u[7];
            r.steps += 1u;
            r.nonfinite += counts[1];
            a.score[s] = r;
        }
        // the next scene stages positions and, in lanes of wave 0 behind this read, clears the counters; its first dump lies behind
        // its staging barrier, which wave 0 reaches with round two's reads done
    }
}

struct ScenesScoreLaunch {
    const ScenesScoreArgs &a;
    hipStream_t s;
    template <int LANES, bool TWO>
    hipError_t operator()() const
    {
        static_assert((size_t)kScenesMaxBodies * sizeof(float4) + 8u * 1024u * sizeof(float) + 32u == 65568u, "the LDS of the largest scene");
        const size_t lds = (size_t)a.n * sizeof(float4) + 8u * LANES * sizeof(float) + 32u;   // 65 568 B at n = 2 048: above the default limit
        return launch_scenes_scene<LANES>(scenes_score_kernel<LANES, TWO>, a.scenes, lds, s, a);
    }
};
hipError_t launch_scenes_score(const ScenesScoreArgs &a, hipStream_t s) { return scenes_by_size(a.n, ScenesScoreLaunch{a, s}); }
#endif   // __HIPCC__
