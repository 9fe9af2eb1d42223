// nb_boids.inc -- boids controller (update_instance_boids, main.rs:443-526): one-lane-per-body kernel (plain and (x, y)-packed),
// chain-split kernel (two waves per 64 bodies) and producer/consumer kernel; nb_api.hip:boids_form picks by bodies per rank.
// Included by nb_kernels.hip inside namespace nbk; see that file for the compilation scheme.
// What the forms share is stated once: boids_wave_flags, BoidsOwn / boids_own (a lane's own body), boids_mask_vgprs, BoidsStage /
// boids_stage_fetch / boids_stage_publish and BoidsTileHead / boids_tile_head (the LDS tile of the one-lane and chain-split
// kernels; the head also serves the producer/consumer body), BOIDS_FOLD_BY_FLAGS (the form ladder), boids_finish (the epilogue,
// also of nb_seen.inc) and BOIDS_LAUNCH (the tile and packed switches of the launchers).

// ------------------------------------------------------------------------------------------------
// Boids controller: update_instance_boids, main.rs:443-526 (SURVEY.md section 8f, rank 1).
//
// Three index-ordered, predicated folds per body over the snapshots of all positions / all velocities:
//   rule 1 (main.rs:471-480)  centre += p_i, count += 1      if |p_i - p_n|^2      < rule_1_distance && i != n
//   rule 2 (main.rs:482-492)  repel  -= (p_i - p_n)           if sqrt(|p_i - p_n|^2) < rule_2_distance && i != n
//   rule 3 (main.rs:494-504)  match  += v_i, vcount += 1      if sqrt(|v_i - v_n|^2) < rule_3_distance && i != n
// One lane per body, j in index order, so every sum sees the reference's sequence of additions.  The two sqrt
// predicates are evaluated WITHOUT a sqrt: sqrt is monotonic and correctly rounded in the reference, so
// `sqrt(x) < r` holds exactly for x <= T(r), T(r) = the largest binary32 whose correctly rounded root is below r;
// nb_api computes T on the host (bisection over bit patterns with the host's IEEE sqrtf).  NaN fails every test on
// both sides.  The epilogue (means, velocity blend, speed clamp, position update: main.rs:506-521) runs once per
// body with the correctly rounded '/' and sqrt.
//
// Per-tile specialisations, all exact (chosen from flags the loaders compute while staging a tile):
//   SELF    only the tile that contains the workgroup's own bodies tests `i != n`; elsewhere it is true by range.
//   MASKED  every record of the tile finite: a skipped term is added as 0 * x through an FMA with a 0/1 mask --
//           fma(1, x, s) == s + x and fma(0, x, s) == s for finite x (the sums never hold -0: they start at +0 and
//           x + (-x) rounds to +0) -- one compare + one select per rule instead of a select per component.
//           Non-finite records take the select-on-result form, which leaves a skipped sum untouched whatever x is.
//   PLANAR  every z (positions and velocities, tile and own bodies) is +/-0: the z terms contribute +/-0 to the
//           squared distances and leave the z sums at +0, so they are skipped (the reference's initial state is
//           planar, main.rs:740,745, and stays planar).
//   ALL3    every velocity component of the tile and of the own bodies has magnitude <= v_lim, the host's bound
//           (nb_api.hip:rule3_always_bound) below which the rule-3 test cannot fail: |v_i - v_n| <= 2 v_lim per
//           component, every rounding is monotonic, so the squared distance as the reference rounds it is at most
//           ((2v)^2 + (2v)^2) + (2v)^2 evaluated in binary32 at v = v_lim, which the host chose <= t3.  Then rule 3 adds
//           EVERY v_i (i != n is true by range outside the SELF tile) and its count is the tile's length: the seven
//           operations of the velocity distance, its test and its mask drop out.  With the reference's own constants
//           (rule_3_distance = 500 against speeds clamped to 1, main.rs:453, 516-518) this is every tile.
// These kernels live in the SLP-off translation unit: the compiler's own packing of the loop cost 25 % in register shuffles
// (the hand-packed pair further down is used only where a wave is alone on its SIMD).
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kBoidsNonFinite = 1u;  // some coordinate is inf/NaN -> select form
constexpr uint32_t kBoidsNonPlanar = 2u;  // some z != 0 (position or velocity)
constexpr uint32_t kBoidsVelFar = 4u;     // some velocity component above v_lim (or not finite): rule 3 must be tested
constexpr uint32_t kBoidsSelfTile = 8u;   // (producer/consumer kernel, per-tile word) the tile holds the workgroup's own bodies: i != n is tested
// rule 3 known to hold for every pair of the tile (ALL3 above): finite records within the bound, and no i == n to exclude
__device__ __forceinline__ bool boids_all3(uint32_t flags) { return (flags & (kBoidsNonFinite | kBoidsVelFar | kBoidsSelfTile)) == 0u; }

__device__ __forceinline__ uint32_t boids_flags(const float4 p, const float4 v, uint32_t vlim_bits)
{
    auto nonfinite = [](float c) { return (__float_as_uint(c) & 0x7f800000u) == 0x7f800000u ? kBoidsNonFinite : 0u; };
    auto nonzero = [](float c) { return (__float_as_uint(c) & 0x7fffffffu) != 0u ? kBoidsNonPlanar : 0u; };
    auto far = [vlim_bits](float c) { return (__float_as_uint(c) & 0x7fffffffu) > vlim_bits ? kBoidsVelFar : 0u; };
    return nonfinite(p.x) | nonfinite(p.y) | nonfinite(p.z) | nonfinite(v.x) | nonfinite(v.y) | nonfinite(v.z) | nonzero(p.z) |
           nonzero(v.z) | far(v.x) | far(v.y) | far(v.z);
}
// the three record flags of a whole wave (every lane takes part)
__device__ __forceinline__ uint32_t boids_wave_flags(uint32_t f)
{
    return (__any((int)(f & kBoidsNonFinite)) ? kBoidsNonFinite : 0u) | (__any((int)(f & kBoidsNonPlanar)) ? kBoidsNonPlanar : 0u) |
           (__any((int)(f & kBoidsVelFar)) ? kBoidsVelFar : 0u);
}

// A lane's own body, the same in every form: `bodies` (256, or 64 in the producer/consumer form) per workgroup, `within` this
// lane's place among them.  A lane past the shard folds for the shard's last body and writes nothing.
struct BoidsOwn {
    uint32_t l;               // index within the shard
    bool live;
    uint32_t gn;              // this body's global index n
    float4 pn, vn;
    uint32_t self;            // the wave's own bodies' flags, the forced ones (tests) OR-ed in
    uint32_t own_lo, own_hi;  // global index range of the workgroup's bodies: only tiles overlapping it can contain i == n
};                            // (own_hi exclusive; past-the-shard indices never match a live body)
__device__ __forceinline__ BoidsOwn boids_own(const BoidsArgs &a, uint32_t bodies, uint32_t within)
{
    BoidsOwn o;
    o.l = blockIdx.x * bodies + within;
    o.live = o.l < a.count;
    o.gn = a.first + (o.live ? o.l : a.count - 1u);
    o.pn = a.pos_in[o.gn];
    o.vn = a.vel_in[o.gn];
    o.self = boids_wave_flags(boids_flags(o.pn, o.vn, a.vlim_bits) | a.force_flags);
    o.own_lo = a.first + blockIdx.x * bodies;
    o.own_hi = o.own_lo + bodies;
    return o;
}

// the radius-test constants in vector registers, once (boids_below)
__device__ __forceinline__ BoidsMaskK boids_mask_vgprs(const BoidsArgs &a)
{
    BoidsMaskK mkv = a.mk;
    asm("" : "+v"(mkv.k1), "+v"(mkv.tk1), "+v"(mkv.k2), "+v"(mkv.tk2), "+v"(mkv.k3), "+v"(mkv.tk3));
    return mkv;
}

// `x < T` as 1.0f / 0.0f in ONE instruction (round 3; a compare and a select before).  k is a power of two with T * k in
// [2^30, 2^31): the FMA forms T*k - x*k with a single rounding, so its sign is that of T - x and it is zero only for x == T;
// a positive result is at least 2^(e_T - 24) * k = 2^6 (the smallest gap between T and a binary32 below it), so the clamp to
// [0, 1] -- an output modifier, free -- gives exactly 1; x*k overflowing gives -inf -> 0; NaN -> 0 (DX10 clamp), like a compare.
// Operands in vector registers (a scalar source halves a plain instruction's rate).
__device__ __forceinline__ float boids_below(float x, float k, float tk)
{
    float m;
    asm("v_fma_f32 %0, -%1, %2, %3 clamp" : "=v"(m) : "v"(x), "v"(k), "v"(tk));
    return m;
}

struct BoidsAcc {
    float cx, cy, cz, rx, ry, rz, mx, my, mz;  // main.rs:472, 483, 495: all start at Vector3::new(0.0, 0.0, 0.0)
    float cnt, vcnt;                           // counts kept in binary32: exact below 2^24 (nb_api refuses larger sets)
};

// ROLE: 0 = all three rules; 1 = rule 1 only, 2 = rules 2 and 3 only (boids_split_kernel: two waves per body share the chains);
// 3 = rules 1 and 2 only (the split form when rule 3 is known to hold for EVERY pair of the step: its sum is the total of the
// velocities minus the body's own, its count n - 1 -- boids_combine_kernel)
template <bool SELF, bool MASKED, bool PLANAR, bool ALL3, int ROLE = 0>
__device__ __forceinline__ void boids_pair(BoidsAcc &s, const float4 pv, const float2 zz, uint32_t j, uint32_t gn,
                                           const float4 pn, const float4 vn, float r1, float t2, float t3, const BoidsMaskK &mk)
{
    // The tile holds (px, py, vx, vy) in one 16-byte record and (pz, vz) in a second array: a planar pair costs ONE
    // ds_read_b128 (4 LDS cycles).  With a position and a velocity record per pair the LDS pipe, not the vector ALU, bounded
    // the planar loop once rule 3 had dropped out of it (8 LDS cycles against 9 issue cycles per pair and CU).
    const float3 pj = make_float3(pv.x, pv.y, PLANAR ? 0.f : zz.x), vj = make_float3(pv.z, pv.w, PLANAR ? 0.f : zz.y);
    const bool ne = SELF ? (j != gn) : true;                              // main.rs:475 n != i
    const float dx = pj.x - pn.x, dy = pj.y - pn.y;                       // distance2: (other - self)
    const float dz = PLANAR ? 0.f : pj.z - pn.z;
    float d2 = (dx * dx) + (dy * dy);
    if (!PLANAR) d2 = d2 + (dz * dz);
    const bool p1 = (d2 < r1) && ne;                                      // main.rs:474-475 (squared distance)
    const bool p2 = (d2 <= t2) && ne;                                     // main.rs:485-486  sqrt(d2) < rule_2_distance
    static_assert(!ALL3 || (MASKED && !SELF), "ALL3: finite records, i != n by range");
    constexpr bool R1 = ROLE != 2, R23 = ROLE != 1, R3 = ROLE != 1 && ROLE != 3;
    bool p3 = true;
    float3 e = make_float3(0.f, 0.f, 0.f);
    if (!ALL3 && R3) {
        e.x = vj.x - vn.x, e.y = vj.y - vn.y;
        e.z = PLANAR ? 0.f : vj.z - vn.z;
        float e2 = (e.x * e.x) + (e.y * e.y);
        if (!PLANAR) e2 = e2 + (e.z * e.z);
        p3 = (e2 <= t3) && ne;                                            // main.rs:497-498  sqrt(e2) < rule_3_distance
    }
    if (MASKED) {  // (never a SELF tile: i != n holds by range; every record finite)
        if (R1) {
            const float m1 = boids_below(d2, mk.k1, mk.tk1);              // main.rs:474-475 as a 0/1 mask, one instruction
            s.cx = __builtin_fmaf(m1, pj.x, s.cx);                        // main.rs:476  sum + p_i
            s.cy = __builtin_fmaf(m1, pj.y, s.cy);
            if (!PLANAR) s.cz = __builtin_fmaf(m1, pj.z, s.cz);
            s.cnt = s.cnt + m1;
        }
        if (R23) {
            const float m2 = boids_below(d2, mk.k2, mk.tk2);              // main.rs:485-486, +1 where the rule holds
            s.rx = __builtin_fmaf(m2, -dx, s.rx);                         // main.rs:487  sum - (p_i - p_n):  (+1) * (-d) == (-1) * d
            s.ry = __builtin_fmaf(m2, -dy, s.ry);
            if (!PLANAR) s.rz = __builtin_fmaf(m2, -dz, s.rz);
            if (!R3) {  // (rule 3 comes from the step's total: boids_combine_kernel)
            } else if (ALL3) {
                s.mx = s.mx + vj.x;                                       // main.rs:499, the test known to hold
                s.my = s.my + vj.y;
                if (!PLANAR) s.mz = s.mz + vj.z;                          // vcount: the caller adds the tile's length
            } else {
                float e2 = (e.x * e.x) + (e.y * e.y);
                if (!PLANAR) e2 = e2 + (e.z * e.z);
                const float m3 = boids_below(e2, mk.k3, mk.tk3);          // main.rs:497-498
                s.mx = __builtin_fmaf(m3, vj.x, s.mx);                    // main.rs:499  sum + v_i
                s.my = __builtin_fmaf(m3, vj.y, s.my);
                if (!PLANAR) s.mz = __builtin_fmaf(m3, vj.z, s.mz);
                s.vcnt = s.vcnt + m3;
            }
        }
    } else {
        if (R1) {
            const float c1x = s.cx + pj.x, c1y = s.cy + pj.y, c1z = s.cz + pj.z;
            s.cx = p1 ? c1x : s.cx;
            s.cy = p1 ? c1y : s.cy;
            s.cz = p1 ? c1z : s.cz;
            s.cnt = p1 ? s.cnt + 1.f : s.cnt;
        }
        if (R23) {
            const float r1x = s.rx - dx, r1y = s.ry - dy, r1z = s.rz - dz;
            s.rx = p2 ? r1x : s.rx;
            s.ry = p2 ? r1y : s.ry;
            s.rz = p2 ? r1z : s.rz;
            if (R3) {
                const float m1x = s.mx + vj.x, m1y = s.my + vj.y, m1z = s.mz + vj.z;
                s.mx = p3 ? m1x : s.mx;
                s.my = p3 ? m1y : s.my;
                s.mz = p3 ? m1z : s.mz;
                s.vcnt = p3 ? s.vcnt + 1.f : s.vcnt;
            }
        }
    }
}

// The planar masked pair with (x, y) in one register pair per quantity: the tile record IS (px, py | vx, vy), so the
// differences, their squares, and the three (x, y) sums are one v_pk_* each -- 11 instructions per pair (ALL3; 18 when rule 3
// is tested) instead of 16 (24).  Same operations on the same operands in the same order, hence the same bits; the lane
// operations are the same too, so this buys nothing where the vector ALU is saturated, but a one-lane-per-body launch runs
// two waves per SIMD or ONE (shards of up to 65 536 bodies), and a lone wave issues an instruction every ~5 cycles whatever
// its width.  (The compiler's own SLP packing of this loop cost 25 % in shuffles; this unit is built without it.)
struct BoidsAcc2 {
    v2f c, r, m;
    float cnt, vcnt;
};

template <bool ALL3, int ROLE = 0>
__device__ __forceinline__ void boids_pair_packed(BoidsAcc2 &s, const float4 pv, const v2f pn, const v2f vn, float r1, float t2, float t3,
                                                  const BoidsMaskK &mk)
{
    constexpr bool R1 = ROLE != 2, R23 = ROLE != 1;
    const v2f pj = {pv.x, pv.y}, vj = {pv.z, pv.w};
    const v2f d = pj - pn;                                                // distance2: (other - self)
    const v2f dd = d * d;
    const float d2 = dd.x + dd.y;
    if (R1) {
        const float m1 = boids_below(d2, mk.k1, mk.tk1);                  // main.rs:474-475 (i != n by range: not the SELF tile)
        s.c = __builtin_elementwise_fma(v2f{m1, m1}, pj, s.c);            // main.rs:476  sum + p_i
        s.cnt = s.cnt + m1;
    }
    if (R23) {
        const float m2 = boids_below(d2, mk.k2, mk.tk2);                  // main.rs:485-486, +1 where the rule holds
        s.r = __builtin_elementwise_fma(v2f{m2, m2}, -d, s.r);            // main.rs:487  sum - (p_i - p_n): (+1) * (-d) == (-1) * d
        if (ALL3) {
            s.m = s.m + vj;                                               // main.rs:499, the test known to hold
        } else {
            const v2f e = vj - vn;
            const v2f ee = e * e;
            const float e2 = ee.x + ee.y;
            const float m3 = boids_below(e2, mk.k3, mk.tk3);              // main.rs:497-498
            s.m = __builtin_elementwise_fma(v2f{m3, m3}, vj, s.m);
            s.vcnt = s.vcnt + m3;
        }
    }
}

template <bool SELF, bool MASKED, bool PLANAR, bool ALL3, bool PACKED, int ROLE = 0>
__device__ __forceinline__ void boids_fold_tile(BoidsAcc &s, const float4 *tpv, const float2 *tz, int nj, uint32_t j0, uint32_t gn,
                                                const float4 pn, const float4 vn, float r1, float t2, float t3, const BoidsMaskK &mk)
{
    // Two register sets of U records: group g+U is read from LDS while group g is evaluated (a one-lane-per-body launch
    // runs two waves per SIMD, too few to hide a read issued right before its use; the scheduling barriers keep the
    // compiler from sinking the reads back down to their uses).
    constexpr int U = 8;
    struct Group {
        float4 pv[U];
        float2 z[PLANAR ? 1 : U];
    };
    const float2 none = make_float2(0.f, 0.f);
    auto load = [&](Group &r, int j) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            r.pv[u] = tpv[j + u];
            if (!PLANAR) r.z[PLANAR ? 0 : u] = tz[j + u];
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    constexpr bool kPacked = PACKED && PLANAR && MASKED && !SELF;
    BoidsAcc2 s2 = {v2f{s.cx, s.cy}, v2f{s.rx, s.ry}, v2f{s.mx, s.my}, s.cnt, s.vcnt};
    const v2f pn2 = {pn.x, pn.y}, vn2 = {vn.x, vn.y};
    auto eval = [&](const Group &r, int j) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (kPacked)
                boids_pair_packed<ALL3, ROLE>(s2, r.pv[u], pn2, vn2, r1, t2, t3, mk);
            else
                boids_pair<SELF, MASKED, PLANAR, ALL3, ROLE>(s, r.pv[u], PLANAR ? none : r.z[PLANAR ? 0 : u], j0 + (uint32_t)(j + u), gn, pn, vn, r1, t2, t3, mk);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    int g = 0;
    if (2 * U <= nj) {
        Group a, b;
        load(a, 0);
        for (; g + 4 * U <= nj; g += 2 * U) {
            load(b, g + U);
            eval(a, g);
            load(a, g + 2 * U);
            eval(b, g + U);
        }
        load(b, g + U);
        eval(a, g);
        eval(b, g + U);
        g += 2 * U;
    }
    for (; g < nj; ++g) {
        if (kPacked)
            boids_pair_packed<ALL3, ROLE>(s2, tpv[g], pn2, vn2, r1, t2, t3, mk);
        else
            boids_pair<SELF, MASKED, PLANAR, ALL3, ROLE>(s, tpv[g], PLANAR ? none : tz[g], j0 + (uint32_t)g, gn, pn, vn, r1, t2, t3, mk);
    }
    if (kPacked) {
        s.cx = s2.c.x, s.cy = s2.c.y, s.rx = s2.r.x, s.ry = s2.r.y, s.mx = s2.m.x, s.my = s2.m.y;
        s.cnt = s2.cnt, s.vcnt = s2.vcnt;
    }
    if (ALL3 && ROLE != 1 && ROLE != 3) s.vcnt = s.vcnt + (float)nj;  // nj ones: counts are integers below 2^24, exact in binary32 either way
}

// What the LDS-tiled kernels (one lane per body, chain split) share: a tile of TJ records is (px, py, vx, vy) in tile_pv, (pz, vz)
// in tile_z and one flag word per staging wave in tile_flags; THREADS threads stage it, R = TJ / THREADS records each, through
// registers (the next tile's loads are in flight while this one is folded).  A record past the end of the set is the zero record.
template <int R>
struct BoidsStage {
    float4 p[R], v[R];
};
template <int THREADS, int R>
__device__ __forceinline__ void boids_stage_fetch(BoidsStage<R> &st, const BoidsArgs &a, uint32_t j0, int tid)
{
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const uint32_t j = j0 + (uint32_t)(k * THREADS + tid);
        st.p[k] = (j < a.n_total) ? a.pos_in[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const uint32_t j = j0 + (uint32_t)(k * THREADS + tid);
        st.v[k] = (j < a.n_total) ? a.vel_in[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
template <int THREADS, int R>
__device__ __forceinline__ void boids_stage_publish(const BoidsStage<R> &st, const BoidsArgs &a, float4 *tile_pv, float2 *tile_z,
                                                    uint32_t *tile_flags, int tid)
{
    uint32_t f = 0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        f |= boids_flags(st.p[k], st.v[k], a.vlim_bits);
        tile_pv[k * THREADS + tid] = make_float4(st.p[k].x, st.p[k].y, st.v[k].x, st.v[k].y);
        tile_z[k * THREADS + tid] = make_float2(st.p[k].z, st.v[k].z);
    }
    f = boids_wave_flags(f);
    if ((tid & 63) == 0) tile_flags[tid >> 6] = f;
}
template <int W>
__device__ __forceinline__ uint32_t boids_or_words(const uint32_t *w)
{
    uint32_t f = 0;
#pragma unroll
    for (int i = 0; i < W; ++i) f |= w[i];
    return f;
}

// per-tile bookkeeping of tile t of TJ records (all uniform): its first record, its length, whether it overlaps the workgroup's
// own bodies, and its W flag words OR-ed into the own bodies' flags
struct BoidsTileHead {
    uint32_t j0;
    int nj;
    bool has_self;
    uint32_t flags;
};
template <int TJ, int W>
__device__ __forceinline__ BoidsTileHead boids_tile_head(uint32_t t, uint32_t n, const BoidsOwn &o, uint32_t self, const uint32_t *tile_flags)
{
    BoidsTileHead h;
    h.j0 = t * (uint32_t)TJ;
    const uint32_t left = n - h.j0;
    h.nj = left < (uint32_t)TJ ? (int)left : TJ;
    h.flags = self | boids_or_words<W>(tile_flags);
    h.has_self = h.j0 < o.own_hi && h.j0 + (uint32_t)h.nj > o.own_lo;
    return h;
}

// The form ladder: a tile's fold chosen from its flags (the specialisations at the top of this file), for head `h` of the tile in
// tile_pv / tile_z and own bodies `o`.  ROLE 3 folds no rule 3 (the split form where the step's total supplies it), so
// kBoidsVelFar, which only says whether rule 3 must be tested, chooses nothing there.  A macro with local copies of what it
// reads, not a function: as a __forceinline__ template the same ladder leaves boids_step_kernel with 52 scalar registers where
// the ladder written out in the kernel has 54 (DESIGN.md section 4.3, "One tile pipeline"), and the change that introduced it
// had to leave every kernel's resources as they were.
#define BOIDS_FOLD_BY_FLAGS(PACKED, ROLE, s, h, tile_pv, tile_z, o, a, mkv)                                                     \
    do {                                                                                                                        \
        constexpr bool kRule3 = (ROLE) != 3;                                                                                    \
        constexpr uint32_t k3dFar = kBoidsNonPlanar | kBoidsVelFar;                                                             \
        const float4 *tp = (tile_pv);                                                                                           \
        const float2 *tv = (tile_z);                                                                                            \
        const uint32_t f = (h).flags, j0 = (h).j0, gn = (o).gn;                                                                 \
        const bool has_self = (h).has_self;                                                                                     \
        const int nj = (h).nj;                                                                                                  \
        const float4 pn = (o).pn, vn = (o).vn;                                                                                  \
        if (has_self || (f & kBoidsNonFinite))                                                                                  \
            boids_fold_tile<true, false, false, false, false, ROLE>(s, tp, tv, nj, j0, gn, pn, vn, (a).r1, (a).t2, (a).t3, mkv);  \
        else if (kRule3 && (f & k3dFar) == k3dFar)                                                                              \
            boids_fold_tile<false, true, false, false, false, ROLE>(s, tp, tv, nj, j0, gn, pn, vn, (a).r1, (a).t2, (a).t3, mkv);  \
        else if (kRule3 && (f & kBoidsVelFar))                                                                                  \
            boids_fold_tile<false, true, true, false, PACKED, ROLE>(s, tp, tv, nj, j0, gn, pn, vn, (a).r1, (a).t2, (a).t3, mkv);  \
        else if (f & kBoidsNonPlanar)                                                                                           \
            boids_fold_tile<false, true, false, true, false, ROLE>(s, tp, tv, nj, j0, gn, pn, vn, (a).r1, (a).t2, (a).t3, mkv);   \
        else                                                                                                                    \
            boids_fold_tile<false, true, true, true, PACKED, ROLE>(s, tp, tv, nj, j0, gn, pn, vn, (a).r1, (a).t2, (a).t3, mkv);   \
    } while (0)

// main.rs:506-521 for one body: means, blend, speed clamp, position update -- the arithmetic, stated once; boids_finish stores its
// records, the scene-batch kernel (nb_scenes.inc) keeps them on chip
__device__ __forceinline__ void boids_finish_records(const BoidsArgs &a, const BoidsAcc &s, const float4 pn, float4 &p_new, float4 &v_new)
{
    float cx = s.cx, cy = s.cy, cz = s.cz, mx = s.mx, my = s.my, mz = s.mz;
    if (s.cnt > 0.f) {  // main.rs:506-508  (count as f32)
        cx = cx / s.cnt;
        cy = cy / s.cnt;
        cz = cz / s.cnt;
    }
    if (s.vcnt > 0.f) {  // main.rs:510-512
        mx = mx / s.vcnt;
        my = my / s.vcnt;
        mz = mz / s.vcnt;
    }
    // main.rs:514  vel = center*s1 + repel*s2 + match*s3, left to right, every product and sum rounded
    const float ax = cx * a.s1, ay = cy * a.s1, az = cz * a.s1;
    const float bx = s.rx * a.s2, by = s.ry * a.s2, bz = s.rz * a.s2;
    const float gx = mx * a.s3, gy = my * a.s3, gz = mz * a.s3;
    float vx = (ax + bx) + gx, vy = (ay + by) + gy, vz = (az + bz) + gz;
    // main.rs:516-518  |vel| > 1 -> vel * (1 / |vel|).  __builtin_sqrtf is correctly rounded under
    // -fhip-fp32-correctly-rounded-divide-sqrt (__fsqrt_rn is NOT: it is the 1-ulp v_sqrt_f32).
    const float q0 = vx * vx, q1 = vy * vy, q2 = vz * vz;
    const float mag = __builtin_sqrtf((q0 + q1) + q2);
    if (mag > 1.0f) {
        const float sc = 1.0f / mag;
        vx = vx * sc;
        vy = vy * sc;
        vz = vz * sc;
    }
    // main.rs:521  pos = vel * dt + pos
    const float sx = vx * a.dt, sy = vy * a.dt, sz = vz * a.dt;
    v_new = make_float4(vx, vy, vz, 0.f);
    p_new = make_float4(sx + pn.x, sy + pn.y, sz + pn.z, 0.f);
}
__device__ __forceinline__ void boids_finish(const BoidsArgs &a, const BoidsAcc &s, uint32_t l, const float4 pn)
{
    float4 p, v;
    boids_finish_records(a, s, pn, p, v);
    a.vel_out[a.first + l] = v;
    a.pos_out[a.first + l] = p;
}

// Split form, first launch: the step's global flags (a non-finite record, a velocity component above the rule-3 bound -- OR-ed
// into one word, which the host clears in front of the launch) and the sum of ALL velocities, 1 024 records per workgroup in a
// fixed order (four per lane, a tree through LDS): where the flags stay clear, rule 3 holds for every pair (boids_all3's argument,
// for the whole step), so its sum is that total minus the body's own velocity and its count n - 1: two of the fourteen operations
// per pair leave the slices' loops.  (Reassociated like everything in the split form; the bit-exact kernels never take this.)
__global__ __launch_bounds__(kBlock) void boids_prep_kernel(BoidsArgs a)
{
    __shared__ float4 red[kBlock];
    const uint32_t base = blockIdx.x * 1024u + threadIdx.x;
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t f = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t j = base + (uint32_t)k * kBlock;
        if (j < a.n_total) {
            const float4 p = a.pos_in[j], v = a.vel_in[j];
            f |= boids_flags(p, v, a.vlim_bits);
            sum.x = sum.x + v.x, sum.y = sum.y + v.y, sum.z = sum.z + v.z;
        }
    }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const float4 o = red[threadIdx.x + w];
            float4 m = red[threadIdx.x];
            m.x = m.x + o.x, m.y = m.y + o.y, m.z = m.z + o.z;
            red[threadIdx.x] = m;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) a.vtot[blockIdx.x] = red[0];
    // the wave's flags first (every lane takes part), then one lane reports them
    const uint32_t wf = (__any((int)(f & kBoidsNonFinite)) ? kBoidsNonFinite : 0u) | (__any((int)(f & kBoidsVelFar)) ? kBoidsVelFar : 0u);
    if (wf && (threadIdx.x & 63) == 0) atomicOr(a.gflags, wf);
}
__device__ __forceinline__ bool boids_no3(const BoidsArgs &a)
{
    return a.gflags && (a.force_flags & 4u) == 0u &&
           ((uint32_t)__builtin_amdgcn_readfirstlane((int)*a.gflags) & (kBoidsNonFinite | kBoidsVelFar)) == 0u;
}

// PACKED: planar tiles take boids_pair_packed -- for launches of at most one wave per SIMD (nb_api.hip:boids_form)
// SLICED (round 4, "split" form: nb_launch_boids_step_split): gridDim.y slices of the j range, a.j_chunk records each (whole
// tiles); a workgroup folds its slice only and leaves its eleven sums as a row of a.partial; boids_combine_kernel adds a body's
// rows in slice order and finishes.  Every predicate is evaluated on the same operands with the same bits as in the unsliced
// kernel, so the neighbour sets and the counts are the reference's; the SUMS are added in another order (within a slice in index
// order, then slice by slice): a tolerance form, for shards whose bodies alone cannot fill the chip.
template <int TJ, bool PACKED, bool SLICED = false>
__global__ __launch_bounds__(kBlock) void boids_step_kernel(BoidsArgs a)
{
    __shared__ float4 tile_pv[2][TJ];  // (px, py, vx, vy)
    __shared__ float2 tile_z[2][TJ];   // (pz, vz): read by 3-D tiles only
    __shared__ uint32_t tile_flags[2][kWaves];
    __shared__ uint32_t self_flags[kWaves];

    const int tid = threadIdx.x;
    const BoidsOwn o = boids_own(a, (uint32_t)kBlock, (uint32_t)tid);
    if ((tid & 63) == 0) self_flags[tid >> 6] = o.self;

    BoidsStage<TJ / kBlock> st;
    const uint32_t n = a.n_total;
    const uint32_t ntiles_all = (n + (uint32_t)TJ - 1u) / (uint32_t)TJ;
    const uint32_t t_lo = SLICED ? blockIdx.y * (a.j_chunk / (uint32_t)TJ) : 0u;
    const uint32_t t_end = SLICED ? t_lo + a.j_chunk / (uint32_t)TJ : ntiles_all;
    const uint32_t ntiles = t_end < ntiles_all ? t_end : ntiles_all;  // (a slice past the end of the set folds nothing)
    boids_stage_fetch<kBlock>(st, a, t_lo * (uint32_t)TJ, tid);
    boids_stage_publish<kBlock>(st, a, tile_pv[0], tile_z[0], tile_flags[0], tid);
    __syncthreads();
    const uint32_t block_self = boids_or_words<kWaves>(self_flags);
    // split form: did boids_prep_kernel find every record of the step finite and every velocity component inside the rule-3 bound?
    // Then rule 3 holds for every pair of the step and its sum comes from the total (boids_combine_kernel).
    const bool no3 = SLICED && boids_no3(a);

    const BoidsMaskK mkv = boids_mask_vgprs(a);
    BoidsAcc s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int buf = 0;
    for (uint32_t t = t_lo; t < ntiles; ++t) {
        const bool more = (t + 1u) < ntiles;
        if (more) boids_stage_fetch<kBlock>(st, a, (t + 1u) * (uint32_t)TJ, tid);
        const BoidsTileHead h = boids_tile_head<TJ, kWaves>(t, n, o, block_self, tile_flags[buf]);
        if (SLICED && no3)
            BOIDS_FOLD_BY_FLAGS(PACKED, 3, s, h, tile_pv[buf], tile_z[buf], o, a, mkv);
        else
            BOIDS_FOLD_BY_FLAGS(PACKED, 0, s, h, tile_pv[buf], tile_z[buf], o, a, mkv);
        if (more) boids_stage_publish<kBlock>(st, a, tile_pv[buf ^ 1], tile_z[buf ^ 1], tile_flags[buf ^ 1], tid);
        __syncthreads();
        buf ^= 1;
    }

    if (!o.live) return;
    if (SLICED) {  // this slice's sums: three 16-byte records per body, [slice][body]
        float4 *row = a.partial + ((size_t)blockIdx.y * a.count + o.l) * 3u;
        row[0] = make_float4(s.cx, s.cy, s.cz, s.cnt);
        row[1] = make_float4(s.rx, s.ry, s.rz, s.vcnt);
        row[2] = make_float4(s.mx, s.my, s.mz, 0.f);
    } else {
        boids_finish(a, s, o.l, o.pn);
    }
}

// the split form's second launch: a body's rows in slice order (the same order every step: deterministic), then main.rs:506-521.
// The counts are sums of integers below 2^24: exact in binary32 whatever the order.
__global__ __launch_bounds__(kBlock) void boids_combine_kernel(BoidsArgs a, uint32_t slices)
{
    __shared__ float4 red[kBlock];
    const bool no3 = boids_no3(a);
    float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
    if (no3) {  // the total of all velocities from boids_prep_kernel's per-workgroup sums: every workgroup adds them in the same order
        const uint32_t groups = (a.n_total + 1023u) / 1024u;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (uint32_t g = threadIdx.x; g < groups; g += kBlock) {
            const float4 o = a.vtot[g];
            t.x = t.x + o.x, t.y = t.y + o.y, t.z = t.z + o.z;
        }
        red[threadIdx.x] = t;
        __syncthreads();
        for (int w = kBlock / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) {
                const float4 o = red[threadIdx.x + w];
                float4 m = red[threadIdx.x];
                m.x = m.x + o.x, m.y = m.y + o.y, m.z = m.z + o.z;
                red[threadIdx.x] = m;
            }
            __syncthreads();
        }
        tot = red[0];
    }
    const uint32_t l = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (l >= a.count) return;
    BoidsAcc s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (uint32_t k = 0; k < slices; ++k) {
        const float4 *row = a.partial + ((size_t)k * a.count + l) * 3u;
        const float4 c = row[0], r = row[1], m = row[2];
        s.cx = s.cx + c.x, s.cy = s.cy + c.y, s.cz = s.cz + c.z, s.cnt = s.cnt + c.w;
        s.rx = s.rx + r.x, s.ry = s.ry + r.y, s.rz = s.rz + r.z, s.vcnt = s.vcnt + r.w;
        s.mx = s.mx + m.x, s.my = s.my + m.y, s.mz = s.mz + m.z;
    }
    if (no3) {  // rule 3 held for every pair: all the velocities but the body's own, and n - 1 of them
        const float4 vn = a.vel_in[a.first + l];
        s.mx = tot.x - vn.x, s.my = tot.y - vn.y, s.mz = tot.z - vn.z;
        s.vcnt = (float)(a.n_total - 1u);
    }
    boids_finish(a, s, l, a.pos_in[a.first + l]);
}

// ------------------------------------------------------------------------------------------------
// Boids, chain-split form: TWO waves per 64 bodies, one folding rule 1 (centre x, y, count), the other rules 2 and 3 (repel,
// match, vcount) -- for shards of about 45 K to 90 K bodies, where one lane per body leaves a single wave on each SIMD
// (bound by its own issue rate) and the producer/consumer form has too much ring traffic.  Both waves evaluate the position
// distance (21 operations per pair in all instead of 16), each keeps the reference's order for its own sums, so the bits are
// those of boids_step_kernel.  A workgroup is 8 waves: waves 0-3 rule 1, waves 4-7 rules 2-3 of the SAME 256 bodies; the
// tiles are staged once, by all 512 threads; at the end the second half hands its sums to the first through LDS.
// ------------------------------------------------------------------------------------------------
constexpr int kSplitThreads = 2 * kBlock;

template <int TJ, bool PACKED>
__global__ __launch_bounds__(kSplitThreads) void boids_split_kernel(BoidsArgs a)
{
    static_assert(TJ % kSplitThreads == 0, "every thread stages TJ / 512 records");
    constexpr int R = TJ / kSplitThreads;
    constexpr int kW = kSplitThreads / 64;
    __shared__ float4 tile_pv[2][TJ];  // (px, py, vx, vy)
    __shared__ float2 tile_z[2][TJ];   // (pz, vz): read by 3-D tiles only
    __shared__ uint32_t tile_flags[2][kW];
    __shared__ uint32_t self_flags[kW];
    __shared__ float handoff[7][kBlock];  // rx, ry, rz, mx, my, mz, vcnt of the rules-2-3 half

    const int tid = threadIdx.x;
    const int role = __builtin_amdgcn_readfirstlane(tid >> 8);  // 0: rule 1; 1: rules 2 and 3
    const int btid = tid & (kBlock - 1);
    const BoidsOwn o = boids_own(a, (uint32_t)kBlock, (uint32_t)btid);
    if ((tid & 63) == 0) self_flags[tid >> 6] = o.self;

    BoidsStage<R> st;
    const uint32_t n = a.n_total;
    const uint32_t ntiles = (n + (uint32_t)TJ - 1u) / (uint32_t)TJ;
    boids_stage_fetch<kSplitThreads>(st, a, 0u, tid);
    boids_stage_publish<kSplitThreads>(st, a, tile_pv[0], tile_z[0], tile_flags[0], tid);
    __syncthreads();
    const uint32_t block_self = boids_or_words<kW>(self_flags);

    const BoidsMaskK mkv = boids_mask_vgprs(a);
    BoidsAcc s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int buf = 0;
    for (uint32_t t = 0; t < ntiles; ++t) {
        const bool more = (t + 1u) < ntiles;
        if (more) boids_stage_fetch<kSplitThreads>(st, a, (t + 1u) * (uint32_t)TJ, tid);
        const BoidsTileHead h = boids_tile_head<TJ, kW>(t, n, o, block_self, tile_flags[buf]);
        if (role == 0)
            BOIDS_FOLD_BY_FLAGS(PACKED, 1, s, h, tile_pv[buf], tile_z[buf], o, a, mkv);
        else
            BOIDS_FOLD_BY_FLAGS(PACKED, 2, s, h, tile_pv[buf], tile_z[buf], o, a, mkv);
        if (more) boids_stage_publish<kSplitThreads>(st, a, tile_pv[buf ^ 1], tile_z[buf ^ 1], tile_flags[buf ^ 1], tid);
        __syncthreads();
        buf ^= 1;
    }

    if (role == 1) {
        handoff[0][btid] = s.rx, handoff[1][btid] = s.ry, handoff[2][btid] = s.rz;
        handoff[3][btid] = s.mx, handoff[4][btid] = s.my, handoff[5][btid] = s.mz;
        handoff[6][btid] = s.vcnt;
    }
    __syncthreads();
    if (role == 0 && o.live) {
        s.rx = handoff[0][btid], s.ry = handoff[1][btid], s.rz = handoff[2][btid];
        s.mx = handoff[3][btid], s.my = handoff[4][btid], s.mz = handoff[5][btid];
        s.vcnt = handoff[6][btid];
        boids_finish(a, s, o.l, o.pn);
    }
}

// ------------------------------------------------------------------------------------------------
// Boids, producer/consumer form ("bpc"), for shards too small to fill the chip with one lane per body.  Boids has
// EIGHT serial chains per body (centre x/y, count, repel x/y, match x/y, vcount; three more in 3-D), so the consumer
// side is one wave per chain.  A workgroup owns 64 bodies (lane = body) and runs 16 waves:
//   waves 0..7   CONSUMERS, one running sum each (main.rs:476, 487, 499), folding the previous 64-j chunk in j order:
//                sum = fma(mask_j, src_j, sum) with the 0/1 (or 0/-1) masks the producers left in the LDS ring and
//                src_j read straight from the SoA tile (a broadcast), four j's per ds_read_b128 on both
//   waves 8..15  PRODUCERS, 8 consecutive j's each per chunk: squared distances and the three radius tests
//                (main.rs:474-475, 485-486, 497-498), written as masks m1, m2 (-1/0), m3 to ring[parity][plane][body][j]
// Only masks cross the ring (3 planes, 54 KB), one barrier per chunk, tiles of 8 chunks staged as SoA planes
// (px, py, pz, vx, vy, vz) one tile ahead by the producers.  Same arithmetic as boids_pair: same bits.
// (Chunks are 64 j's, 8 per producer: the masks travel as binary16, see BpcRing.)
// Per-tile forms as in boids_step_kernel: the self test only in the tile holding the workgroup's bodies, select-on-
// result instead of the masked FMA when a record is not finite, z chains only when some z is non-zero.
// ------------------------------------------------------------------------------------------------
constexpr int kBpcConsumers = 8;
constexpr int kBpcProducers = 8;
constexpr int kBpcThreads = (kBpcConsumers + kBpcProducers) * 64;
constexpr int kBpcPer = 8;                          // consecutive j's per producer per chunk (16, i.e. 128 j's per barrier: 1.38 against 1.35 ms on a 16 384-body shard, 2.77 against 2.10 on 32 768 where it leaves room for one workgroup per CU only)
constexpr int kBpcChunk = kBpcProducers * kBpcPer;  // 64
typedef _Float16 BpcMask;  // (binary32 masks, i.e. twice the LDS traffic of the ring: 1.91 against 1.35 ms on a 16 384-body shard -- the ring is what this form is bound by)
constexpr int kBpcStride = kBpcChunk + 8;           // masks per body row: rows stay 16-B aligned and spread over the banks
constexpr int kBpcTile = 512;
constexpr int kBpcChunksPerTile = kBpcTile / kBpcChunk;  // 8

// The masks are 0, 1 or -1: exact in binary16, and v_fma_mix_f32 takes a binary16 multiplicand straight into an fp32 FMA,
// so half-width masks cost the consumers nothing and let a chunk (one barrier) cover 64 j's in the same 54 KB of LDS.
struct BpcRing {
    BpcMask m[3][64][kBpcStride];  // masks of rule 1, 2 (negated), 3: [plane][body][j within chunk]
};
typedef BpcMask half8 __attribute__((ext_vector_type(8)));
struct BpcTile {
    float c[6][kBpcTile];  // px, py, pz, vx, vy, vz
};
enum BpcSrc { kSrcPx = 0, kSrcPy = 1, kSrcPz = 2, kSrcVx = 3, kSrcVy = 4, kSrcVz = 5, kSrcDx = 6, kSrcDy = 7, kSrcDz = 8, kSrcOne = 9 };

// the three masks of 8 consecutive j's for this lane's body
template <bool SELF, bool PLANAR, bool ALL3>
__device__ __forceinline__ void bpc_produce(const BpcTile &t, int jt, uint32_t jglobal, uint32_t gn, const float4 pn, const float4 vn,
                                            float r1, float t2, float t3, BpcRing &ring, int j0, int lane)
{
    // four j's at a time: what is live at once is one float4 per plane, not two (the kernel's register count is the maximum
    // over its roles and forms, and this 3-D / rule-3-tested producer used to set it)
    half8 m1[kBpcPer / 8], m2[kBpcPer / 8], m3[kBpcPer / 8];
#pragma unroll
    for (int q = 0; q < kBpcPer / 4; ++q) {
        const float4 px = *reinterpret_cast<const float4 *>(&t.c[kSrcPx][jt + 4 * q]);
        const float4 py = *reinterpret_cast<const float4 *>(&t.c[kSrcPy][jt + 4 * q]);
        float4 pz = make_float4(0.f, 0.f, 0.f, 0.f), vz = pz, vx = pz, vy = pz;
        if (!ALL3) {
            vx = *reinterpret_cast<const float4 *>(&t.c[kSrcVx][jt + 4 * q]);
            vy = *reinterpret_cast<const float4 *>(&t.c[kSrcVy][jt + 4 * q]);
        }
        if (!PLANAR) {
            pz = *reinterpret_cast<const float4 *>(&t.c[kSrcPz][jt + 4 * q]);
            if (!ALL3) vz = *reinterpret_cast<const float4 *>(&t.c[kSrcVz][jt + 4 * q]);
        }
        const float pxs[4] = {px.x, px.y, px.z, px.w}, pys[4] = {py.x, py.y, py.z, py.w}, pzs[4] = {pz.x, pz.y, pz.z, pz.w};
        const float vxs[4] = {vx.x, vx.y, vx.z, vx.w}, vys[4] = {vy.x, vy.y, vy.z, vy.w}, vzs[4] = {vz.x, vz.y, vz.z, vz.w};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int u = 4 * q + w;
            const bool ne = SELF ? (jglobal + (uint32_t)u != gn) : true;          // main.rs:475 n != i
            const float dx = pxs[w] - pn.x, dy = pys[w] - pn.y;
            float d2 = (dx * dx) + (dy * dy);
            if (!PLANAR) {
                const float dz = pzs[w] - pn.z;
                d2 = d2 + (dz * dz);
            }
            // (the one-instruction masks of the one-lane kernels, boids_below, were tried here too: 1.347 -> 1.329 ms on a
            // 16 384-body shard, 2.11 -> 2.17 on 32 768 -- the producers are not what bounds this form; not kept)
            m1[u / 8][u % 8] = ((d2 < r1) && ne) ? (BpcMask)1.0f : (BpcMask)0.0f;    // main.rs:474-475
            m2[u / 8][u % 8] = ((d2 <= t2) && ne) ? (BpcMask)-1.0f : (BpcMask)0.0f;  // main.rs:485-486 (negated: repel SUBTRACTS)
            if (!ALL3) {  // ALL3: the rule-3 test holds for every pair of the tile; its consumers add without a mask
                const float ex = vxs[w] - vn.x, ey = vys[w] - vn.y;
                float e2 = (ex * ex) + (ey * ey);
                if (!PLANAR) {
                    const float ez = vzs[w] - vn.z;
                    e2 = e2 + (ez * ez);
                }
                m3[u / 8][u % 8] = ((e2 <= t3) && ne) ? (BpcMask)1.0f : (BpcMask)0.0f;  // main.rs:497-498
            }
        }
        if (q + 1 < kBpcPer / 4) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int h = 0; h < kBpcPer / 8; ++h) {
        *reinterpret_cast<half8 *>(&ring.m[0][lane][j0 + 8 * h]) = m1[h];
        *reinterpret_cast<half8 *>(&ring.m[1][lane][j0 + 8 * h]) = m2[h];
        if (!ALL3) *reinterpret_cast<half8 *>(&ring.m[2][lane][j0 + 8 * h]) = m3[h];
    }
}

// One chain over one chunk: sum = sum (+) mask_j * src_j for j = 0..nvalid-1 in order.  MASKED: fma form (finite data);
// else select-on-result.  src: a tile plane, a difference to the own coordinate (repel), or the constant 1 (counts).
// 16 j's per trip: two 16-byte mask reads (8 halfs each) and four 16-byte source reads.
// ONES: every mask of the chunk is known to be 1 (rule 3 on an ALL3 tile): plain adds, no mask reads; a count grows by nvalid.
template <int SRC, bool MASKED, bool ONES = false>
__device__ __forceinline__ void bpc_chain(const BpcMask (*mrow)[kBpcStride], const BpcTile &t, int jt, float own, int lane, int nvalid,
                                          float &sum)
{
    constexpr int plane = SRC == kSrcOne ? 0 : SRC >= kSrcDx ? SRC - kSrcDx : SRC;
    if (ONES) {
        static_assert(!ONES || SRC < kSrcDx || SRC == kSrcOne, "rule-3 chains read a plane or count");
        if (SRC == kSrcOne) {
            sum = sum + (float)nvalid;  // nvalid ones: integers below 2^24, exact either way
            return;
        }
#pragma unroll 1
        for (int h = 0; h < kBpcChunk / 16; ++h) {
            float4 sv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) sv[g] = *reinterpret_cast<const float4 *>(&t.c[plane][jt + 16 * h + 4 * g]);
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                if (16 * h + u >= nvalid) continue;
                const float4 v4 = sv[u / 4];
                sum = sum + ((u % 4) == 0 ? v4.x : (u % 4) == 1 ? v4.y : (u % 4) == 2 ? v4.z : v4.w);  // main.rs:499
            }
        }
        return;
    }
#pragma unroll 1
    for (int h = 0; h < kBpcChunk / 16; ++h) {
        half8 mk[2];
        float4 sv[4];
#pragma unroll
        for (int g = 0; g < 2; ++g) mk[g] = *reinterpret_cast<const half8 *>(&mrow[lane][16 * h + 8 * g]);
#pragma unroll
        for (int g = 0; g < 4; ++g)
            sv[g] = SRC != kSrcOne ? *reinterpret_cast<const float4 *>(&t.c[plane][jt + 16 * h + 4 * g]) : make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if (16 * h + u >= nvalid) continue;  // uniform; only the last chunk of the set is short
            const BpcMask mh = mk[u / 8][u % 8];
            const float4 v4 = sv[u / 4];
            float x = (u % 4) == 0 ? v4.x : (u % 4) == 1 ? v4.y : (u % 4) == 2 ? v4.z : v4.w;
            if (SRC >= kSrcDx && SRC <= kSrcDz) x = x - own;  // p_i - p_n
            if (MASKED) {
                sum = SRC == kSrcOne ? sum + (float)mh : __builtin_fmaf((float)mh, x, sum);
            } else {  // select on the result: a skipped term leaves the sum untouched whatever x is
                const float cand = (SRC >= kSrcDx && SRC <= kSrcDz) ? sum - x : sum + x;
                sum = (mh != (BpcMask)0.0f) ? cand : sum;
            }
        }
    }
}

// the chain(s) of consumer wave ROLE: sum_a always, sum_b a z chain in 3-D for roles 2, 3, 7
template <int ROLE, bool MASKED, bool PLANAR, bool ALL3>
__device__ __forceinline__ void bpc_fold(const BpcRing &rg, const BpcTile &tl, int jt, const float4 pn, int lane, int nvalid, float &sum_a,
                                         float &sum_b)
{
    if (ROLE == 0) bpc_chain<kSrcPx, MASKED>(rg.m[0], tl, jt, 0.f, lane, nvalid, sum_a);                     // centre x
    if (ROLE == 1) bpc_chain<kSrcPy, MASKED>(rg.m[0], tl, jt, 0.f, lane, nvalid, sum_a);                     // centre y
    if (ROLE == 2) {
        bpc_chain<kSrcOne, MASKED>(rg.m[0], tl, jt, 0.f, lane, nvalid, sum_a);                               // count
        if (!PLANAR) bpc_chain<kSrcPz, MASKED>(rg.m[0], tl, jt, 0.f, lane, nvalid, sum_b);                   // centre z
    }
    if (ROLE == 3) {
        bpc_chain<kSrcDx, MASKED>(rg.m[1], tl, jt, pn.x, lane, nvalid, sum_a);                               // repel x
        if (!PLANAR) bpc_chain<kSrcDz, MASKED>(rg.m[1], tl, jt, pn.z, lane, nvalid, sum_b);                  // repel z
    }
    if (ROLE == 4) bpc_chain<kSrcDy, MASKED>(rg.m[1], tl, jt, pn.y, lane, nvalid, sum_a);                    // repel y
    if (ROLE == 5) bpc_chain<kSrcVx, MASKED, ALL3>(rg.m[2], tl, jt, 0.f, lane, nvalid, sum_a);               // match x
    if (ROLE == 6) bpc_chain<kSrcVy, MASKED, ALL3>(rg.m[2], tl, jt, 0.f, lane, nvalid, sum_a);               // match y
    if (ROLE == 7) {
        bpc_chain<kSrcOne, MASKED, ALL3>(rg.m[2], tl, jt, 0.f, lane, nvalid, sum_a);                         // vcount
        if (!PLANAR) bpc_chain<kSrcVz, MASKED, ALL3>(rg.m[2], tl, jt, 0.f, lane, nvalid, sum_b);             // match z
    }
}

// form (masked FMA / select, planar / 3-D) chosen once per call, outside the chunk loop
template <int ROLE>
__device__ __forceinline__ void bpc_fold_flags(uint32_t flags, const BpcRing &rg, const BpcTile &tl, int jt, const float4 pn, int lane,
                                               int nvalid, float &sum_a, float &sum_b)
{
    const bool masked = (flags & kBoidsNonFinite) == 0u, planar = (flags & kBoidsNonPlanar) == 0u;
    const bool all3 = ROLE >= 5 && boids_all3(flags);  // only the rule-3 chains have a form of their own for it
    if (masked && planar && all3)
        bpc_fold<ROLE, true, true, true>(rg, tl, jt, pn, lane, nvalid, sum_a, sum_b);
    else if (masked && all3)
        bpc_fold<ROLE, true, false, true>(rg, tl, jt, pn, lane, nvalid, sum_a, sum_b);
    else if (masked && planar)
        bpc_fold<ROLE, true, true, false>(rg, tl, jt, pn, lane, nvalid, sum_a, sum_b);
    else if (masked)
        bpc_fold<ROLE, true, false, false>(rg, tl, jt, pn, lane, nvalid, sum_a, sum_b);
    else
        bpc_fold<ROLE, false, false, false>(rg, tl, jt, pn, lane, nvalid, sum_a, sum_b);
}

__device__ __forceinline__ void boids_pc_body(const BoidsArgs &a)
{
    __shared__ __attribute__((aligned(16))) BpcTile tile[2];
    __shared__ __attribute__((aligned(16))) BpcRing ring[2];
    __shared__ uint32_t tile_flags[2][8];
    // the 11 final sums per body are handed to wave 0 through ring[0]'s storage once every fold is done (keeps the
    // workgroup under 80 KiB of LDS, i.e. two workgroups per CU)
    float(*sums)[64] = reinterpret_cast<float(*)[64]>(&ring[0]);

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const BoidsOwn o = boids_own(a, 64u, (uint32_t)lane);  // the same 64 bodies in every wave

    const uint32_t n = a.n_total;
    const uint32_t ntiles = (n + (uint32_t)kBpcTile - 1u) / (uint32_t)kBpcTile;
    // loaders: the 512 threads of the producer waves stage one position and one velocity record each
    const int ltid = tid - kBpcConsumers * 64;
    const bool loader = ltid >= 0;
    struct Staged {
        float4 p, v;
    };
    auto fetch = [&](uint32_t t) -> Staged {
        Staged r = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
        const uint32_t j = t * (uint32_t)kBpcTile + (uint32_t)(loader ? ltid : 0);
        if (loader && j < n) {
            r.p = a.pos_in[j];
            r.v = a.vel_in[j];
        }
        return r;
    };
    auto publish = [&](int buf, Staged rec) {
        // keep the flag arithmetic (pure, on prefetched data) at the use point instead of right behind the loads
        asm volatile("" : "+v"(rec.p.x), "+v"(rec.p.y), "+v"(rec.p.z), "+v"(rec.p.w), "+v"(rec.v.x), "+v"(rec.v.y), "+v"(rec.v.z), "+v"(rec.v.w));
        if (loader) {
            tile[buf].c[kSrcPx][ltid] = rec.p.x;
            tile[buf].c[kSrcPy][ltid] = rec.p.y;
            tile[buf].c[kSrcPz][ltid] = rec.p.z;
            tile[buf].c[kSrcVx][ltid] = rec.v.x;
            tile[buf].c[kSrcVy][ltid] = rec.v.y;
            tile[buf].c[kSrcVz][ltid] = rec.v.z;
            const uint32_t f = boids_wave_flags(boids_flags(rec.p, rec.v, a.vlim_bits));
            if (lane == 0) tile_flags[buf][wave - kBpcConsumers] = f;
        }
    };
    publish(0, fetch(0u));
    __syncthreads();

    // per-tile bookkeeping shared by both roles (all wave-uniform)
    struct TileInfo {
        int tb, nk;
        bool stage, has_self;
        uint32_t flags, j_first;
    };
    auto tile_info = [&](uint32_t t) {
        TileInfo ti;
        ti.tb = (int)(t & 1u);
        ti.stage = t + 1u < ntiles;
        const BoidsTileHead h = boids_tile_head<kBpcTile, 8>(t, n, o, o.self, tile_flags[ti.tb]);
        ti.flags = __builtin_amdgcn_readfirstlane(h.flags);
        ti.j_first = h.j0;
        ti.nk = (h.nj + kBpcChunk - 1) / kBpcChunk;
        ti.has_self = h.has_self;
        if (ti.has_self) ti.flags |= kBoidsSelfTile;
        return ti;
    };

    // ---- consumer waves: the whole step for one role, forms chosen per tile ------------------------------
    auto consumer = [&](auto role_tag) {
        constexpr int ROLE = decltype(role_tag)::value;
        float sum_a = 0.f, sum_b = 0.f;
        uint32_t prev_flags = 0u;
        int last_nk = 1;
        for (uint32_t t = 0; t < ntiles; ++t) {
            const TileInfo ti = tile_info(t);
            last_nk = ti.nk;
            const bool first_tile = t == 0u;
            auto nothing = [] {};
            // at step k fold chunk k-1; step 0: the previous tile's last chunk (tile buffer tb^1, ring parity 1)
            pc_steps(ti.nk, [&](int k, int par) {
                if (k == 0) {
                    if (!first_tile)
                        bpc_fold_flags<ROLE>(prev_flags, ring[par ^ 1], tile[ti.tb ^ 1], (kBpcChunksPerTile - 1) * kBpcChunk, o.pn, lane,
                                             kBpcChunk, sum_a, sum_b);
                } else {
                    bpc_fold_flags<ROLE>(ti.flags, ring[par ^ 1], tile[ti.tb], (k - 1) * kBpcChunk, o.pn, lane, kBpcChunk, sum_a, sum_b);
                }
            }, nothing);
            prev_flags = ti.flags;
        }
        // drain: the last chunk of the step (its tile buffer and ring slot are still intact)
        const int tb = (int)((ntiles - 1u) & 1u), k = last_nk - 1;
        const uint32_t first_j = (ntiles - 1u) * (uint32_t)kBpcTile + (uint32_t)k * (uint32_t)kBpcChunk;
        bpc_fold_flags<ROLE>(prev_flags, ring[k & 1], tile[tb], k * kBpcChunk, o.pn, lane, (int)(n - first_j), sum_a, sum_b);
        __syncthreads();  // every consumer is done with the ring: its storage now carries the sums (producers match this barrier)
        sums[ROLE][lane] = sum_a;
        if (ROLE == 2) sums[8][lane] = sum_b;   // centre z
        if (ROLE == 3) sums[9][lane] = sum_b;   // repel z
        if (ROLE == 7) sums[10][lane] = sum_b;  // match z
    };

    // ---- producer waves ------------------------------------------------------------------------------------
    auto producer = [&]() {
        const int j0 = (wave - kBpcConsumers) * kBpcPer;
        for (uint32_t t = 0; t < ntiles; ++t) {
            const TileInfo ti = tile_info(t);
            Staged rec = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
            if (ti.stage) rec = fetch(t + 1u);  // in flight across the chunks of this tile
            auto stage_next = [&]() {
                if (ti.stage) publish(ti.tb ^ 1, rec);  // tile t+1 goes to the buffer tile t-1 used
            };
            const bool planar = (ti.flags & kBoidsNonPlanar) == 0u;
            auto run = [&](auto self_tag, auto planar_tag, auto all3_tag) {
                pc_steps(ti.nk, [&](int k, int par) {
                    const int jt = k * kBpcChunk + j0;
                    bpc_produce<decltype(self_tag)::value, decltype(planar_tag)::value, decltype(all3_tag)::value>(
                        tile[ti.tb], jt, ti.j_first + (uint32_t)jt, o.gn, o.pn, o.vn, a.r1, a.t2, a.t3, ring[par], j0, lane);
                }, stage_next);
            };
            using T = std::true_type;
            using F = std::false_type;
            if (ti.has_self) {
                if (planar) run(T{}, T{}, F{}); else run(T{}, F{}, F{});
            } else if (boids_all3(ti.flags)) {  // the consumers of this tile's rule-3 chains decide the same way (bpc_fold_flags)
                if (planar) run(F{}, T{}, T{}); else run(F{}, F{}, T{});
            } else {
                if (planar) run(F{}, T{}, F{}); else run(F{}, F{}, F{});
            }
        }
        __syncthreads();  // matches the consumers' barrier in front of the sums hand-off
    };

    switch (wave) {
        case 0: consumer(std::integral_constant<int, 0>{}); break;
        case 1: consumer(std::integral_constant<int, 1>{}); break;
        case 2: consumer(std::integral_constant<int, 2>{}); break;
        case 3: consumer(std::integral_constant<int, 3>{}); break;
        case 4: consumer(std::integral_constant<int, 4>{}); break;
        case 5: consumer(std::integral_constant<int, 5>{}); break;
        case 6: consumer(std::integral_constant<int, 6>{}); break;
        case 7: consumer(std::integral_constant<int, 7>{}); break;
        default: producer(); break;
    }
    __syncthreads();
    if (wave == 0 && o.live) {
        const BoidsAcc s = {sums[0][lane], sums[1][lane], sums[8][lane],    // centre x, y, z
                            sums[3][lane], sums[4][lane], sums[9][lane],    // repel
                            sums[5][lane], sums[6][lane], sums[10][lane],   // match
                            sums[2][lane], sums[7][lane]};                  // count, vcount
        boids_finish(a, s, o.l, o.pn);
    }
}

// Two builds of the one body.  Left alone the allocator takes 65 registers: 7 waves per SIMD, i.e. ONE 16-wave workgroup per CU --
// right for launches of up to 256 workgroups (16 384 bodies), which have one per CU anyway.  Larger launches take the build
// held to 64 registers (8 waves per SIMD, two workgroups per CU: one folds while the other waits at its chunk barrier; 9
// registers spilled): 32 768 bodies 2.73 -> 2.13 ms, 65 536: 5.39 -> 4.15; 16 384: 1.43 -> 1.49 when forced, hence two builds.
__global__ __launch_bounds__(kBpcThreads) void boids_pc_kernel(BoidsArgs a) { boids_pc_body(a); }
__global__ __launch_bounds__(kBpcThreads) __attribute__((amdgpu_waves_per_eu(8))) void boids_pc_kernel_occ8(BoidsArgs a) { boids_pc_body(a); }

hipError_t launch_boids_pc(const BoidsArgs &a, hipStream_t s)
{
    const uint32_t blocks = ceil_div_u(a.count, 64);
    if (blocks > 256u)
        hipLaunchKernelGGL(boids_pc_kernel_occ8, dim3(blocks), dim3(kBpcThreads), 0, s, a);
    else
        hipLaunchKernelGGL(boids_pc_kernel, dim3(blocks), dim3(kBpcThreads), 0, s, a);
    return hipGetLastError();
}

// one launch of KERNEL<tile, packed, ...> on `grid` x `block`; every instantiation the unit holds is named below
#define BOIDS_LAUNCH(KERNEL, ...) hipLaunchKernelGGL((KERNEL<__VA_ARGS__>), grid, block, 0, s, a)
#define BOIDS_LAUNCH_PACKED(KERNEL, TJ)                      \
    do {                                                     \
        if (packed) BOIDS_LAUNCH(KERNEL, TJ, true);          \
        else BOIDS_LAUNCH(KERNEL, TJ, false);                \
    } while (0)

// the split form: `slices` slices of a.j_chunk records (a multiple of the tile) x count / 256 workgroups, then the combine
hipError_t launch_boids_split(const BoidsArgs &a, uint32_t tile, uint32_t slices, hipStream_t s)
{
    const dim3 grid(ceil_div_u(a.count, kBlock), slices), block(kBlock);
    if (a.gflags) {  // the step's global flags and the total of the velocities (rule 3 out of the slices' loops where it always holds)
        hipError_t e = hipMemsetAsync(a.gflags, 0, sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(boids_prep_kernel, dim3(ceil_div_u(a.n_total, 1024u)), block, 0, s, a);
    }
    switch (tile) {
        case 256: BOIDS_LAUNCH(boids_step_kernel, 256, false, true); break;
        case 512: BOIDS_LAUNCH(boids_step_kernel, 512, false, true); break;
        case 1024: BOIDS_LAUNCH(boids_step_kernel, 1024, false, true); break;
        default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(boids_combine_kernel, dim3(ceil_div_u(a.count, kBlock)), block, 0, s, a, slices);
    return hipGetLastError();
}

hipError_t launch_boids(const BoidsArgs &a, uint32_t tile, uint32_t form, hipStream_t s)
{
    if (form == 1) return launch_boids_pc(a, s);
    const dim3 grid(ceil_div_u(a.count, kBlock));
    if (form == 3 || form == 4) {  // chain split: 512 threads stage a tile, so tiles of 512 or 1024 records
        const dim3 block(kSplitThreads);
        const bool packed = form == 4;
        if (tile == 512) BOIDS_LAUNCH_PACKED(boids_split_kernel, 512);
        else BOIDS_LAUNCH_PACKED(boids_split_kernel, 1024);
        return hipGetLastError();
    }
    const dim3 block(kBlock);
    const bool packed = form == 2;
    switch (tile) {
        case 256: BOIDS_LAUNCH_PACKED(boids_step_kernel, 256); break;
        case 512: BOIDS_LAUNCH_PACKED(boids_step_kernel, 512); break;
        case 1024: BOIDS_LAUNCH_PACKED(boids_step_kernel, 1024); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
#undef BOIDS_LAUNCH_PACKED
#undef BOIDS_LAUNCH
