// nb_launch.inc -- host-side launchers (grid shapes, template dispatch).
// Included by nb_kernels.hip inside namespace nbk; see that file for the compilation scheme.
//
// The forms that read x / y / z planes (block chain, scalar loads, pairs, ring) lay them into the caller's scratch.  That layout
// is stated ONCE: plane_scratch() makes the view (PlaneScratch, nb_kernels.h) and strict_bc_scratch_bytes() gives its size from
// the same constants; next_plane_generation() stamps a launch's flag words, launch_fast_planes() is FAST's planes launch.  No
// launcher below computes a scratch offset of its own (the ring phases' flag sub-sets, flags + kRingFlags*, are theirs).

// ------------------------------------------------------------------------------------------------
// host-side launchers
// ------------------------------------------------------------------------------------------------
static inline uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }

template <int TJ, int U, int S>
static hipError_t launch_strict_t(const StepArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL((step_strict_kernel<TJ, U, S>), dim3(ceil_div(a.count, kBlock / S)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

#define NBK_CASE(T, U_, S_) \
    if (tile == T && unroll == U_ && lanes == S_) return launch_strict_t<T, U_, S_>(a, s)

#ifdef NBK_NOSLP_TU
// This translation unit is the same source compiled with -DNBK_NOSLP_TU -fno-slp-vectorize: it holds only the
// j-parallel STRICT shapes (S > 1).  Without SLP the x/y running-sum adds stay scalar v_add_f32, so the row_shl DPP
// fetch folds into them (v_add_f32_dpp); packed v_pk_add_f32 cannot take a DPP operand and would need a mov per term.
hipError_t launch_strict_jp(const StepArgs &a, uint32_t tile, uint32_t unroll, uint32_t lanes, hipStream_t s)
{
    // unroll counts groups of S pairs in flight.  What make_plan reaches by itself: sets below 1 536 bodies, sixteen lanes per body
    // (tile 1024, or 256 when params.tile names it); the other shapes are measurement history (NB_STRICT_LANES / NB_STRICT_UNROLL)
    // and live in the NB_LEGACY_FORMS build only (make legacy: what the test suite's form tests load)
    NBK_CASE(256, 2, 16);
    NBK_CASE(1024, 2, 16);
#ifdef NB_LEGACY_FORMS
    NBK_CASE(256, 4, 2);
    NBK_CASE(256, 2, 2);
    NBK_CASE(256, 4, 4);
    NBK_CASE(256, 2, 4);
    NBK_CASE(256, 4, 8);
    NBK_CASE(256, 2, 8);
    NBK_CASE(256, 4, 16);
    NBK_CASE(1024, 4, 2);
    NBK_CASE(1024, 4, 4);
    NBK_CASE(1024, 4, 8);
    NBK_CASE(1024, 2, 8);
#endif
    return hipErrorNotSupported;
}

#else
hipError_t launch_strict_pc(const StepArgs &a, uint32_t producers, hipStream_t s)
{
#ifdef NB_LEGACY_FORMS   // the producer/consumer form: no shape takes it by itself since the block chain (NB_STRICT_PC)
    if (producers == 8)
        hipLaunchKernelGGL(step_strict_pc_kernel<8>, dim3(ceil_div(a.count, 64)), dim3(PcShape<8>::kThreads), 0, s, a);
    else if (producers == 14)
        hipLaunchKernelGGL(step_strict_pc_kernel<14>, dim3(ceil_div(a.count, 64)), dim3(PcShape<14>::kThreads), 0, s, a);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
#else
    return hipErrorNotSupported;
#endif
}

// The planes area: flags + three zero-padded planes + one request's worth of slack (the scalar-load kernel requests one group past
// the last full one).  Its size and the view into it are made from the same three terms.
constexpr size_t kPlaneSlackBytes = 64;
size_t strict_bc_scratch_bytes(uint32_t n_total) { return (size_t)kBcFlagsBytes + 3u * (size_t)bc_padded(n_total) * sizeof(float) + kPlaneSlackBytes; }

PlaneScratch plane_scratch(void *scratch, uint32_t n_total)
{
    PlaneScratch v;
    v.npad = bc_padded(n_total);
    v.flags = (uint32_t *)scratch;
    v.px = (float *)((char *)scratch + kBcFlagsBytes);
    v.py = v.px + v.npad;
    v.pz = v.py + v.npad;
    v.behind = (char *)scratch + strict_bc_scratch_bytes(n_total);  // = the end of pz + the slack
    return v;
}

// The flag words are stamped with a generation number instead of being cleared (nb_nbody_bc.inc); 0 is what zeroed scratch holds,
// so no launch is ever given it.
static std::atomic<uint32_t> g_bc_generation{0};
static uint32_t next_plane_generation()
{
    uint32_t gen = g_bc_generation.fetch_add(1u, std::memory_order_relaxed) + 1u;
    if (gen == 0u) gen = g_bc_generation.fetch_add(1u, std::memory_order_relaxed) + 1u;
    return gen;
}

// flags + planes of the whole set from the records; [lo_bits, hi_bits]: the magnitudes that leave the "IEEE" flag word clear
static void enqueue_planes(const StepArgs &a, const PlaneScratch &v, uint32_t lo_bits, uint32_t hi_bits, uint32_t gen, hipStream_t s)
{
    hipLaunchKernelGGL(planes_kernel, dim3(ceil_div(v.npad, kBlock)), dim3(kBlock), 0, s, a.n_total, v.npad, a.pos_in, v.px, v.py, v.pz,
                       v.flags, lo_bits, hi_bits, 0u, gen);
}
// FAST's: "IEEE" = a coordinate of 2^28 or more (no shared reciprocal)
constexpr uint32_t kFastPlaneLoBits = 0u, kFastPlaneHiBits = 0x4d7fffffu;
static hipError_t launch_fast_planes(const StepArgs &a, const PlaneScratch &v, uint32_t gen, hipStream_t s)
{
    enqueue_planes(a, v, kFastPlaneLoBits, kFastPlaneHiBits, gen, s);
    return hipGetLastError();
}

// block-chain form: flags + planes from the records (scratch: strict_bc_scratch_bytes), then the step: two launches.
hipError_t launch_strict_bc(const StepArgs &a, void *scratch, uint32_t *status, hipStream_t s)
{
    const PlaneScratch v = plane_scratch(scratch, a.n_total);
    const uint32_t gen = next_plane_generation();
    enqueue_planes(a, v, a.lo_bits, a.hi_bits, gen, s);
    hipLaunchKernelGGL(step_strict_bc_kernel, dim3(ceil_div(a.count, 64)), dim3(kBcThreads), 0, s, a, (const uint32_t *)v.flags, gen,
                       (const float *)v.px, (const float *)v.py, (const float *)v.pz, status);
    return hipGetLastError();
}

// scalar-load form: flags + planes (as for the block chain), then one wave per 64 bodies
hipError_t launch_strict_sl(const StepArgs &a, uint32_t shape, void *scratch, hipStream_t s)
{
    const PlaneScratch v = plane_scratch(scratch, a.n_total);
    const uint32_t gen = next_plane_generation();
    enqueue_planes(a, v, a.lo_bits, a.hi_bits, gen, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_strict_sl_kernel(a, shape, v.flags, gen, v.px, v.py, v.pz, s);
}

hipError_t launch_strict(const StepArgs &a, uint32_t tile, uint32_t unroll, uint32_t lanes, hipStream_t s)
{
    if (lanes > 1) return launch_strict_jp(a, tile, unroll, lanes, s);
    NBK_CASE(256, 8, 1);   // (params.tile names the LDS-tiled kernel; its unroll of 8 is the plan's)
    NBK_CASE(512, 8, 1);
    NBK_CASE(1024, 8, 1);
#ifdef NB_LEGACY_FORMS    // NB_STRICT_UNROLL
    NBK_CASE(256, 4, 1);
    NBK_CASE(512, 4, 1);
    NBK_CASE(1024, 4, 1);
    NBK_CASE(1024, 16, 1);
#endif
    return hipErrorNotSupported;
}
#endif
#undef NBK_CASE

#ifndef NBK_NOSLP_TU
hipError_t launch_integrate_partials(const StepArgs &a, uint32_t rows, hipStream_t s)
{
    hipLaunchKernelGGL(integrate_partials_kernel, dim3(ceil_div(a.count, kBlock)), dim3(kBlock), 0, s, a, rows);
    return hipGetLastError();
}

template <int TJ, int IB, int G>
static hipError_t launch_fast_t(const StepArgs &a, uint32_t slices, hipStream_t s)
{
    hipLaunchKernelGGL((step_fast_kernel<TJ, IB, G>), dim3(ceil_div(a.count, kBlock * IB), slices), dim3(kBlock * G), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || slices == 1 || a.always_partial) return e;
    return launch_integrate_partials(a, slices, s);
}

// tile: 256 / 512 / 1024 records; ib: bodies per lane; groups: 256-lane groups per workgroup folding different j chunks
// (1, 2 or 4; with 4 groups a tile of 1024 records would need 128 KB of LDS: not built); slices: grid.y
hipError_t launch_fast(const StepArgs &a, uint32_t tile, uint32_t ib, uint32_t groups, uint32_t slices, hipStream_t s)
{
#ifndef NB_LEGACY_FORMS   // the workgroup-tile form of round 1 (NB_FAST_WAVES=0): no shape takes it by itself
    return hipErrorNotSupported;
#else
#define NBK_CASE(T, I, G_) \
    if (tile == T && ib == I && groups == G_) return launch_fast_t<T, I, G_>(a, slices, s)
    NBK_CASE(256, 1, 1);
    NBK_CASE(256, 2, 1);
    NBK_CASE(256, 4, 1);
    NBK_CASE(512, 1, 1);
    NBK_CASE(512, 2, 1);
    NBK_CASE(512, 4, 1);
    NBK_CASE(1024, 1, 1);
    NBK_CASE(1024, 2, 1);
    NBK_CASE(1024, 4, 1);
    NBK_CASE(256, 1, 2);
    NBK_CASE(256, 2, 2);
    NBK_CASE(256, 4, 2);
    NBK_CASE(512, 1, 2);
    NBK_CASE(512, 2, 2);
    NBK_CASE(512, 4, 2);
    NBK_CASE(256, 1, 4);
    NBK_CASE(256, 2, 4);
    NBK_CASE(256, 4, 4);
    NBK_CASE(512, 1, 4);
    NBK_CASE(512, 2, 4);
    NBK_CASE(512, 4, 4);
#undef NBK_CASE
    return hipErrorInvalidValue;
#endif
}

template <int TJ, int IB, int W>
static hipError_t launch_fast_wave_t(const StepArgs &a, uint32_t slices, hipStream_t s)
{
    hipLaunchKernelGGL((step_fast_wave_kernel<TJ, IB, W>), dim3(ceil_div(a.count, 64 * IB), slices), dim3(64 * W), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || slices == 1 || a.always_partial) return e;
    return launch_integrate_partials(a, slices, s);
}

// the barrier-free form: `waves` waves per workgroup share 64*ib bodies and fold one j chunk each
hipError_t launch_fast_wave(const StepArgs &a, uint32_t tile, uint32_t ib, uint32_t waves, uint32_t slices, hipStream_t s)
{
#define NBK_CASE(T, I, W_) \
    if (tile == T && ib == I && waves == W_) return launch_fast_wave_t<T, I, W_>(a, slices, s)
    NBK_CASE(256, 1, 8);   // eight waves per workgroup: the plan's (bodies per lane by launch size, the tile by params.tile)
    NBK_CASE(256, 2, 8);
    NBK_CASE(256, 4, 8);
    NBK_CASE(512, 2, 8);
    NBK_CASE(512, 4, 8);
#ifdef NB_LEGACY_FORMS    // NB_FAST_WAVES = 1, 4, 16
    NBK_CASE(256, 1, 1);
    NBK_CASE(256, 1, 4);
    NBK_CASE(256, 1, 16);
    NBK_CASE(256, 2, 1);
    NBK_CASE(256, 2, 4);
    NBK_CASE(256, 2, 16);
    NBK_CASE(256, 4, 1);
    NBK_CASE(256, 4, 4);
    NBK_CASE(256, 4, 16);
    NBK_CASE(512, 2, 4);
    NBK_CASE(512, 2, 16);
    NBK_CASE(512, 4, 4);
    NBK_CASE(512, 4, 16);
#endif
#undef NBK_CASE
    return hipErrorNotSupported;
}

// FAST through scalar loads: planes + flags ("IEEE" = a coordinate of 2^28 or more: no shared reciprocal), the fold, and --
// after a split over grid.y -- the fixed-order combine
hipError_t launch_fast_sl(const StepArgs &a_in, uint32_t ib, uint32_t slices, void *scratch, hipStream_t s)
{
    StepArgs a = a_in;
    const PlaneScratch v = plane_scratch(scratch, a.n_total);
    a.partial = (float4 *)v.behind;
    const uint32_t gen = next_plane_generation();
    hipError_t e = launch_fast_planes(a, v, gen, s);
    if (e != hipSuccess) return e;
    e = launch_fast_sl_kernel(a, ib, slices, v.flags, gen, v.px, v.py, v.pz, s);
    if (e != hipSuccess || slices == 1 || a.always_partial) return e;
    return launch_integrate_partials(a, slices, s);
}

// One phase of a FAST step in two phases through scalar loads (StepArgs::j_base / hole_lo / hole_len / partial_row0 name the phase's
// records and rows; always_partial is set).  `range`: the first phase -- only the records [r0, r1) it folds and the launch's own
// bodies are read (the other slots may still be landing); else the whole set is in place.  Scratch as launch_fast_sl.
hipError_t launch_fast_sl_phase(const StepArgs &a_in, uint32_t ib, uint32_t slices, bool range, uint32_t r0, uint32_t r1, void *scratch,
                                hipStream_t s)
{
    StepArgs a = a_in;
    const PlaneScratch v = plane_scratch(scratch, a.n_total);
    a.partial = (float4 *)v.behind;
    const uint32_t gen = next_plane_generation();
    hipError_t e;
    if (range) {
        hipLaunchKernelGGL(planes_range_kernel, dim3(ceil_div(a.n_total, kBlock)), dim3(kBlock), 0, s, a.n_total, a.pos_in, v.px, v.py, v.pz, v.flags,
                           r0, r1, a.first, a.first + a.count, kFastPlaneLoBits, kFastPlaneHiBits, 0u, gen);
        e = hipGetLastError();
    } else {
        e = launch_fast_planes(a, v, gen, s);
    }
    if (e != hipSuccess) return e;
    return launch_fast_sl_kernel(a, ib, slices, v.flags, gen, v.px, v.py, v.pz, s);
}

// FAST, every unordered pair once: planes + flags, the superblocks against themselves, the superblock pairs, the rows' combine
hipError_t launch_fast_pairs(const StepArgs &a, uint32_t w, uint32_t np, uint32_t chunk, void *scratch, hipStream_t s)
{
    const PlaneScratch v = plane_scratch(scratch, a.n_total);
    const uint32_t gen = next_plane_generation();
    hipError_t e = launch_fast_planes(a, v, gen, s);
    if (e != hipSuccess) return e;
    return launch_fast_pairs_kernels(a, w, np, chunk, v.flags, gen, v.px, v.py, v.pz, (float *)v.behind, s);
}

// FAST pairs form on a shard: planes + flags, then the ring's sweeps and reduces (nb_nbody_ring.inc)
hipError_t launch_fast_ring(const StepArgs &a, uint32_t np, uint32_t ga, uint32_t wpb, void *scratch, float4 *sums, hipStream_t s)
{
    const PlaneScratch v = plane_scratch(scratch, a.n_total);
    const uint32_t gen = next_plane_generation();
    hipError_t e = launch_fast_planes(a, v, gen, s);
    if (e != hipSuccess) return e;
    return launch_fast_ring_kernels(a, np, ga, wpb, v.flags, gen, v.px, v.py, v.pz, (float *)v.behind, sums, s);
}

// One PHASE of the same step (nb_nbody_ring.inc "PHASES"): what = 1 the pairs inside the rank's own slot that one round of
// workgroups holds -- reads only the records [first, first + count) of pos_in --, 2 every other pair and the sums of the ranks in
// front, 3 the rank's own sums.  Phases 1 and 2 put the planes (and flag words) of what they read in place first.
hipError_t launch_fast_ring_phase(const StepArgs &a, uint32_t np, uint32_t ga, uint32_t wpb, uint32_t c4_own, uint32_t c4_rest, uint32_t cap, uint32_t what,
                                  void *scratch, float4 *sums, hipStream_t s)
{
    const PlaneScratch v = plane_scratch(scratch, a.n_total);
    if (what == 1u || what == 2u) {  // (what == 4: RING_OWN behind a fused finish, which left the own slot's planes and flag words)
        const uint32_t gen = next_plane_generation();
        const bool own = what == 1u;
        const uint32_t r0 = own ? a.first : 0u, r1 = own ? a.first + a.count : a.n_total;
        hipLaunchKernelGGL(ring_planes_kernel, dim3(ceil_div(r1 - r0, kBlock)), dim3(kBlock), 0, s, a.n_total, a.pos_in, v.px, v.py, v.pz,
                           v.flags + (own ? kRingFlagsNext : kRingFlagsRest), r0, r1, gen, own ? (const uint32_t *)nullptr : v.flags + kRingFlagsNext,
                           own ? (uint32_t *)nullptr : v.flags + kRingFlagsOwn);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_ring_phase_kernels(a, np, ga, wpb, c4_own, c4_rest, cap, what, v.flags, v.px, v.py, v.pz, (float *)v.behind, sums, s);
}

// The finish of a step in phases, fused (nb_nbody_ring.inc: ring_finish_phase_kernel): RING_SUMS need not be launched (sums == NULL:
// the rank's own records are added here), and the next step's RING_OWN finds its planes and flag words in `scratch` (what == 4).
hipError_t launch_fast_ring_finish_phase(const StepArgs &a, uint32_t np, uint32_t ga, uint32_t wpb, uint32_t c4_own, uint32_t c4_rest, uint32_t cap, void *scratch,
                                         const float4 *sums, const float4 *recv, hipStream_t s)
{
    const PlaneScratch v = plane_scratch(scratch, a.n_total);
    return launch_ring_finish_phase_kernel(a, np, ga, wpb, c4_own, c4_rest, cap, v.flags, v.px, v.py, v.pz, (float *)v.behind, sums, recv,
                                           next_plane_generation(), s);
}

hipError_t launch_instances(uint32_t count, const float4 *pos, const float4 *vel, float4 *inst, hipStream_t s, uint32_t device_libm)
{
    hipLaunchKernelGGL(instances_kernel, dim3(ceil_div(count, kBlock)), dim3(kBlock), 0, s, count, pos, vel, inst, device_libm);
    return hipGetLastError();
}

hipError_t launch_pack(uint32_t count, const float *xyz, float4 *rec, hipStream_t s)
{
    hipLaunchKernelGGL(pack_kernel, dim3(ceil_div(count, kBlock)), dim3(kBlock), 0, s, count, xyz, rec);
    return hipGetLastError();
}

hipError_t launch_unpack(uint32_t count, const float4 *rec, float *xyz, hipStream_t s)
{
    hipLaunchKernelGGL(unpack_kernel, dim3(ceil_div(count, kBlock)), dim3(kBlock), 0, s, count, rec, xyz);
    return hipGetLastError();
}

hipError_t launch_import(uint32_t count, const float *pos_xyz, const float *vel_xyz, float4 *pos_rec, float4 *vel_rec, hipStream_t s)
{
    hipLaunchKernelGGL(import_kernel, dim3(ceil_div(count, kBlock), 2), dim3(kBlock), 0, s, count, pos_xyz, vel_xyz, pos_rec, vel_rec);
    return hipGetLastError();
}

hipError_t launch_export(uint32_t count, const float4 *pos_rec, const float4 *vel_rec, float4 *inst, float *pos_xyz, float *vel_xyz,
                         const uint32_t *status_src, uint32_t *status_dst, hipStream_t s, uint32_t device_libm, ExportDone done)
{
    hipLaunchKernelGGL(export_kernel, dim3(ceil_div(count, kBlock), 3), dim3(kBlock), 0, s, count, pos_rec, vel_rec, inst, pos_xyz,
                       vel_xyz, status_src, status_dst, device_libm, done);
    return hipGetLastError();
}

#endif  // !NBK_NOSLP_TU

