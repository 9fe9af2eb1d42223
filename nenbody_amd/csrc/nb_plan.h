// nb_plan.h -- the n-body step planner: which kernel form a step of (params, n_total, count) takes and with which launch shape.
//
// Pure host arithmetic: plain C++17, no HIP header, no global state; it compiles with g++ against include/nenbody.h alone
// (tests/cpp/plan_table.cpp holds every decision below against tests/golden/plan_table.txt).  nb_api.hip passes the process's
// overrides and the kernels' own size functions in, and instantiates visit_launch() with the real launchers.
// The measurements behind the size lines are told in DESIGN.md sections 4 and 8; each line keeps its reason and its profile here.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>

#include "../../include/nenbody.h"

namespace nbp {

// ---- the size lines ------------------------------------------------------------------------------------------------------------
// MI355X: 256 CUs x 4 SIMDs.  FAST launches aim at 16 waves per SIMD's worth of work items, four times what is resident at once:
// later rounds go to whoever is free (2.53 ms against 2.80 with one round at N = 131 072, profiles/r02/fast_forms.log).
constexpr uint32_t kTargetWaves = 16384;
constexpr uint32_t kMaxSlices = 64;  // blockIdx.y slices of a FAST j range
// The kernels index records and tiles in 32 bits with headroom for padding.
constexpr uint32_t kMaxBodies = 0x80000000u;
// FAST bodies per lane by the size of the launch in pairs: 4 from 16 384 of 131 072 bodies on (0.340 ms against 0.360 with 2), 2 for
// standalone sets of 32 768 and 16 384 (0.184 against 0.207 with 4), 1 for 8 192 and below (profiles/r02/fast_forms.log).
constexpr uint64_t kFastIb4Pairs = 1ull << 31;
constexpr uint64_t kFastIb2Pairs = 1ull << 27;
// FAST through scalar loads from 4 096 bodies on: below, its second launch -- the planes -- costs more than it saves.
constexpr uint32_t kFastSlMinN = 4096;
// The FAST pairs form wins from 32 768 bodies on: 0.95 of the ordered fold's time there, 0.82 at 65 536, 0.76-0.78 from 114 688 on
// (profiles/r03/pairs_sizes.log); beyond 4 194 304 bodies its chunked walk is not built.
constexpr uint32_t kPairsMinN = 32768;
constexpr uint32_t kPairsMaxN = 4194304;
// Pairs form, from 98 304 bodies on a lane holds EIGHT bodies (blocks of 512) where the size allows: the step's fixed costs are shared
// by twice the pairs (1.68 against 1.78 ms at 131 072, profiles/r03/pairs_sizes_np.log); below, 142 registers leave too few waves.
constexpr uint32_t kPairsNp4MinN = 98304;
// Pairs form, waves per workgroup double from 131 072 bodies on: below, the larger workgroups are too few and too long (1.12 ms
// against 1.02 at 98 304, profiles/r03/pairs_sizes.log).
constexpr uint32_t kPairsWideMinN = 131072;
// STRICT shards of up to 57 344 bodies take a chained form: above, the scalar-load kernel, one wave per SIMD and nothing to wait
// for, beats every chain (a 65 536-body shard of 131 072: 2.95 ms against the block chain's 3.35, profiles/r03/shard_strict_forms.log).
constexpr uint32_t kChainMax = 57344;
// STRICT sets below 1 536 bodies keep the j-parallel form: the block chain's second launch costs more than the form gains
// (profiles/r02/small_forms.log).
constexpr uint32_t kSmallSet = 1536;
// STRICT, j-parallel: lanes per body double until the shard supplies 2 waves per SIMD (256 CUs x 4 SIMDs x 2 waves x 64 lanes); the
// DPP adds cost about twice a plain add, so one lane stays ahead down to one wave per SIMD (profiles/r01_jp/sweep_lanes.log).
constexpr uint64_t kStrictFillLanes = 2048ull * 64ull;

// ---- diagnostic overrides (the structs; nb_api.hip reads the environment into them) -----------------------------------------------
struct Knob {
    bool set = false;
    uint32_t v = 0;
    // the override if present, else the default
    uint32_t or_else(uint32_t dflt) const { return set ? v : dflt; }
    bool on() const { return set && v != 0; }
};
struct DebugOverrides {
    Knob tile, fast_pairs_w, fast_pairs_np, fast_pairs_chunk, fast_ib, fast_groups, fast_waves, fast_slices, fast_no_share, strict_force_ieee, force_3d, strict_no_packed, strict_lanes, strict_unroll,
        strict_pc, strict_bc, strict_sl, fast_sl, fast_pairs, ring, ring_np, ring_ga, ring_wpb, ring_c4_own, ring_c4_rest, ring_cap, inst_device_libm, boids_slices, bc_spin_budget, bc_prio, boids_pc, boids_tile, boids_force, selftest_control, roctx, dropin_zero_copy, dropin_poll, dropin_poll_budget_us;
    uint32_t generation = 0;  // bumped by every reload: invalidates cached plans
};

// The NB_* variable of each knob -- NB_ROCTX apart, a feature for the host that is read whether or not the knobs are enabled.
struct KnobName {
    const char *name;
    Knob DebugOverrides::*knob;
};
constexpr KnobName kKnobNames[] = {
    {"NB_TILE", &DebugOverrides::tile}, {"NB_FAST_IB", &DebugOverrides::fast_ib}, {"NB_FAST_GROUPS", &DebugOverrides::fast_groups},
    {"NB_FAST_WAVES", &DebugOverrides::fast_waves}, {"NB_FAST_SLICES", &DebugOverrides::fast_slices}, {"NB_FAST_NO_SHARE", &DebugOverrides::fast_no_share},
    {"NB_STRICT_FORCE_IEEE", &DebugOverrides::strict_force_ieee}, {"NB_FORCE_3D", &DebugOverrides::force_3d}, {"NB_STRICT_NO_PACKED", &DebugOverrides::strict_no_packed},
    {"NB_STRICT_LANES", &DebugOverrides::strict_lanes}, {"NB_STRICT_UNROLL", &DebugOverrides::strict_unroll}, {"NB_STRICT_PC", &DebugOverrides::strict_pc},
    {"NB_STRICT_BC", &DebugOverrides::strict_bc}, {"NB_STRICT_SL", &DebugOverrides::strict_sl}, {"NB_FAST_SL", &DebugOverrides::fast_sl},
    {"NB_FAST_PAIRS", &DebugOverrides::fast_pairs}, {"NB_FAST_PAIRS_W", &DebugOverrides::fast_pairs_w}, {"NB_FAST_PAIRS_CHUNK", &DebugOverrides::fast_pairs_chunk},
    {"NB_FAST_PAIRS_NP", &DebugOverrides::fast_pairs_np}, {"NB_INST_DEVICE_LIBM", &DebugOverrides::inst_device_libm}, {"NB_RING", &DebugOverrides::ring},
    {"NB_RING_NP", &DebugOverrides::ring_np}, {"NB_RING_GA", &DebugOverrides::ring_ga}, {"NB_RING_WPB", &DebugOverrides::ring_wpb},
    {"NB_RING_C4_OWN", &DebugOverrides::ring_c4_own}, {"NB_RING_C4_REST", &DebugOverrides::ring_c4_rest}, {"NB_RING_CAP", &DebugOverrides::ring_cap},
    {"NB_BC_SPIN_BUDGET", &DebugOverrides::bc_spin_budget}, {"NB_BC_PRIO", &DebugOverrides::bc_prio}, {"NB_BOIDS_PC", &DebugOverrides::boids_pc},
    {"NB_BOIDS_TILE", &DebugOverrides::boids_tile}, {"NB_BOIDS_FORCE", &DebugOverrides::boids_force}, {"NB_BOIDS_SLICES", &DebugOverrides::boids_slices},
    {"NB_DROPIN_ZERO_COPY", &DebugOverrides::dropin_zero_copy}, {"NB_DROPIN_POLL", &DebugOverrides::dropin_poll}, {"NB_DROPIN_POLL_BUDGET_US", &DebugOverrides::dropin_poll_budget_us},
    {"NB_SELFTEST_CONTROL", &DebugOverrides::selftest_control},
};

// ---- forms ----------------------------------------------------------------------------------------------------------------------
// One value per thing that can be launched (visit_launch below is the one place that maps them to launchers).
enum class Form : uint32_t {
    StrictTiled,  // the LDS-tiled kernel (nb_nbody_strict.inc): one lane per body, or j-parallel with Plan::lanes lanes
    StrictPc,     // producer/consumer (nb_nbody_pc.inc)
    StrictBc,     // block chain (nb_nbody_bc.inc)
    StrictSl,     // scalar loads from planes (nb_nbody_sl.inc)
    FastTile,     // workgroup tiles (step_fast_kernel)
    FastWave,     // barrier-free, a tile per wave (step_fast_wave_kernel)
    FastSl,       // scalar loads from planes (step_fast_sl_kernel)
    FastPairs,    // every unordered pair once (nb_nbody_sym.inc)
};

struct FormInfo {
    const char *kernels;     // what nb_diag_plan prints, dominant kernel first ...
    const char *tail_whole;  // ... followed by this when one launch holds the fold (FAST: one slice; pairs: one tile),
    const char *tail_split;  // ... or by this when the fold is split
    bool planes;             // lays the planes area at the start of its scratch
    bool status_word;        // reports through the device status word
    bool stamps;             // its kernels carry nb_diag_step_clock's stamps
};
constexpr FormInfo kFormInfo[] = {
    {"step_strict_kernel", "", "", false, false, true},
    {"step_strict_pc_kernel", "", "", false, false, false},
    {"step_strict_bc_kernel,planes_kernel", "", "", true, true, false},
    {"step_strict_sl_kernel,planes_kernel", "", "", true, false, true},
    {"step_fast_kernel", "", ",integrate_partials_kernel", false, false, false},
    {"step_fast_wave_kernel", "", ",integrate_partials_kernel", false, false, true},
    {"step_fast_sl_kernel,planes_kernel", "", ",integrate_partials_kernel", true, false, true},
    {"step_fast_pairs_kernel,planes_kernel,pairs_diag_kernel", ",pairs_integrate_kernel", ",pairs_accumulate_kernel,pairs_finish_kernel", true, false, true},
};  // in the order of Form
inline const FormInfo &form_info(Form f) { return kFormInfo[(uint32_t)f]; }
inline bool is_strict(Form f) { return f <= Form::StrictSl; }

// STRICT: magnitude range {0} U [2^a, 2^b] of coordinates inside which the shared-reciprocal ladder equals the IEEE divide bit for bit
// (strict_divide_guard); |G| in [2^g, 2^(g+1)), bias in [2^c, 2^(c+1)).  force_ieee = 1: no such range, always divide with '/'.
struct DivideGuard {
    uint32_t lo_bits, hi_bits, force_ieee;
    int a, b, g, c;
};

// A planned step.  Fields a form does not read are zero for that form.
struct Plan {
    Form form;
    uint32_t tile;               // STRICT tiled, FAST tile and wave: records per tile (256, 512 or 1024)
    // STRICT
    uint32_t unroll, lanes;      // tiled: pairs in flight per lane (2, 4, 8 or 16), lanes per body (1 = plain; 2..16 = j-parallel, same summation order)
    uint32_t no_packed;          // tiled, producer/consumer: 1 = do not use the j-packed planar fold (NB_STRICT_NO_PACKED=1)
    uint32_t producers;          // producer/consumer: producers per workgroup (8 or 14)
    uint32_t spin_budget, bc_prio;  // block chain: polls per wait, 0 = kernel default (NB_BC_SPIN_BUDGET: the give-up test); raised wave priority around the chain turns (NB_BC_PRIO=0: off)
    uint32_t sl_shape;           // scalar-load: launch shape 0..2 (nb_nbody_sl.inc)
    DivideGuard guard;           // every STRICT form
    // FAST
    uint32_t ib;                 // bodies per lane of the ordered folds: tile, wave, scalar-load, and the phases of every form (make_phase_plan)
    uint32_t slices, j_chunk;    // tile, wave, scalar-load: blockIdx.y slices of the j range (combined through memory), records per chunk
    uint32_t groups;             // tile: 256-lane groups per workgroup, each folding its own j chunk (combined in LDS)
    uint32_t waves;              // wave: waves per workgroup (1, 4, 8 or 16), each folding its own j chunk
    uint32_t pairs_w, pairs_np, pairs_chunk;  // pairs: waves per workgroup (8, 4, 2, 1), packed pairs of bodies per lane (2 or 4), bodies per chunk of the two-level walk (0: the default)
    uint32_t no_share;           // every FAST form: 1 = never share a reciprocal between two pairs (fast_may_share)
    // what every form shares
    uint32_t stamped;  // 1 = nb_diag_step_clock may stamp this launch: the form's kernels carry stamps and, in STRICT, the shape is a whole set's own (one lane per body, no producers)
    uint32_t n_total;  // the set size the plan was made for
    uint32_t force_3d; // 2 = never take the planar shortcut (NB_FORCE_3D=1: tests, measurements)
};

// The one mapping from a form to its launcher and that launcher's scalar arguments.  `v` has one member per launcher of
// nb_kernels.h; nb_api.hip's calls them, the table test's prints them.
template <typename Visitor>
auto visit_launch(const Plan &pl, Visitor &&v)
{
    switch (pl.form) {
    case Form::StrictTiled: return v.strict(pl.tile, pl.unroll, pl.lanes);
    case Form::StrictPc: return v.strict_pc(pl.producers);
    case Form::StrictBc: return v.strict_bc();
    case Form::StrictSl: return v.strict_sl(pl.sl_shape);
    case Form::FastTile: return v.fast(pl.tile, pl.ib, pl.groups, pl.slices);
    case Form::FastWave: return v.fast_wave(pl.tile, pl.ib, pl.waves, pl.slices);
    case Form::FastSl: return v.fast_sl(pl.ib, pl.slices);
    case Form::FastPairs: break;
    }
    return v.fast_pairs(pl.pairs_w, pl.pairs_np, pl.pairs_chunk);
}

// Every plan-derived field of a launch's arguments (nbk::StepArgs, or the table test's stand-in).  The STRICT guard's verdict and FAST's
// sharing verdict land in the same word: each mode's kernels read it as their own.
template <typename Args>
void plan_step_args(const Plan &pl, Args *a)
{
    a->lo_bits = pl.guard.lo_bits;
    a->hi_bits = pl.guard.hi_bits;
    a->force_ieee = pl.guard.force_ieee | pl.no_share;
    a->force_3d = pl.force_3d;
    a->j_chunk = pl.j_chunk;
    a->no_packed = pl.no_packed;
    a->spin_budget = pl.spin_budget;
    a->bc_prio = pl.bc_prio;
}

// `Sizes` below: the kernels' own layout arithmetic (nb_kernels.h) -- planes_bytes(n), pairs_chunk(n, chunk), pairs_rows(n, w, np),
// pairs_scratch_floats(n, w, np, chunk).
template <typename Sizes>
size_t plan_scratch_bytes(const Plan &pl, uint32_t count, const Sizes &sz)
{
    const size_t planes = form_info(pl.form).planes ? sz.planes_bytes(pl.n_total) : 0;
    if (pl.form == Form::FastPairs) return planes + sz.pairs_scratch_floats(pl.n_total, pl.pairs_w, pl.pairs_np, pl.pairs_chunk) * sizeof(float);
    return planes + (pl.slices > 1 ? (size_t)pl.slices * count * 16u : 0);  // rows of float4 partial sums
}
// the kernels one step launches, as nb_diag_plan prints them
template <typename Sizes>
std::string plan_kernels(const Plan &pl, const Sizes &sz)
{
    const FormInfo info = form_info(pl.form);
    const bool split = pl.form == Form::FastPairs ? sz.pairs_chunk(pl.n_total, pl.pairs_chunk) < pl.n_total : pl.slices > 1;
    return std::string(info.kernels) + (split ? info.tail_split : info.tail_whole);
}
// workgroups of a stamped whole-set launch of n bodies (4 stamp words each)
template <typename Sizes>
size_t stamp_groups(const Plan &pl, uint32_t n, const Sizes &sz)
{
    if (pl.form == Form::FastPairs) {  // one workgroup per superblock pair
        const size_t ns = sz.pairs_rows(n, pl.pairs_w, pl.pairs_np);
        return std::max<size_t>(1, ns * (ns - 1) / 2);
    }
    const uint32_t bodies = is_strict(pl.form) ? (pl.sl_shape == 2u ? 64u : 256u) : 64u * pl.ib;
    return (size_t)((n + bodies - 1u) / bodies) * (is_strict(pl.form) ? 1u : pl.slices);
}

// ---- the planner ----------------------------------------------------------------------------------------------------------------
inline bool valid_tile(uint32_t t) { return t == 256 || t == 512 || t == 1024; }

inline int floor_log2f(float x)
{
    int e;
    std::frexp(x, &e);  // x = m * 2^e, m in [0.5, 1)
    return e - 1;
}

// FAST: bodies per thread; two or four also let the thread's pairs share reciprocals
inline uint32_t fast_bodies_per_lane(uint32_t n_total, uint32_t count, const DebugOverrides &dbg)
{
    const uint64_t pairs = (uint64_t)n_total * count;
    uint32_t ib = dbg.fast_ib.or_else(pairs >= kFastIb4Pairs ? 4u : pairs >= kFastIb2Pairs ? 2u : 1u);
    return (ib == 1 || ib == 2 || ib == 4) ? ib : 1u;
}

// FAST: 0 = the workgroup-tile form (step_fast_kernel), else waves per workgroup of the barrier-free form (1, 4, 8 or 16)
inline uint32_t fast_wave_form(const DebugOverrides &dbg)
{
    const uint32_t w = dbg.fast_waves.or_else(8u);  // NB_FAST_WAVES=0: the workgroup-tile form
    return (w == 1 || w == 4 || w == 8 || w == 16) ? w : 0u;
}

// FAST: how a fold over `n_fold` records is split for `count` bodies at `ib` bodies per lane: `groups` chunks inside a
// workgroup (combined in LDS) times `slices` across workgroups (combined through memory by integrate_partials_kernel),
// `chunk` records each (a multiple of the tile).  The split aims at kTargetWaves waves in all.
// `waves` != 0 selects the barrier-free form (step_fast_wave_kernel): a workgroup is `waves` waves that share 64*ib bodies
// and fold one chunk each; then *groups = waves.
inline void fast_split(uint32_t n_fold, uint32_t count, uint32_t ib, uint32_t waves, const DebugOverrides &dbg, uint32_t *tile, uint32_t *groups,
                       uint32_t *slices, uint32_t *chunk)
{
    if (waves && *tile == 1024u) *tile = 512u;  // the wave form stages a whole tile per wave: 256 or 512 records
    if (waves && *tile == 512u && (ib == 1 || waves == 1)) *tile = 256u;  // built 512-record shapes: 4, 8, 16 waves at 2 / 4 bodies per lane
    const uint32_t bodies = waves ? 64u * ib : 256u * ib, chunk_waves = waves ? 1u : 4u;
    const uint32_t blocks = (count + bodies - 1u) / bodies;
    const uint32_t max_by_tiles = std::max(1u, (n_fold + *tile - 1u) / *tile);
    uint32_t split = (kTargetWaves + blocks * chunk_waves - 1u) / (blocks * chunk_waves);
    if (split > max_by_tiles) split = max_by_tiles;
    if (split < 1) split = 1;
    uint32_t g = waves ? waves : dbg.fast_groups.or_else(split >= 4u ? 4u : split >= 2u ? 2u : 1u);
    if (!waves && g != 1 && g != 2 && g != 4) g = 1;
    if (!waves && *tile == 1024u) g = 1;  // groups are built for tiles of 256 and 512 records (4 x 2 x 1024 records = 128 KB of LDS)
    uint32_t sl = dbg.fast_slices.or_else((split + g - 1u) / g);
    if (sl > kMaxSlices) sl = kMaxSlices;
    if (sl < 1) sl = 1;
    uint32_t chunks = sl * g;
    if (chunks > max_by_tiles) chunks = max_by_tiles;
    uint32_t c = (std::max(n_fold, 1u) + chunks - 1u) / chunks;
    c = ((c + *tile - 1u) / *tile) * *tile;
    chunks = (std::max(n_fold, 1u) + c - 1u) / c;   // drop empty chunks ...
    sl = (chunks + g - 1u) / g;                     // ... and the slices made of them
    *groups = g;
    *slices = sl;
    *chunk = c;
}

// STRICT: magnitude range {0} U [2^a, 2^b] of coordinates for which d, n = dx*G, q = n/d and the
// ladder's residuals are all normal binary32 with headroom, so that v_div_scale/v_div_fixup would be
// the identity and the shared-reciprocal ladder equals the IEEE divide bit for bit.
//   nonzero |dx| >= 2^(a-23), |dx| <= 2^(b+1);  d in [bias, 3*2^(2b+2)+bias];  |n| >= 2^(a-23+g)
inline DivideGuard strict_divide_guard(float G_signed, float bias)
{
    DivideGuard gd{0x3f800000u, 0x3f800000u, 1u, 0, 0, 0, 0};
    const float G = std::fabs(G_signed);
    if (!(std::isfinite(G_signed) && std::isfinite(bias) && G > 0.f && bias > 0.f)) return gd;
    const int g = floor_log2f(G), c = floor_log2f(bias);
    const int b = 20;
    const int dmax = std::max(2 * b + 4, c + 2);
    int a = std::max(-100 + 23 - g, -120 + 23 - g + dmax);
    const bool ok = g >= -100 && g <= 100 && c >= -100 && dmax <= 100 && (b + 2 + g - c) <= 120 && a <= b - 1;
    if (!ok) return gd;
    if (a < -120) a = -120;
    return {(uint32_t)(a + 127) << 23, (uint32_t)(b + 127) << 23, 0u, a, b, g, c};
}

// FAST: may two pairs share a reciprocal?  The product of two r^2 must stay normal: bias in [2^-60, 2^60] (coordinates are checked per
// tile on the device).  NB_FAST_NO_SHARE=1: tests, measurements.
inline bool fast_may_share(float bias, const DebugOverrides &dbg)
{
    const bool bias_ok = std::isfinite(bias) && bias >= 0x1p-60f && bias <= 0x1p60f;
    return bias_ok && !dbg.fast_no_share.on();
}

// FAST.  The pairs form where it can run (whole sets of whole 256-body blocks) and wins; else scalar loads for sets of 4 096 bodies and
// more; else the wave form.  Naming a tile, a wave count or groups asks for one of the LDS forms; NB_FAST_SL=0/1 and NB_FAST_PAIRS=0/1
// decide outright, NB_FAST_PAIRS_W / _NP / _CHUNK name the pairs form's shape.  `tile` is legal (make_plan).
inline void plan_fast(const nb_params &p, uint32_t n_total, uint32_t count, uint32_t tile, const DebugOverrides &dbg, Plan *pl)
{
    pl->no_share = fast_may_share(p.bias, dbg) ? 0u : 1u;
    pl->ib = fast_bodies_per_lane(n_total, count, dbg);
    const uint32_t waves = fast_wave_form(dbg);
    const bool no_form_named = p.tile == 0 && !dbg.tile.set && !dbg.fast_waves.set && !dbg.fast_groups.set;
    const bool pairs_ok = count == n_total && n_total % 256u == 0 && n_total <= kPairsMaxN;
    const bool pairs_wins = n_total >= kPairsMinN && no_form_named && !dbg.fast_sl.set && !dbg.fast_ib.set && !dbg.fast_slices.set;
    if (pairs_ok && dbg.fast_pairs.or_else(pairs_wins ? 1u : 0u)) {
        uint32_t np = (n_total >= kPairsNp4MinN && n_total % 512u == 0) ? 4u : 2u;
        if (dbg.fast_pairs_np.set && (dbg.fast_pairs_np.v == 2 || (dbg.fast_pairs_np.v == 4 && n_total % 512u == 0))) np = dbg.fast_pairs_np.v;
        uint32_t w = np == 4u ? (n_total >= kPairsWideMinN ? 4u : 2u) : (n_total >= kPairsWideMinN ? 8u : 4u);
        if (dbg.fast_pairs_w.set && (dbg.fast_pairs_w.v == 1 || dbg.fast_pairs_w.v == 2 || dbg.fast_pairs_w.v == 4 || (dbg.fast_pairs_w.v == 8 && np == 2u)))
            w = dbg.fast_pairs_w.v;
        pl->form = Form::FastPairs;
        pl->pairs_w = w;
        pl->pairs_np = np;
        if (dbg.fast_pairs_chunk.on()) {  // whole superblocks per chunk
            const uint32_t super = 128u * np * w;
            pl->pairs_chunk = std::max(super, dbg.fast_pairs_chunk.v / super * super);
        }
        return;
    }
    uint32_t groups = 0;
    if (dbg.fast_sl.or_else((waves == 8u && n_total >= kFastSlMinN && no_form_named) ? 1u : 0u)) {
        // its own split: 8 waves per workgroup, chunks of whole 256-record tiles (16-record requests stay aligned)
        uint32_t sl_tile = 256u;
        pl->form = Form::FastSl;
        fast_split(n_total, count, pl->ib, 8u, dbg, &sl_tile, &groups, &pl->slices, &pl->j_chunk);
        return;
    }
    pl->tile = tile;
    fast_split(n_total, count, pl->ib, waves, dbg, &pl->tile, &groups, &pl->slices, &pl->j_chunk);
    pl->form = waves ? Form::FastWave : Form::FastTile;
    pl->waves = waves;
    pl->groups = waves ? 0u : groups;
}

// STRICT cannot split the fold over j (the sum is sequential).  Whole sets and shards above kChainMax fill the chip with one lane per
// body: the scalar-load kernel.  Below, from kSmallSet bodies on, the block chain; smaller sets give each body several lanes.  Naming
// another shape (params.tile / NB_TILE, NB_STRICT_PC / _LANES / _UNROLL / _NO_PACKED) asks for the LDS-tiled kernel or the
// producer/consumer form; NB_STRICT_BC=0/1 and NB_STRICT_SL=0/1..3 decide outright.  `tile` is legal (make_plan).
inline void plan_strict(const nb_params &p, uint32_t n_total, uint32_t count, uint32_t tile, const DebugOverrides &dbg, Plan *pl)
{
    pl->guard = strict_divide_guard(p.G, p.bias);
    if (dbg.strict_force_ieee.on()) pl->guard.force_ieee = 1;
    const bool chain_range = count <= kChainMax && n_total >= kSmallSet;
    // the LDS-tiled kernel's shape, legalised to what is built: j-parallel tiles of 256 and 1024 records
    uint32_t lanes = 1;
    if (count <= kChainMax)
        while (lanes < 16 && (uint64_t)count * lanes < kStrictFillLanes) lanes *= 2;
    lanes = dbg.strict_lanes.or_else(lanes);
    if (lanes != 1 && lanes != 2 && lanes != 4 && lanes != 8 && lanes != 16) lanes = 1;
    uint32_t unroll = dbg.strict_unroll.or_else(lanes == 1 ? 8 : (lanes == 16 ? 2 : 4));
    if (lanes == 1 && unroll != 4 && unroll != 8 && unroll != 16) unroll = 8;
    if (lanes > 1 && unroll != 2 && unroll != 4) unroll = 4;
    if (lanes == 16) unroll = 2;
    if (lanes > 1 && tile == 512) tile = 1024;
    if (lanes > 1 && tile == 1024 && unroll == 2 && lanes < 8) unroll = 4;
    uint32_t pc = dbg.strict_pc.or_else(chain_range ? 14u : 0u);
    if (pc != 0 && pc != 14) pc = 8;
    const bool bc = dbg.strict_bc.or_else((chain_range && !dbg.strict_pc.set && !dbg.strict_lanes.set) ? 1u : 0u) != 0;
    const uint32_t sl = bc ? 0u
                           : std::min(3u, dbg.strict_sl.or_else((!pc && lanes == 1 && p.tile == 0 && !dbg.tile.set && !dbg.strict_lanes.set && !dbg.strict_pc.set &&
                                                                 !dbg.strict_unroll.set && !dbg.strict_no_packed.set && n_total >= kSmallSet) ? 1u : 0u));
    pl->form = bc ? Form::StrictBc : sl ? Form::StrictSl : pc ? Form::StrictPc : Form::StrictTiled;
    pl->stamped = (form_info(pl->form).stamps && !pc && lanes == 1) ? 1u : 0u;
    const uint32_t no_packed = dbg.strict_no_packed.on() ? 1u : 0u;
    if (bc) pl->spin_budget = dbg.bc_spin_budget.or_else(0u), pl->bc_prio = dbg.bc_prio.or_else(1u) ? 1u : 0u;
    else if (sl) pl->sl_shape = sl - 1u;  // NB_STRICT_SL = 1 + launch shape
    else if (pc) pl->producers = pc, pl->no_packed = no_packed;
    else pl->tile = tile, pl->unroll = unroll, pl->lanes = lanes, pl->no_packed = no_packed;
}

inline int refuse(std::string *err, const char *why, int rc)
{
    *err = why;
    return rc;
}

inline int validate_plan_request(const nb_params &p, uint32_t n_total, uint32_t count, const DebugOverrides &dbg, uint32_t *tile, std::string *err)
{
    if (n_total == 0 || count == 0 || count > n_total) return refuse(err, "nb: need 0 < count <= n_total", NB_ERR_INVALID);
    if (p.mode != NB_MODE_STRICT && p.mode != NB_MODE_FAST) return refuse(err, "nb: params.mode must be NB_MODE_STRICT or NB_MODE_FAST", NB_ERR_INVALID);
    if (n_total > kMaxBodies) return refuse(err, "nb: sets of more than 2^31 bodies are not supported", NB_ERR_UNSUPPORTED);
    // FAST: the barrier-free form stages a whole tile per wave (256 records: 4 per lane, 120 registers at 4 bodies per lane;
    // 512 would take 142 and cost a wave per SIMD); the workgroup-tile form shares tiles of 512
    *tile = p.tile ? p.tile : dbg.tile.or_else((p.mode == NB_MODE_STRICT) ? 1024u : fast_wave_form(dbg) ? 256u : 512u);
    if (!valid_tile(*tile)) return refuse(err, "nb: params.tile must be 0, 256, 512 or 1024", NB_ERR_INVALID);
    return NB_OK;
}

// Launch shape + STRICT guard range for (params, n_total, count).
inline int make_plan(const nb_params &p, uint32_t n_total, uint32_t count, const DebugOverrides &dbg, Plan *out, std::string *err)
{
    uint32_t tile = 0;
    int rc = validate_plan_request(p, n_total, count, dbg, &tile, err);
    if (rc != NB_OK) return rc;
    Plan pl{};
    pl.n_total = n_total;
    pl.force_3d = dbg.force_3d.on() ? 2u : 0u;
    if (p.mode == NB_MODE_STRICT) {
        plan_strict(p, n_total, count, tile, dbg, &pl);
    } else {
        plan_fast(p, n_total, count, tile, dbg, &pl);
        pl.stamped = form_info(pl.form).stamps ? 1u : 0u;
    }
    *out = pl;
    return NB_OK;
}

// ---- a FAST step in two phases ("Overlap") ------------------------------------------------------------------
struct PhasePlan {
    Plan base;                 // the one-call step's plan: its form, ib, tile, the sharing verdict, force_3d
    uint32_t len[2];           // records folded by phase 0 (the range) and phase 1 (the rest)
    uint32_t groups[2], slices[2], chunk[2];
};
// The phases fold through scalar loads (step_fast_sl_kernel; the planes area in front of the rows) where a shard's one-call step would
// not take an LDS form -- never the pairs form: a phase folds a range of j's, not pairs.
inline bool phase_sl(const PhasePlan &pp) { return pp.base.form == Form::FastSl || pp.base.form == Form::FastPairs; }

inline int make_phase_plan(const nb_params &p, uint32_t n_total, uint32_t count, uint32_t j_lo, uint32_t j_hi, const DebugOverrides &dbg, PhasePlan *out,
                           std::string *err)
{
    if (p.mode != NB_MODE_FAST) return refuse(err, "nb: a step in phases is FAST only: the reference's sum runs j = 0..N-1 in order, and STRICT keeps that order", NB_ERR_UNSUPPORTED);
    if (j_lo > j_hi || j_hi > n_total) return refuse(err, "nb: need j_lo <= j_hi <= n_total", NB_ERR_INVALID);
    int rc = make_plan(p, n_total, count, dbg, &out->base, err);
    if (rc != NB_OK) return rc;
    out->len[0] = j_hi - j_lo;
    out->len[1] = n_total - out->len[0];
    for (int ph = 0; ph < 2; ++ph) {  // scalar loads: eight waves per workgroup, chunks of whole 256-record tiles; else the LDS form's own
        uint32_t tile = phase_sl(*out) ? 256u : out->base.tile;
        fast_split(out->len[ph], count, out->base.ib, phase_sl(*out) ? 8u : out->base.waves, dbg, &tile, &out->groups[ph], &out->slices[ph], &out->chunk[ph]);
    }
    return NB_OK;
}
template <typename Sizes>
size_t phase_scratch_bytes(const PhasePlan &pp, uint32_t count, const Sizes &sz)
{
    return (phase_sl(pp) ? sz.planes_bytes(pp.base.n_total) : 0) + (size_t)(pp.slices[0] + pp.slices[1]) * count * 16u;
}

}  // namespace nbp
