// nb_ring_api.inc -- FAST on shards with every unordered pair once (nb_nbody_ring.inc) behind the C ABI: the plan (which shards take the form, its phases resolved once), nb_ring_partners / _scratch_bytes / _phased, nb_launch_ring_fold / _fold_phase / _finish.
// Included by nb_api.hip (it uses that file's planning, context and launch helpers); not a translation unit of its own.

// ---- FAST on shards, every unordered pair once ("half shell", nb_nbody_ring.inc) ------------------------------------------
namespace {
constexpr uint64_t kRingMinPairs = 1ull << 30;  // ordered pairs of a rank's step from which the form is taken by itself
struct RingPlan {
    Plan base;      // the sharing verdict (force_ieee), force_3d
    uint32_t np;    // packed pairs of bodies per lane: 4 (blocks of 512) where the shard is whole blocks of 512, else 2 (256)
    uint32_t ga, wpb;
    uint32_t partners;  // 0: this shape does not take the form
    uint32_t c4_own, c4_rest, cap;  // the step in phases: sub-tiles per workgroup, sub-tiles of a block's own part in the first phase (0: the kernels' defaults)
    bool phased;        // the shape can run its step in phases (nb_launch_ring_fold_phase)
    size_t scratch_floats;  // rows behind the planes area: the most ANY rank of the job needs (a host may size one buffer for all)
};
// Which shards take the form by themselves: FAST, at least two equal ranks of whole blocks, and enough pairs per rank that what
// the form saves pays for its second exchange: against the ordered fold of the same shard it saves n_total x count / 3e7 us
// (profiles/r04/ring_times.log, ring_small.log: 15 us at 65 536 x 8 192, 26 at 65 536 x 16 384, 73 at 131 072 x 16 384; nothing at
// 32 768 bodies on 4 or 8 ranks), the second exchange costs 17-23 us on a communicator of one (profiles/r04/step_overhead.log):
// the line is n_total x count >= 2^30.  NB_RING=0/1 decides outright where the shape allows it; NB_RING_NP / NB_RING_GA /
// NB_RING_WPB name the kernel's shape (tests, tools/).
int make_ring_plan(const nb_params &p, uint32_t n_total, uint32_t first, uint32_t count, RingPlan *out, std::string *err)
{
    int rc = make_plan(p, n_total, count, &out->base, err);
    if (rc != NB_OK) return rc;
    const DebugOverrides &dbg = overrides();
    out->partners = 0;
    out->np = (count % 512u == 0u) ? 4u : 2u;
    if (dbg.ring_np.set && (dbg.ring_np.v == 2u || dbg.ring_np.v == 4u)) out->np = dbg.ring_np.v;
    out->ga = dbg.ring_ga.or_else(0u);
    out->wpb = dbg.ring_wpb.or_else(0u) & ~3u;
    out->c4_own = dbg.ring_c4_own.or_else(0u);
    out->c4_rest = dbg.ring_c4_rest.or_else(0u);
    out->cap = dbg.ring_cap.or_else(0u);
    out->phased = false;
    out->scratch_floats = 0;
    if (p.mode != NB_MODE_FAST || (uint64_t)first + count > n_total) return NB_OK;
    if (!dbg.ring.or_else((uint64_t)n_total * count >= kRingMinPairs ? 1u : 0u)) return NB_OK;
    out->partners = nbk::ring_partners(n_total, first, count, out->np);
    // the rows: the phases' layout differs a little from rank to rank (the lists of the upper half of the ring are a block shorter), so
    // the size is the largest of all ranks' -- every rank of a job gets the same answer, as before the phases existed
    if (out->partners)
        for (uint32_t f = 0; (uint64_t)f + count <= n_total; f += count)
            out->scratch_floats = std::max(out->scratch_floats, nbk::ring_scratch_floats(n_total, f, count, out->np, out->ga, out->wpb, out->c4_own, out->c4_rest, out->cap));
    // (the phases' shape is searched for ONCE, here: c4_own / c4_rest / cap leave resolved, and every launch of the plan names them)
    out->phased = out->partners != 0u && nbk::ring_phased(n_total, first, count, out->np, out->ga, out->wpb, &out->c4_own, &out->c4_rest, &out->cap);
    return NB_OK;
}
size_t ring_scratch_bytes(const RingPlan &rp, uint32_t n_total, uint32_t first, uint32_t count)
{
    return nbk::strict_bc_scratch_bytes(n_total) + rp.scratch_floats * sizeof(float);
}
int cached_ring_plan(const nb_params &p, uint32_t n_total, uint32_t first, uint32_t count, const RingPlan **out, std::string *err)
{
    thread_local PlanCache<PlanKey, RingPlan, 2> cache;
    return cache.get(plan_key(p, n_total, first, count), out, [&](RingPlan *rp) { return make_ring_plan(p, n_total, first, count, rp, err); });
}
int launch_ring_fold_planned(const nb_params &p, const RingPlan &rp, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                             void *sums, void *scratch, hipStream_t stream, std::string *err)
{
    const nbk::StepArgs a = step_args(p, rp.base, n_total, first, count, pos_in, nullptr, nullptr);
    hipError_t e = nbk::launch_fast_ring(a, rp.np, rp.ga, rp.wpb, scratch, (float4 *)sums, stream);
    return launch_status(e, "nb: kernel launch failed (ring fold): ", err);
}
int launch_ring_phase_planned(const nb_params &p, const RingPlan &rp, uint32_t n_total, uint32_t first, uint32_t count, int phase, const void *pos_in,
                              void *sums, void *scratch, hipStream_t stream, std::string *err)
{
    const nbk::StepArgs a = step_args(p, rp.base, n_total, first, count, pos_in, nullptr, nullptr);
    hipError_t e = nbk::launch_fast_ring_phase(a, rp.np, rp.ga, rp.wpb, rp.c4_own, rp.c4_rest, rp.cap, (uint32_t)phase, scratch, (float4 *)sums, stream);
    if (e == hipSuccess) return NB_OK;
    return launch_status(e, ("nb: kernel launch failed (ring fold, phase " + std::to_string(phase) + "): ").c_str(), err);
}
int launch_ring_finish_planned(const nb_params &p, const RingPlan &rp, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                               void *pos_out, void *vel, const void *sums, const void *recv, hipStream_t stream, std::string *err)
{
    const nbk::StepArgs a = step_args(p, rp.base, n_total, first, count, pos_in, pos_out, vel);
    hipError_t e = nbk::launch_ring_finish(a, (const float4 *)sums, (const float4 *)recv, rp.partners, stream);
    return launch_status(e, "nb: kernel launch failed (ring finish): ", err);
}
int launch_ring_finish_phase_planned(const nb_params &p, const RingPlan &rp, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                                     void *pos_out, void *vel, const void *sums, const void *recv, void *scratch, hipStream_t stream, std::string *err)
{
    const nbk::StepArgs a = step_args(p, rp.base, n_total, first, count, pos_in, pos_out, vel);
    hipError_t e = nbk::launch_fast_ring_finish_phase(a, rp.np, rp.ga, rp.wpb, rp.c4_own, rp.c4_rest, rp.cap, scratch, (const float4 *)sums, (const float4 *)recv,
                                                      stream);
    return launch_status(e, "nb: kernel launch failed (ring finish, fused): ", err);
}
}  // namespace

NB_EXPORT int nb_ring_partners(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count)
{
    const nb_params p = params_or_default(params);
    const RingPlan *rp = nullptr;
    int rc = cached_ring_plan(p, n_total, first, count, &rp, &g_tls_error);
    if (rc != NB_OK) return rc;
    return (int)rp->partners;
}

NB_EXPORT size_t nb_ring_scratch_bytes(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count)
{
    const nb_params p = params_or_default(params);
    RingPlan rp;
    std::string err;
    if (make_ring_plan(p, n_total, first, count, &rp, &err) != NB_OK || rp.partners == 0u) return 0;
    return ring_scratch_bytes(rp, n_total, first, count);
}

NB_EXPORT int nb_launch_ring_fold(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in, void *sums,
                                  void *scratch, size_t scratch_bytes, void *stream)
{
    const nb_params p = params_or_default(params);
    if (!pos_in || !sums || !scratch) {
        g_tls_error = "nb_launch_ring_fold: pos_in, sums and scratch must be non-null";
        return NB_ERR_INVALID;
    }
    const RingPlan *rp = nullptr;
    int rc = cached_ring_plan(p, n_total, first, count, &rp, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (rp->partners == 0u) {
        g_tls_error = "nb_launch_ring_fold: this shape does not take the pairs form on shards (nb_ring_partners() == 0): use nb_launch_step";
        return NB_ERR_UNSUPPORTED;
    }
    if (scratch_bytes < ring_scratch_bytes(*rp, n_total, first, count)) {
        g_tls_error = "nb_launch_ring_fold: scratch smaller than nb_ring_scratch_bytes()";
        return NB_ERR_INVALID;
    }
    rc = device_for_launch(pos_in, stream, SelectDevice::kForNullStream);
    if (rc != NB_OK) return rc;
    return launch_ring_fold_planned(p, *rp, n_total, first, count, pos_in, sums, scratch, (hipStream_t)stream, &g_tls_error);
}

NB_EXPORT int nb_ring_phased(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count)
{
    const nb_params p = params_or_default(params);
    const RingPlan *rp = nullptr;
    int rc = cached_ring_plan(p, n_total, first, count, &rp, &g_tls_error);
    if (rc != NB_OK) return rc;
    return rp->phased ? 1 : 0;
}

NB_EXPORT int nb_launch_ring_fold_phase(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, int phase, const void *pos_in,
                                        void *sums, void *scratch, size_t scratch_bytes, void *stream)
{
    const nb_params p = params_or_default(params);
    if (!pos_in || !sums || !scratch) {
        g_tls_error = "nb_launch_ring_fold_phase: pos_in, sums and scratch must be non-null";
        return NB_ERR_INVALID;
    }
    if (phase < NB_RING_OWN || phase > NB_RING_OWN_READY) {
        g_tls_error = "nb_launch_ring_fold_phase: phase must be NB_RING_OWN, NB_RING_REST, NB_RING_SUMS or NB_RING_OWN_READY";
        return NB_ERR_INVALID;
    }
    const RingPlan *rp = nullptr;
    int rc = cached_ring_plan(p, n_total, first, count, &rp, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (!rp->phased) {
        g_tls_error = "nb_launch_ring_fold_phase: this shape does not run its step in phases (nb_ring_phased() == 0): use nb_launch_ring_fold";
        return NB_ERR_UNSUPPORTED;
    }
    if (scratch_bytes < ring_scratch_bytes(*rp, n_total, first, count)) {
        g_tls_error = "nb_launch_ring_fold_phase: scratch smaller than nb_ring_scratch_bytes()";
        return NB_ERR_INVALID;
    }
    rc = device_for_launch(pos_in, stream, SelectDevice::kForNullStream);
    if (rc != NB_OK) return rc;
    return launch_ring_phase_planned(p, *rp, n_total, first, count, phase, pos_in, sums, scratch, (hipStream_t)stream, &g_tls_error);
}

NB_EXPORT int nb_launch_ring_finish(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                                    void *pos_out, void *vel, const void *sums, const void *recv, void *stream)
{
    const nb_params p = params_or_default(params);
    if (!pos_in || !pos_out || !vel || !sums || !recv || pos_in == pos_out) {
        g_tls_error = "nb_launch_ring_finish: pos_in, pos_out, vel, sums, recv must be non-null and pos_out must not alias pos_in";
        return NB_ERR_INVALID;
    }
    const RingPlan *rp = nullptr;
    int rc = cached_ring_plan(p, n_total, first, count, &rp, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (rp->partners == 0u) {
        g_tls_error = "nb_launch_ring_finish: this shape does not take the pairs form on shards (nb_ring_partners() == 0)";
        return NB_ERR_UNSUPPORTED;
    }
    rc = device_for_launch(pos_in, stream, SelectDevice::kForNullStream);
    if (rc != NB_OK) return rc;
    return launch_ring_finish_planned(p, *rp, n_total, first, count, pos_in, pos_out, vel, sums, recv, (hipStream_t)stream, &g_tls_error);
}

NB_EXPORT int nb_launch_ring_finish_phase(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                                          void *pos_out, void *vel, const void *sums, const void *recv, void *scratch, size_t scratch_bytes, void *stream)
{
    const nb_params p = params_or_default(params);
    if (!pos_in || !pos_out || !vel || !recv || !scratch || pos_in == pos_out) {
        g_tls_error = "nb_launch_ring_finish_phase: pos_in, pos_out, vel, recv, scratch must be non-null and pos_out must not alias pos_in";
        return NB_ERR_INVALID;
    }
    const RingPlan *rp = nullptr;
    int rc = cached_ring_plan(p, n_total, first, count, &rp, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (!rp->phased) {
        g_tls_error = "nb_launch_ring_finish_phase: this shape does not run its step in phases (nb_ring_phased() == 0): use nb_launch_ring_finish";
        return NB_ERR_UNSUPPORTED;
    }
    if (scratch_bytes < ring_scratch_bytes(*rp, n_total, first, count)) {
        g_tls_error = "nb_launch_ring_finish_phase: scratch smaller than nb_ring_scratch_bytes()";
        return NB_ERR_INVALID;
    }
    rc = device_for_launch(pos_in, stream, SelectDevice::kForNullStream);
    if (rc != NB_OK) return rc;
    return launch_ring_finish_phase_planned(p, *rp, n_total, first, count, pos_in, pos_out, vel, sums, recv, scratch, (hipStream_t)stream, &g_tls_error);
}
