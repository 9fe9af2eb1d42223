// nb_dropin.inc -- the one-call drop-ins nb_update_instance_nbody / _boids / _random: the reference's free functions themselves (src/main.rs:404-410, 443-449, 381-385), their device contexts kept between frames.
// Included by nb_api.hip (it uses that file's planning, context and launch helpers); not a translation unit of its own.

// ---- one-call drop-ins (src/main.rs:404-410, 443-449) ---------------------------------------------------
namespace {
// The drop-in calls keep their device contexts between frames.  A host may alternate controllers or entity counts from
// frame to frame (the reference swaps controllers by editing main.rs:925), so a few contexts are kept, keyed by controller,
// body count and constants; the least recently used slot is rebuilt (stream + five allocations) only when a FOURTH shape shows up.
// The kept contexts hold their device memory -- a FAST whole set in the pairs form has n x n / 2048 x 12 B of rows: 100 MB at
// 131 072 bodies, 0.4 GB at 262 144 -- so the slots OTHER than the one just used are also dropped, least recently used first,
// while the kept contexts together exceed kUpdateCacheBytes (round 4: a host alternating large shapes pinned up to 1.2 GB).
struct UpdateSlot {
    nb_ctx *ctx = nullptr;
    int kind = -1;  // 0 = n-body, 1 = boids, 2 = random walk
    nb_params p{};
    uint64_t used = 0;
    size_t bytes = 0;  // device memory the context holds (records, matrices, staging, scratch)
};
constexpr size_t kUpdateCacheBytes = (size_t)256 << 20;
struct UpdateCache {
    std::mutex mu;
    static constexpr int kSlots = 3;
    UpdateSlot slot[kSlots];
    uint64_t clock = 0;
    nb_ctx *last = nullptr;  // whose error message update_fail reports
    std::vector<float> pos_full, vel_full, tmp;
    // update_instance_random (three slices, main.rs:381-385): the library's own stream position
    uint64_t random_seed = 0x6e656e626f6479ull, random_calls = 0;
};
// never destroyed: a static destructor could run after the HIP runtime's own teardown
UpdateCache &update_cache()
{
    static UpdateCache *c = new UpdateCache();
    return *c;
}

int update_fail(UpdateCache &uc, const char *who, int rc)
{
    g_tls_error = std::string(who) + ": " + (uc.last ? uc.last->err : g_tls_error);
    return rc;
}

// the context for (kind, n, p): a kept one, or a new one in the least recently used slot.  uc.mu is held.
int update_context(UpdateCache &uc, int kind, uint32_t n, const nb_params &p, nb_ctx **out)
{
    UpdateSlot *victim = &uc.slot[0];
    for (UpdateSlot &sl : uc.slot) {
        if (sl.ctx && sl.kind == kind && sl.ctx->n == n && std::memcmp(&sl.p, &p, sizeof(p)) == 0) {
            sl.used = ++uc.clock;
            uc.last = *out = sl.ctx;
            return NB_OK;
        }
        if (!sl.ctx ? victim->ctx != nullptr : (victim->ctx && sl.used < victim->used)) victim = &sl;
    }
    if (victim->ctx) nb_destroy(victim->ctx);
    victim->ctx = nullptr;
    uc.last = nullptr;
    int rc = nb_create(n, 1, &p, &victim->ctx);
    if (rc != NB_OK) return rc;
    victim->kind = kind;
    victim->p = p;
    victim->used = ++uc.clock;
    Plan pl{};
    std::string ignored;
    victim->bytes = (size_t)n * (3 * sizeof(float4) + 16 * sizeof(float) + 22 * sizeof(float)) +
                    (make_plan(p, n, n, &pl, &ignored) == NB_OK ? plan_scratch_bytes(pl, n) : 0);
    for (;;) {  // the new context stays; older ones go while the cache is over its budget
        size_t total = 0;
        UpdateSlot *oldest = nullptr;
        for (UpdateSlot &sl : uc.slot) {
            if (!sl.ctx) continue;
            total += sl.bytes;
            if (&sl != victim && (!oldest || sl.used < oldest->used)) oldest = &sl;
        }
        if (total <= kUpdateCacheBytes || !oldest) break;
        nb_destroy(oldest->ctx);
        oldest->ctx = nullptr;
        oldest->bytes = 0;
    }
    uc.last = *out = victim->ctx;
    return NB_OK;
}

// upload + one step + download with ONE host<->device copy each way and one wait: the per-frame cost of the drop-in
// calls at the reference's own sizes (entity_count 100 .. 2048) is all latency, so every separate copy and
// synchronisation of nb_upload / nb_download shows.  pos / vel: n bodies each; outputs: the first `count` bodies.
// upload + one step + download with ONE host<->device copy each way, one launch to unpack, one to pack, and one wait: the
// per-frame cost of the drop-in calls at the reference's own sizes (entity_count 100 .. 2048) is all latency, so every
// separate copy, launch and synchronisation shows.  (Replaying the five operations as a captured hipGraph was measured
// too: 37 us per call at N = 100 against 30 us with plain launches, no difference at N = 2 048 -- not adopted.)
// pos / vel: n bodies each; outputs: the first `count` bodies.
// kind: 0 = n-body step, 1 = boids step, 2 = random-walk step (stream (seed, step, n) of nb_step_random)
int update_roundtrip(nb_ctx *c, int kind, const nb_boids_params *bp, const float *pos, const float *vel, size_t count,
                     float *pos_out, float *vel_out, float *inst_out, uint64_t seed = 0, uint64_t step = 0)
{
    const size_t n = c->n, xyz = 3 * sizeof(float);
    int rc = ensure_xfer(c);
    if (rc != NB_OK) return rc;
    c->cur = 0;
    c->uploaded = true;
    c->steps = 0;
    // the pack / unpack kernels read and write the pinned host buffer THROUGH THE BUS themselves: the two DMA operations of a
    // staged copy cost more in fixed latency than these few kilobytes cost in bandwidth (kZeroCopyMax)
    rc = small_import(c, pos, vel);  // (no wait between the import and the step)
    if (rc != NB_OK) return rc;
    if (kind == 2) c->steps = step;  // the random walk's stream is indexed by the step counter
    rc = kind == 2 ? nb_step_random(c, 1, seed) : kind == 1 ? nb_step_boids(c, 1, bp) : nb_step(c, 1);
    if (rc != NB_OK) return rc;
    bool with_status = false;
    rc = small_export(c, true, true, true, &with_status);
    // a failure is reported before anything is copied out: the caller's arrays are also this call's inputs
    if (rc == NB_OK) rc = status_from_tail(c, with_status);
    if (rc != NB_OK) return rc;
    std::memcpy(inst_out, c->hxfer, count * 16 * sizeof(float));
    std::memcpy(pos_out, c->hxfer + 16 * n, count * xyz);
    std::memcpy(vel_out, c->hxfer + 19 * n, count * xyz);
    return NB_OK;
}

int update_common(const char *who, bool boids, float *inst, size_t n_inst, float *pos, size_t n_pos, float *opos, size_t n_opos,
                  float *vel, size_t n_vel, float *ovel, size_t n_ovel, const nb_params *np, const nb_boids_params *bp)
{
    if (n_opos != n_pos || n_ovel != n_vel) {  // copy_from_slice (main.rs:415-416, 459-460) panics
        g_tls_error = std::string(who) + ": source slice length does not match destination slice length (" +
                      (n_opos != n_pos ? "old_positions vs positions" : "old_velocities vs velocities") + ")";
        return NB_ERR_INVALID;
    }
    if ((n_pos && (!pos || !opos)) || (n_vel && (!vel || !ovel)) || (n_inst && !inst)) {
        g_tls_error = std::string(who) + ": null array with a nonzero length";
        return NB_ERR_INVALID;
    }
    const size_t xyz = 3 * sizeof(float);
    if (n_pos) std::memcpy(opos, pos, n_pos * xyz);  // main.rs:415 / 459
    if (n_vel) std::memcpy(ovel, vel, n_vel * xyz);  // main.rs:416 / 460
    const size_t count = std::min(n_inst, std::min(n_pos, n_vel));  // zip, main.rs:420-423 / 465-469
    if (count == 0) return NB_OK;
    // The set the device folds over.  n-body: old_positions (main.rs:425).  boids: the position folds run over
    // old_positions.iter() (main.rs:471, 482) and the velocity fold over old_velocities.iter() (main.rs:494), each with its own
    // length -- the reference never indexes one slice by the other's length -- so the device set is the longer of the two
    // and the shorter snapshot is padded with NaN records: a NaN distance fails every `dist < radius` test (main.rs:475, 486,
    // 498), so a padding record contributes to no sum and no count, exactly like an element that is not there.
    const size_t n_set = boids ? std::max(n_pos, n_vel) : n_pos;
    if (n_set > 0xffffffffull) {
        g_tls_error = std::string(who) + ": more than 2^32-1 bodies";
        return NB_ERR_INVALID;
    }
    const nb_params p = params_or_default(np);

    UpdateCache &uc = update_cache();
    std::lock_guard<std::mutex> lock(uc.mu);
    const uint32_t n = (uint32_t)n_set;
    nb_ctx *ctx = nullptr;
    int rc = update_context(uc, boids ? 1 : 0, n, p, &ctx);
    if (rc != NB_OK) return update_fail(uc, who, rc);
    const float *pos_src = opos, *vel_src = ovel;
    if (n_pos < n_set) {  // boids only
        uc.pos_full.assign(n_set * 3, std::nanf(""));
        std::memcpy(uc.pos_full.data(), opos, n_pos * xyz);
        pos_src = uc.pos_full.data();
    }
    if (n_vel < n_set) {
        // n-body: bodies past the zip are computed and dropped; give them a velocity to carry.  boids: see above.
        uc.vel_full.assign(n_set * 3, boids ? std::nanf("") : 0.f);
        std::memcpy(uc.vel_full.data(), ovel, n_vel * xyz);
        vel_src = uc.vel_full.data();
    }
    // Small sets are all latency: one copy each way through pinned memory (41 us per call at N = 100, 87 us at 2 048,
    // against 104 / 143 us with separate copies).  Large sets are all bandwidth: copy straight from and to the caller's
    // arrays (at N = 131 072 the detour through the pinned buffer costs 0.7 ms).  Measured: tools/crossover.py.
    if (n <= kRoundtripMax) {
        rc = update_roundtrip(ctx, boids ? 1 : 0, bp, pos_src, vel_src, count, pos, vel, inst);
        if (rc != NB_OK) return update_fail(uc, who, rc);
        return NB_OK;
    }
    rc = nb_upload(ctx, pos_src, vel_src);
    if (rc == NB_OK) rc = boids ? nb_step_boids(ctx, 1, bp) : nb_step(ctx, 1);
    if (rc != NB_OK) return update_fail(uc, who, rc);
    if (count == n_set) {  // the usual case: all three slices as long as the set
        rc = nb_download(ctx, pos, vel, inst);
        if (rc != NB_OK) return update_fail(uc, who, rc);
        return NB_OK;
    }
    uc.tmp.resize(n_set * 22);
    float *pos_tmp = uc.tmp.data(), *vel_tmp = pos_tmp + 3 * n_set, *inst_tmp = pos_tmp + 6 * n_set;
    rc = nb_download(ctx, pos_tmp, vel_tmp, inst_tmp);
    if (rc != NB_OK) return update_fail(uc, who, rc);
    std::memcpy(pos, pos_tmp, count * xyz);
    std::memcpy(vel, vel_tmp, count * xyz);
    std::memcpy(inst, inst_tmp, count * 16 * sizeof(float));
    return NB_OK;
}
}  // namespace

NB_EXPORT int nb_update_instance_nbody(float *instances_16n, size_t n_instances, float *positions_xyz, size_t n_positions,
                                       float *old_positions_xyz, size_t n_old_positions, float *velocities_xyz,
                                       size_t n_velocities, float *old_velocities_xyz, size_t n_old_velocities,
                                       const nb_params *params)
{
    return update_common("nb_update_instance_nbody", false, instances_16n, n_instances, positions_xyz, n_positions,
                         old_positions_xyz, n_old_positions, velocities_xyz, n_velocities, old_velocities_xyz, n_old_velocities,
                         params, nullptr);
}

NB_EXPORT int nb_update_instance_boids(float *instances_16n, size_t n_instances, float *positions_xyz, size_t n_positions,
                                       float *old_positions_xyz, size_t n_old_positions, float *velocities_xyz,
                                       size_t n_velocities, float *old_velocities_xyz, size_t n_old_velocities,
                                       const nb_boids_params *params)
{
    return update_common("nb_update_instance_boids", true, instances_16n, n_instances, positions_xyz, n_positions,
                         old_positions_xyz, n_old_positions, velocities_xyz, n_velocities, old_velocities_xyz, n_old_velocities,
                         nullptr, params);
}

// update_instance_random (src/main.rs:381-402): three slices, no snapshots; the zip (:386-389) bounds which bodies move.
namespace {
int update_random_common(const char *who, float *instances_16n, size_t n_instances, float *positions_xyz, size_t n_positions,
                         float *velocities_xyz, size_t n_velocities, bool own_stream, uint64_t seed, uint64_t step)
{
    if ((n_positions && !positions_xyz) || (n_velocities && !velocities_xyz) || (n_instances && !instances_16n)) {
        g_tls_error = std::string(who) + ": null array with a nonzero length";
        return NB_ERR_INVALID;
    }
    const size_t count = std::min(n_instances, std::min(n_positions, n_velocities));  // zip, main.rs:386-389
    if (count == 0) return NB_OK;
    if (count > 0xffffffffull) {
        g_tls_error = std::string(who) + ": more than 2^32-1 bodies";
        return NB_ERR_INVALID;
    }
    nb_params p;
    nb_default_params(&p);
    UpdateCache &uc = update_cache();
    std::lock_guard<std::mutex> lock(uc.mu);
    if (own_stream) {  // the three-slice form: the library keeps the seed and counts the calls
        seed = uc.random_seed;
        step = uc.random_calls;
    }
    const uint32_t n = (uint32_t)count;  // every body walks on its own: the device set is exactly the bodies that move
    nb_ctx *ctx = nullptr;
    int rc = update_context(uc, 2, n, p, &ctx);
    if (rc != NB_OK) return update_fail(uc, who, rc);
    if (n <= kRoundtripMax) {
        rc = update_roundtrip(ctx, 2, nullptr, positions_xyz, velocities_xyz, count, positions_xyz, velocities_xyz, instances_16n, seed, step);
    } else {
        rc = nb_upload(ctx, positions_xyz, velocities_xyz);
        if (rc == NB_OK) {
            ctx->steps = step;
            rc = nb_step_random(ctx, 1, seed);
        }
        if (rc == NB_OK) rc = nb_download(ctx, positions_xyz, velocities_xyz, instances_16n);
    }
    if (rc != NB_OK) return update_fail(uc, who, rc);
    if (own_stream) uc.random_calls++;
    return NB_OK;
}
}  // namespace

NB_EXPORT int nb_update_instance_random(float *instances_16n, size_t n_instances, float *positions_xyz, size_t n_positions,
                                        float *velocities_xyz, size_t n_velocities)
{
    return update_random_common("nb_update_instance_random", instances_16n, n_instances, positions_xyz, n_positions, velocities_xyz,
                                n_velocities, true, 0, 0);
}

NB_EXPORT int nb_update_instance_random_seeded(float *instances_16n, size_t n_instances, float *positions_xyz, size_t n_positions,
                                               float *velocities_xyz, size_t n_velocities, uint64_t seed, uint64_t step)
{
    return update_random_common("nb_update_instance_random_seeded", instances_16n, n_instances, positions_xyz, n_positions,
                                velocities_xyz, n_velocities, false, seed, step);
}

NB_EXPORT void nb_update_random_seed(uint64_t seed)
{
    UpdateCache &uc = update_cache();
    std::lock_guard<std::mutex> lock(uc.mu);
    uc.random_seed = seed;
    uc.random_calls = 0;
}

NB_EXPORT void nb_update_release(void)
{
    UpdateCache &uc = update_cache();
    std::lock_guard<std::mutex> lock(uc.mu);
    for (UpdateSlot &sl : uc.slot) {
        if (sl.ctx) nb_destroy(sl.ctx);
        sl = UpdateSlot();
    }
    uc.last = nullptr;
    uc.pos_full = std::vector<float>();
    uc.vel_full = std::vector<float>();
    uc.tmp = std::vector<float>();
}
