// nb_vision_api.inc -- the C ABI of DESIGN.md sections 12 and 13: the seen set of every eye (nb_launch_seen, nb_eyes_seen), where the
// eye sees its members (nb_seen_located_launch, nb_eyes_located), and the two steps over what each body sees: boids over the seen
// sets (nb_launch_boids_seen_step, nb_step_boids_seen) and gravity over the located ones (nb_nbody_located_step_launch,
// nb_step_nbody_located).  Included by nb_api.hip behind the eye entries, whose checks (eyes_range_check, outputs_check) and staging
// (grow_rows, stage_matrices, launch_matrices) it uses.  The context's entries are one chain -- eye rows, seen sets, located
// sets -- behind one row-entry body and one step body; every check runs before anything touches the device.

static const char kNoSeenOutputs[] = ": seen_count, seen_ids, seen_depth and seen_cols are all NULL";
static const char kNoLocatedOutputs[] = ": seen_count, seen_ids, seen_depth, seen_cols, seen_col and seen_rel are all NULL";
static const char kSeenAlias[] = ": the outputs must not alias each other or an input";

// L6: the rule inverts cp * view only for a perspective constant of the shape nb_camera_constant produces
static int located_cp_check(const char *fn, const float *cp, std::string *err)
{
    static const int zero[11] = {1, 2, 3, 4, 6, 7, 8, 9, 12, 13, 15};
    if (!(cp[11] == -1.0f)) {
        *err = std::string(fn) + ": cp16 cannot be inverted: cp16[11] must be -1 (a perspective constant as nb_camera_constant forms it)";
        return NB_ERR_INVALID;
    }
    for (int i : zero)
        if (!(cp[i] == 0.0f)) {
            *err = std::string(fn) + ": cp16 cannot be inverted: cp16[" + std::to_string(i) + "] must be 0 (a perspective constant as nb_camera_constant forms it)";
            return NB_ERR_INVALID;
        }
    if (cp[0] == 0.0f || cp[14] == 0.0f) {
        *err = std::string(fn) + ": cp16 cannot be inverted: cp16[" + (cp[0] == 0.0f ? "0" : "14") + "] must not be 0 (a perspective constant as nb_camera_constant forms it)";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

static nbk::LocatedArgs located_args(uint32_t count, uint32_t width, const void *ids_rows, const void *depth_rows, const void *seen_count,
                                     const void *seen_ids, const void *seen_depth, const void *dirs, const float *up_xyz, const float *cp16,
                                     void *seen_col, void *seen_rel)
{
    nbk::LocatedArgs a;
    a.count = count, a.width = width;
    a.ids_rows = (const uint32_t *)ids_rows, a.depth_rows = (const uint32_t *)depth_rows;
    a.seen_count = (const uint32_t *)seen_count, a.seen_ids = (const uint32_t *)seen_ids, a.seen_depth = (const uint32_t *)seen_depth;
    a.dirs = (const float4 *)dirs;
    a.ux = up_xyz[0], a.uy = up_xyz[1], a.uz = up_xyz[2];
    a.cp0 = cp16[0], a.cp10 = cp16[10], a.cp14 = cp16[14];
    a.seen_col = (uint32_t *)seen_col, a.seen_rel = (float4 *)seen_rel;
    return a;
}

// ---- the stateless entries of the sets ---------------------------------------------------------------------------------------------------
NB_EXPORT int nb_launch_seen(uint32_t count, uint32_t width, const void *ids_rows, const void *depth_rows, void *seen_count, void *seen_ids,
                             void *seen_depth, void *seen_cols, void *stream)
{
    if (!ids_rows || !seen_count || !seen_ids) {
        g_tls_error = "nb_launch_seen: ids_rows, seen_count and seen_ids must be non-null";
        return NB_ERR_INVALID;
    }
    if (seen_depth && !depth_rows) {
        g_tls_error = "nb_launch_seen: seen_depth needs depth_rows";
        return NB_ERR_INVALID;
    }
    if (((uintptr_t)ids_rows | (uintptr_t)depth_rows) & 3u) {
        g_tls_error = "nb_launch_seen: ids_rows and depth_rows must be 4-byte aligned";
        return NB_ERR_INVALID;
    }
    const size_t cells = (size_t)count * width;
    const ByteRange in[2] = {{ids_rows, cells * 4u}, {depth_rows, cells * 4u}};
    const ByteRange out[4] = {{seen_count, (size_t)count * 4u}, {seen_ids, cells * 4u}, {seen_depth, cells * 4u}, {seen_cols, cells * 4u}};
    int rc = eyes_range_check("nb_launch_seen", count, 0, count, width, false, 0, &g_tls_error);
    if (rc == NB_OK) rc = outputs_check("nb_launch_seen", out, 0xFu, kNoSeenOutputs, true, in, 2, kSeenAlias, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (count == 0) return NB_OK;
    rc = device_for_launch(ids_rows, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    return launch_status(nbk::launch_seen(count, width, (const uint32_t *)ids_rows, (const float *)depth_rows, (uint32_t *)seen_count,
                                          (uint32_t *)seen_ids, (float *)seen_depth, (uint32_t *)seen_cols, (hipStream_t)stream),
                         "nb: seen kernel launch failed: ", &g_tls_error);
}

NB_EXPORT int nb_seen_located_launch(uint32_t count, uint32_t width, const void *ids_rows, const void *depth_rows, const void *seen_count,
                                     const void *seen_ids, const void *seen_depth, const void *eyes, const void *dirs, const float *up_xyz,
                                     const float *cp16, void *seen_col, void *seen_rel, void *stream)
{
    static const char fn[] = "nb_seen_located_launch";
    if (!ids_rows || !depth_rows || !seen_count || !seen_ids || !seen_depth || !eyes || !dirs || !up_xyz || !cp16 || !seen_rel) {
        g_tls_error = std::string(fn) + ": every argument but seen_col and stream must be non-null";
        return NB_ERR_INVALID;
    }
    if (((uintptr_t)ids_rows | (uintptr_t)depth_rows | (uintptr_t)seen_count | (uintptr_t)seen_ids | (uintptr_t)seen_depth | (uintptr_t)seen_col) & 3u) {
        g_tls_error = std::string(fn) + ": the rows, the lists and seen_col must be 4-byte aligned";
        return NB_ERR_INVALID;
    }
    if (((uintptr_t)eyes | (uintptr_t)dirs | (uintptr_t)seen_rel) & 15u) {
        g_tls_error = std::string(fn) + ": eyes, dirs and seen_rel must be 16-byte aligned";
        return NB_ERR_INVALID;
    }
    const size_t cells = (size_t)count * width;
    const ByteRange in[9] = {{ids_rows, cells * 4u},   {depth_rows, cells * 4u},          {seen_count, (size_t)count * 4u},
                             {seen_ids, cells * 4u},   {seen_depth, cells * 4u},          {eyes, (size_t)count * 16u},
                             {dirs, (size_t)count * 16u}, {up_xyz, 3 * sizeof(float)},    {cp16, 16 * sizeof(float)}};
    const ByteRange out[2] = {{seen_col, cells * 4u}, {seen_rel, cells * 16u}};
    int rc = eyes_range_check(fn, count, 0, count, width, false, 0, &g_tls_error);
    if (rc == NB_OK) rc = located_cp_check(fn, cp16, &g_tls_error);
    if (rc == NB_OK) rc = outputs_check(fn, out, 0x2u, "", false, in, 9, kSeenAlias, &g_tls_error);   // (seen_rel is there, aligned: above)
    if (rc != NB_OK) return rc;
    if (count == 0) return NB_OK;
    rc = device_for_launch(ids_rows, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    return launch_status(nbk::launch_located(located_args(count, width, ids_rows, depth_rows, seen_count, seen_ids, seen_depth, dirs, up_xyz,
                                                          cp16, seen_col, seen_rel),
                                             (hipStream_t)stream),
                         "nb: located kernel launch failed: ", &g_tls_error);
}

// ---- the context's chain: eye rows, seen sets, located sets ------------------------------------------------------------------------------
// Which of the context's optional rows an entry wants, beside the id rows, seen_count and seen_ids that every entry has.
struct VisionRows {
    bool depth;     // the depth rows and seen_depth
    bool cols;      // seen_cols
    bool located;   // loc_rel: the chain ends with the located sets (which read the depth rows and seen_depth: L1)
    bool col;       // loc_col
};

// those rows for `eyes` eyes of `cells` slots together
static int grow_vision(nb_ctx *ctx, const VisionRows &r, size_t eyes, size_t cells)
{
    const int rc = grow_rows(ctx, ctx, r.depth ? ctx : nullptr, nullptr, nullptr, cells, cells);
    if (rc != NB_OK) return rc;
    NB_HIP(ctx, ctx->seen_count.reserve(eyes));
    NB_HIP(ctx, ctx->seen_ids.reserve(cells));
    if (r.depth) NB_HIP(ctx, ctx->seen_depth.reserve(cells));
    if (r.cols) NB_HIP(ctx, ctx->seen_cols.reserve(cells));
    if (r.col) NB_HIP(ctx, ctx->loc_col.reserve(cells));
    if (r.located) NB_HIP(ctx, ctx->loc_rel.reserve(cells));
    return NB_OK;
}

// Eyes [first, first + cnt) on the context's rows and stream: their rows, their seen sets and, where wanted, their located sets.
// The caller has staged their cameras (ctx->cams, eye `first` at its head) and the set's model matrices (ctx->inst).
static int vision_chain(nb_ctx *ctx, const VisionRows &r, uint32_t first, uint32_t cnt, uint32_t width, uint32_t flags, const float *up_xyz,
                        const float *cp16)
{
    NB_HIP(ctx, nbk::launch_eyes(ctx->n, first, cnt, (const float *)ctx->cams.p, (const float *)ctx->inst.p, width, flags, ctx->eye_ids.p,
                                 r.depth ? ctx->eye_depth.p : nullptr, ctx->stream));
    NB_HIP(ctx, nbk::launch_seen(cnt, width, ctx->eye_ids.p, r.depth ? ctx->eye_depth.p : nullptr, ctx->seen_count.p, ctx->seen_ids.p,
                                 r.depth ? ctx->seen_depth.p : nullptr, r.cols ? ctx->seen_cols.p : nullptr, ctx->stream));
    if (r.located)
        NB_HIP(ctx, nbk::launch_located(located_args(cnt, width, ctx->eye_ids.p, ctx->eye_depth.p, ctx->seen_count.p, ctx->seen_ids.p,
                                                     ctx->seen_depth.p, ctx->vel.p + first, up_xyz, cp16, r.col ? ctx->loc_col.p : nullptr,
                                                     ctx->loc_rel.p),
                                        ctx->stream));
    return NB_OK;
}

// The context's row entries: check, grow, stage, chain, download.  host: seen_count, seen_ids, seen_depth, seen_cols, seen_col,
// seen_rel (NULL: not wanted; nb_eyes_seen has no last two); only the rows the wanted outputs need are computed.
static int ctx_vision_rows(nb_ctx *ctx, const char *fn, bool located, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16,
                           uint32_t width, uint32_t flags, void *const (&host)[6])
{
    int rc = ctx_check(ctx, fn);
    if (rc != NB_OK) return rc;
    if (!up_xyz || !cp16) {
        ctx->err = std::string(fn) + ": null argument";
        return NB_ERR_INVALID;
    }
    const size_t cells = (size_t)count * width;
    const ByteRange in[2] = {{up_xyz, 3 * sizeof(float)}, {cp16, 16 * sizeof(float)}};
    const ByteRange out[6] = {{host[0], (size_t)count * 4u}, {host[1], cells * 4u}, {host[2], cells * 4u},
                              {host[3], cells * 4u},         {host[4], cells * 4u}, {host[5], cells * 16u}};
    rc = eyes_range_check(fn, ctx->n, first, count, width, false, flags, &ctx->err);
    if (rc == NB_OK && located) rc = located_cp_check(fn, cp16, &ctx->err);
    if (rc == NB_OK) rc = outputs_check(fn, out, 0x3Fu, located ? kNoLocatedOutputs : kNoSeenOutputs, false, in, 2, kSeenAlias, &ctx->err);
    if (rc == NB_OK) rc = ctx_check(ctx, fn, "");
    if (rc != NB_OK) return rc;
    if (count == 0) return NB_OK;
    const VisionRows r = {located || host[2], host[3] != nullptr, located, host[4] != nullptr};
    rc = grow_vision(ctx, r, count, cells);
    if (rc == NB_OK) rc = stage_matrices(ctx, first, count, up_xyz, cp16);
    if (rc == NB_OK) rc = vision_chain(ctx, r, first, count, width, flags, up_xyz, cp16);
    if (rc != NB_OK) return rc;
    const void *const rows[6] = {ctx->seen_count.p, ctx->seen_ids.p, ctx->seen_depth.p, ctx->seen_cols.p, ctx->loc_col.p, ctx->loc_rel.p};
    for (int a = 0; a < 6; ++a)
        if (host[a]) NB_HIP(ctx, hipMemcpyAsync(host[a], rows[a], out[a].bytes, hipMemcpyDeviceToHost, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NB_OK;
}

NB_EXPORT int nb_eyes_seen(nb_ctx *ctx, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16, uint32_t width,
                           uint32_t flags, uint32_t *seen_count, uint32_t *seen_ids, float *seen_depth, uint32_t *seen_cols)
{
    return ctx_vision_rows(ctx, "nb_eyes_seen", false, first, count, up_xyz, cp16, width, flags,
                           {seen_count, seen_ids, seen_depth, seen_cols, nullptr, nullptr});
}

NB_EXPORT int nb_eyes_located(nb_ctx *ctx, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16, uint32_t width,
                              uint32_t flags, uint32_t *seen_count, uint32_t *seen_ids, float *seen_depth, uint32_t *seen_cols,
                              uint32_t *seen_col, float *seen_rel)
{
    return ctx_vision_rows(ctx, "nb_eyes_located", true, first, count, up_xyz, cp16, width, flags,
                           {seen_count, seen_ids, seen_depth, seen_cols, seen_col, seen_rel});
}

// ---- the steps over what each body sees --------------------------------------------------------------------------------------------------
// What the two stateless folds check, in their order: the four records and the two lists (there, and no output an input), the
// stride, then `own` -- the entry's own alignment and range checks --, then the written records against the lists (`list_bytes`: of
// one slot of the second list).
template <typename Own>
static int list_step_check(const char *fn, uint32_t first, uint32_t count, const void *pos_in, const void *vel_in, const void *seen_count,
                           const void *list, size_t list_bytes, uint32_t stride, const void *pos_out, const void *vel_out, Own own)
{
    if (!pos_in || !vel_in || !pos_out || !vel_out || !seen_count || !list || pos_in == pos_out || vel_in == vel_out) {
        g_tls_error = std::string(fn) + ": buffers must be non-null and the outputs must not alias the inputs";
        return NB_ERR_INVALID;
    }
    if (stride == 0) {
        g_tls_error = std::string(fn) + ": stride must be at least 1";
        return NB_ERR_INVALID;
    }
    const int rc = own();
    if (rc != NB_OK) return rc;
    const ByteRange lists[2] = {{seen_count, (size_t)count * 4u}, {list, (size_t)count * stride * list_bytes}};
    const void *outs[2] = {(const char *)pos_out + (size_t)first * sizeof(float4), (const char *)vel_out + (size_t)first * sizeof(float4)};
    for (const void *o : outs)
        for (const ByteRange &l : lists)
            if (ranges_overlap(o, (size_t)count * sizeof(float4), l.p, l.bytes)) {
                g_tls_error = std::string(fn) + ": the outputs must not alias the lists";
                return NB_ERR_INVALID;
            }
    return NB_OK;
}

NB_EXPORT int nb_launch_boids_seen_step(const nb_boids_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                                        const void *vel_in, const void *seen_count, const void *seen_ids, uint32_t stride, void *pos_out,
                                        void *vel_out, void *stream)
{
    static const char fn[] = "nb_launch_boids_seen_step";
    nbk::BoidsArgs a;
    int rc = list_step_check(fn, first, count, pos_in, vel_in, seen_count, seen_ids, 4u, stride, pos_out, vel_out, [&]() -> int {
        if (((uintptr_t)seen_count | (uintptr_t)seen_ids) & 3u) {
            g_tls_error = std::string(fn) + ": seen_count and seen_ids must be 4-byte aligned";
            return NB_ERR_INVALID;
        }
        uint32_t tile = 0;
        return make_boids_args(boids_params_or_default(params), n_total, first, count, &a, &tile, &g_tls_error);
    });
    if (rc == NB_OK) rc = device_for_launch(pos_in, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    a.pos_in = (const float4 *)pos_in;
    a.vel_in = (const float4 *)vel_in;
    a.pos_out = (float4 *)pos_out;
    a.vel_out = (float4 *)vel_out;
    return launch_status(nbk::launch_boids_seen(a, (const uint32_t *)seen_count, (const uint32_t *)seen_ids, stride, (hipStream_t)stream),
                         "nb: boids kernel launch failed (seen form): ", &g_tls_error);
}

NB_EXPORT int nb_nbody_located_step_launch(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                                           const void *vel_in, const void *seen_count, const void *seen_rel, uint32_t stride, void *pos_out,
                                           void *vel_out, void *stream)
{
    static const char fn[] = "nb_nbody_located_step_launch";
    const nb_params p = params_or_default(params);
    int rc = list_step_check(fn, first, count, pos_in, vel_in, seen_count, seen_rel, 16u, stride, pos_out, vel_out, [&]() -> int {
        if (count == 0 || (uint64_t)first + count > n_total) {
            g_tls_error = std::string(fn) + ": bodies [first, first + count) must be at least one and lie inside the set";
            return NB_ERR_INVALID;
        }
        if ((uintptr_t)seen_count & 3u) {
            g_tls_error = std::string(fn) + ": seen_count must be 4-byte aligned";
            return NB_ERR_INVALID;
        }
        if (((uintptr_t)pos_in | (uintptr_t)vel_in | (uintptr_t)pos_out | (uintptr_t)vel_out | (uintptr_t)seen_rel) & 15u) {
            g_tls_error = std::string(fn) + ": the records and seen_rel must be 16-byte aligned";
            return NB_ERR_INVALID;
        }
        return NB_OK;
    });
    if (rc == NB_OK) rc = device_for_launch(pos_in, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    nbk::LocatedStepArgs a;
    a.pos_in = (const float4 *)pos_in, a.vel_in = (const float4 *)vel_in, a.pos_out = (float4 *)pos_out, a.vel_out = (float4 *)vel_out;
    a.first = first, a.count = count;
    a.dt = p.dt, a.G = p.G, a.bias = p.bias;
    return launch_status(nbk::launch_nbody_located(a, (const uint32_t *)seen_count, (const float4 *)seen_rel, stride, (hipStream_t)stream),
                         "nb: gravity kernel launch failed (located form): ", &g_tls_error);
}

// What differs between the context's two steps, beside their folds.
struct VisionStep {
    const char *fn;      // the entry's name, for its messages and its trace range
    VisionRows rows;     // what the fold reads (located: cp16 must be invertible, L6)
    size_t col_bytes;    // bytes a column of an eye takes in those rows together: the 64 MiB rule of the default batch
};

// Eyes per batch where the caller leaves the choice (batch = 0): the most whose rows (col_bytes a column and 4 bytes of count an
// eye) stay together at or below 64 MiB, whole sets below that.  The seen step's id rows and list ids, 8 bytes a column: 8 188 eyes
// at width 1024, >= 2 047 (width 4096).  The located step's id and depth rows, list ids and depths and seen_rel, 32 bytes: 2 047
// eyes at width 1024, >= 511.
static uint32_t vision_default_batch(uint32_t n, uint32_t width, size_t col_bytes)
{
    const size_t per_eye = (size_t)width * col_bytes + 4u;
    return (uint32_t)std::min<size_t>(n, ((size_t)64 << 20) / per_eye);
}

// The context's steps: check, `prepare` (the fold's constant arguments, which it may refuse), then k times the snapshot's model
// matrices once a step and per batch its cameras, the chain, and `fold` over eyes [b0, b0 + cnt) from ctx->pos[ctx->cur] and
// ctx->vel into ctx->pos[ctx->cur ^ 1] and ctx->vel_alt (V1-V3, G1-G3).
template <typename Prepare, typename Fold>
static int ctx_vision_step(nb_ctx *ctx, const VisionStep &f, uint32_t k, const float *up_xyz, const float *cp16, uint32_t width, uint32_t batch,
                           Prepare prepare, Fold fold)
{
    int rc = ctx_check(ctx, f.fn);
    if (rc != NB_OK) return rc;
    if (!up_xyz || !cp16) {
        ctx->err = std::string(f.fn) + ": null argument";
        return NB_ERR_INVALID;
    }
    rc = eyes_range_check(f.fn, ctx->n, 0, ctx->n, width, false, 0, &ctx->err);
    if (rc == NB_OK && f.rows.located) rc = located_cp_check(f.fn, cp16, &ctx->err);
    if (rc == NB_OK) rc = ctx_check(ctx, f.fn, kCallUpload);
    if (rc == NB_OK) rc = prepare();
    if (rc != NB_OK) return rc;
    if (k == 0) return NB_OK;
    const uint32_t per = std::min(batch ? batch : vision_default_batch(ctx->n, width, f.col_bytes), ctx->n);
    rc = grow_vision(ctx, f.rows, per, (size_t)per * width);
    if (rc != NB_OK) return rc;
    NB_HIP(ctx, ctx->vel_alt.reserve(ctx->n));
    NB_HIP(ctx, ctx->cams.reserve((size_t)ctx->n * 4));
    RoctxRange range(f.fn);
    for (uint32_t s = 0; s < k; ++s) {
        const float4 *pos = ctx->pos[ctx->cur].p;
        NB_HIP(ctx, launch_matrices(ctx->n, pos, ctx->vel.p, &ctx->inst, ctx->stream));
        for (uint32_t b0 = 0; b0 < ctx->n; b0 += per) {
            const uint32_t cnt = std::min(per, ctx->n - b0);
            NB_HIP(ctx, nbk::launch_cameras(cnt, pos + b0, ctx->vel.p + b0, up_xyz, cp16, ctx->cams.p, ctx->stream));
            rc = vision_chain(ctx, f.rows, b0, cnt, width, 0u, up_xyz, cp16);
            if (rc != NB_OK) return rc;
            NB_HIP(ctx, fold(b0, cnt));
        }
        step_done(ctx, true);
    }
    return NB_OK;
}

NB_EXPORT int nb_step_boids_seen(nb_ctx *ctx, uint32_t k, const nb_boids_params *params, const float *up_xyz, const float *cp16,
                                 uint32_t width, uint32_t batch)
{
    static const VisionStep f = {"nb_step_boids_seen", {false, false, false, false}, 8u};
    nbk::BoidsArgs a;
    return ctx_vision_step(
        ctx, f, k, up_xyz, cp16, width, batch,
        [&]() -> int {
            uint32_t tile = 0;
            return make_boids_args(boids_params_or_default(params), ctx->n, 0, ctx->n, &a, &tile, &ctx->err);
        },
        [&](uint32_t b0, uint32_t cnt) {
            a.pos_in = ctx->pos[ctx->cur].p, a.pos_out = ctx->pos[ctx->cur ^ 1].p, a.vel_in = ctx->vel.p, a.vel_out = ctx->vel_alt.p;
            a.first = b0, a.count = cnt;
            return nbk::launch_boids_seen(a, ctx->seen_count.p, ctx->seen_ids.p, width, ctx->stream);
        });
}

NB_EXPORT int nb_step_nbody_located(nb_ctx *ctx, uint32_t k, const float *up_xyz, const float *cp16, uint32_t width, uint32_t batch)
{
    static const VisionStep f = {"nb_step_nbody_located", {true, false, true, false}, 32u};
    nbk::LocatedStepArgs a;
    return ctx_vision_step(
        ctx, f, k, up_xyz, cp16, width, batch,
        [&]() -> int {
            a.dt = ctx->p.dt, a.G = ctx->p.G, a.bias = ctx->p.bias;
            return NB_OK;
        },
        [&](uint32_t b0, uint32_t cnt) {
            a.pos_in = ctx->pos[ctx->cur].p, a.pos_out = ctx->pos[ctx->cur ^ 1].p, a.vel_in = ctx->vel.p, a.vel_out = ctx->vel_alt.p;
            a.first = b0, a.count = cnt;
            return nbk::launch_nbody_located(a, ctx->seen_count.p, ctx->loc_rel.p, width, ctx->stream);
        });
}
