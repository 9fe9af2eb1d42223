// nb_seen_api.inc -- the C ABI of DESIGN.md section 12: the seen set of every eye (nb_launch_seen, nb_eyes_seen) and the boids step
// over what each body sees (nb_launch_boids_seen_step, nb_step_boids_seen).  Included by nb_api.hip behind the eye entries, whose
// checks (eyes_range_check, outputs_check) and staging (grow_row, grow_rows) it uses.  Every check runs before anything touches the
// device.

static const char kNoSeenOutputs[] = ": seen_count, seen_ids, seen_depth and seen_cols are all NULL";
static const char kSeenAlias[] = ": the outputs must not alias each other or an input";

// Eyes per batch of nb_step_boids_seen where the caller leaves the choice (batch = 0): the most whose id rows and lists (8 bytes a
// column and 4 bytes of count an eye) stay together at or below 64 MiB -- 8 188 eyes at width 1024 --, whole sets below that.
static uint32_t seen_default_batch(uint32_t n, uint32_t width)
{
    const size_t per_eye = (size_t)width * 8u + 4u;
    const size_t most = ((size_t)64 << 20) / per_eye;   // >= 2 047 (width 4096)
    return (uint32_t)std::min<size_t>(n, most);
}

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

// the context's list rows for `eyes` eyes of `cells` slots together (depth / cols: wanted or not)
static int grow_seen(nb_ctx *ctx, size_t eyes, size_t cells, bool depth, bool cols)
{
    NB_HIP(ctx, grow_row(&ctx->seen_count, &ctx->seen_count_cap, eyes, sizeof(uint32_t)));
    NB_HIP(ctx, grow_row(&ctx->seen_ids, &ctx->seen_ids_cap, cells, sizeof(uint32_t)));
    if (depth) NB_HIP(ctx, grow_row(&ctx->seen_depth, &ctx->seen_depth_cap, cells, sizeof(float)));
    if (cols) NB_HIP(ctx, grow_row(&ctx->seen_cols, &ctx->seen_cols_cap, cells, sizeof(uint32_t)));
    return NB_OK;
}

NB_EXPORT int nb_eyes_seen(nb_ctx *ctx, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16, uint32_t width,
                           uint32_t flags, uint32_t *seen_count, uint32_t *seen_ids, float *seen_depth, uint32_t *seen_cols)
{
    if (!ctx) {
        g_tls_error = "nb_eyes_seen: ctx is null";
        return NB_ERR_INVALID;
    }
    if (!up_xyz || !cp16) {
        ctx->err = "nb_eyes_seen: null argument";
        return NB_ERR_INVALID;
    }
    const size_t cells = (size_t)count * width;
    const ByteRange in[2] = {{up_xyz, 3 * sizeof(float)}, {cp16, 16 * sizeof(float)}};
    const ByteRange out[4] = {{seen_count, (size_t)count * 4u}, {seen_ids, cells * 4u}, {seen_depth, cells * 4u}, {seen_cols, cells * 4u}};
    int rc = eyes_range_check("nb_eyes_seen", ctx->n, first, count, width, false, flags, &ctx->err);
    if (rc == NB_OK) rc = outputs_check("nb_eyes_seen", out, 0xFu, kNoSeenOutputs, false, in, 2, kSeenAlias, &ctx->err);
    if (rc != NB_OK) return rc;
    if (!ctx->uploaded) {
        ctx->err = "nb_eyes_seen: no state uploaded";
        return NB_ERR_STATE;
    }
    if (count == 0) return NB_OK;
    rc = grow_rows(ctx, ctx, seen_depth, nullptr, nullptr, cells, cells);   // the id rows always, the depth rows for seen_depth
    if (rc == NB_OK) rc = grow_seen(ctx, count, cells, seen_depth != nullptr, seen_cols != nullptr);
    if (rc == NB_OK) rc = stage_matrices(ctx, first, count, up_xyz, cp16);
    if (rc != NB_OK) return rc;
    NB_HIP(ctx, nbk::launch_eyes(ctx->n, first, count, (const float *)ctx->cams, (const float *)ctx->inst, width, flags, ctx->eye_ids,
                                 seen_depth ? ctx->eye_depth : nullptr, ctx->stream));
    NB_HIP(ctx, nbk::launch_seen(count, width, ctx->eye_ids, seen_depth ? ctx->eye_depth : nullptr, ctx->seen_count, ctx->seen_ids,
                                 seen_depth ? ctx->seen_depth : nullptr, seen_cols ? ctx->seen_cols : nullptr, ctx->stream));
    if (seen_count) NB_HIP(ctx, hipMemcpyAsync(seen_count, ctx->seen_count, (size_t)count * 4u, hipMemcpyDeviceToHost, ctx->stream));
    if (seen_ids) NB_HIP(ctx, hipMemcpyAsync(seen_ids, ctx->seen_ids, cells * 4u, hipMemcpyDeviceToHost, ctx->stream));
    if (seen_depth) NB_HIP(ctx, hipMemcpyAsync(seen_depth, ctx->seen_depth, cells * 4u, hipMemcpyDeviceToHost, ctx->stream));
    if (seen_cols) NB_HIP(ctx, hipMemcpyAsync(seen_cols, ctx->seen_cols, cells * 4u, hipMemcpyDeviceToHost, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NB_OK;
}

NB_EXPORT int nb_launch_boids_seen_step(const nb_boids_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                                        const void *vel_in, const void *seen_count, const void *seen_ids, uint32_t stride, void *pos_out,
                                        void *vel_out, void *stream)
{
    const nb_boids_params p = boids_params_or_default(params);
    if (!pos_in || !vel_in || !pos_out || !vel_out || !seen_count || !seen_ids || pos_in == pos_out || vel_in == vel_out) {
        g_tls_error = "nb_launch_boids_seen_step: buffers must be non-null and the outputs must not alias the inputs";
        return NB_ERR_INVALID;
    }
    if (stride == 0) {
        g_tls_error = "nb_launch_boids_seen_step: stride must be at least 1";
        return NB_ERR_INVALID;
    }
    if (((uintptr_t)seen_count | (uintptr_t)seen_ids) & 3u) {
        g_tls_error = "nb_launch_boids_seen_step: seen_count and seen_ids must be 4-byte aligned";
        return NB_ERR_INVALID;
    }
    nbk::BoidsArgs a;
    uint32_t tile = 0;
    int rc = make_boids_args(p, n_total, first, count, &a, &tile, &g_tls_error);
    if (rc != NB_OK) return rc;
    const ByteRange lists[2] = {{seen_count, (size_t)count * 4u}, {seen_ids, (size_t)count * stride * 4u}};
    const void *outs[2] = {(const char *)pos_out + (size_t)first * sizeof(float4), (const char *)vel_out + (size_t)first * sizeof(float4)};
    for (const void *o : outs)
        for (const ByteRange &l : lists)
            if (ranges_overlap(o, (size_t)count * sizeof(float4), l.p, l.bytes)) {
                g_tls_error = "nb_launch_boids_seen_step: the outputs must not alias the lists";
                return NB_ERR_INVALID;
            }
    rc = device_for_launch(pos_in, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    a.pos_in = (const float4 *)pos_in;
    a.vel_in = (const float4 *)vel_in;
    a.pos_out = (float4 *)pos_out;
    a.vel_out = (float4 *)vel_out;
    return launch_status(nbk::launch_boids_seen(a, (const uint32_t *)seen_count, (const uint32_t *)seen_ids, stride, (hipStream_t)stream),
                         "nb: boids kernel launch failed (seen form): ", &g_tls_error);
}

NB_EXPORT int nb_step_boids_seen(nb_ctx *ctx, uint32_t k, const nb_boids_params *params, const float *up_xyz, const float *cp16,
                                 uint32_t width, uint32_t batch)
{
    if (!ctx) {
        g_tls_error = "nb_step_boids_seen: ctx is null";
        return NB_ERR_INVALID;
    }
    if (!up_xyz || !cp16) {
        ctx->err = "nb_step_boids_seen: null argument";
        return NB_ERR_INVALID;
    }
    int rc = eyes_range_check("nb_step_boids_seen", ctx->n, 0, ctx->n, width, false, 0, &ctx->err);
    if (rc != NB_OK) return rc;
    if (!ctx->uploaded) {
        ctx->err = "nb_step_boids_seen: no state uploaded (call nb_upload first)";
        return NB_ERR_STATE;
    }
    const nb_boids_params p = boids_params_or_default(params);
    nbk::BoidsArgs a;
    uint32_t tile = 0;
    rc = make_boids_args(p, ctx->n, 0, ctx->n, &a, &tile, &ctx->err);
    if (rc != NB_OK) return rc;
    if (k == 0) return NB_OK;
    const uint32_t per = std::min(batch ? batch : seen_default_batch(ctx->n, width), ctx->n);
    const size_t cells = (size_t)per * width;
    rc = grow_rows(ctx, ctx, nullptr, nullptr, nullptr, cells, cells);
    if (rc == NB_OK) rc = grow_seen(ctx, per, cells, false, false);
    if (rc != NB_OK) return rc;
    if (!ctx->vel_alt) NB_HIP(ctx, hipMalloc((void **)&ctx->vel_alt, (size_t)ctx->n * sizeof(float4)));
    if (!ctx->cams) NB_HIP(ctx, hipMalloc((void **)&ctx->cams, (size_t)ctx->n * 16 * sizeof(float)));
    if (!ctx->inst) NB_HIP(ctx, hipMalloc((void **)&ctx->inst, (size_t)ctx->n * 16 * sizeof(float)));
    RoctxRange range("nb_step_boids_seen");
    for (uint32_t s = 0; s < k; ++s) {
        a.pos_in = ctx->pos[ctx->cur];
        a.pos_out = ctx->pos[ctx->cur ^ 1];
        a.vel_in = ctx->vel;
        a.vel_out = ctx->vel_alt;
        // V1: the snapshot's model matrices once a step; then per batch its cameras, id rows and seen sets, and the fold (V2-V3)
        NB_HIP(ctx, nbk::launch_instances(ctx->n, a.pos_in, a.vel_in, ctx->inst, ctx->stream, overrides().inst_device_libm.on() ? 1u : 0u));
        for (uint32_t b0 = 0; b0 < ctx->n; b0 += per) {
            const uint32_t cnt = std::min(per, ctx->n - b0);
            NB_HIP(ctx, nbk::launch_cameras(cnt, a.pos_in + b0, a.vel_in + b0, up_xyz, cp16, ctx->cams, ctx->stream));
            NB_HIP(ctx, nbk::launch_eyes(ctx->n, b0, cnt, (const float *)ctx->cams, (const float *)ctx->inst, width, 0u, ctx->eye_ids, nullptr,
                                         ctx->stream));
            NB_HIP(ctx, nbk::launch_seen(cnt, width, ctx->eye_ids, nullptr, ctx->seen_count, ctx->seen_ids, nullptr, nullptr, ctx->stream));
            a.first = b0;
            a.count = cnt;
            NB_HIP(ctx, nbk::launch_boids_seen(a, ctx->seen_count, ctx->seen_ids, width, ctx->stream));
        }
        ctx->cur ^= 1;
        std::swap(ctx->vel, ctx->vel_alt);
        ctx->steps++;
    }
    return NB_OK;
}
