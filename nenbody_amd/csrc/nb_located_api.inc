// nb_located_api.inc -- the C ABI of DESIGN.md section 13: where each eye sees the members of its seen set (nb_seen_located_launch,
// nb_eyes_located) and the gravity step over those relative positions alone (nb_nbody_located_step_launch, nb_step_nbody_located).
// Included by nb_api.hip behind nb_seen_api.inc, whose staging (grow_seen) it uses beside the eye entries' checks (eyes_range_check,
// ranges_overlap) and staging (grow_row, grow_rows, stage_matrices).  Every check runs before anything touches the device.

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

// no output may share a byte with another output or with an input (a NULL range shares none)
static bool located_alias(const ByteRange *out, int n_out, const ByteRange *in, int n_in)
{
    for (int a = 0; a < n_out; ++a) {
        for (int b = a + 1; b < n_out; ++b)
            if ((out[a].p && out[a].p == out[b].p) || ranges_overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes)) return true;
        for (int b = 0; b < n_in; ++b)
            if (ranges_overlap(out[a].p, out[a].bytes, in[b].p, in[b].bytes)) return true;
    }
    return false;
}

// Eyes per batch of nb_step_nbody_located where the caller leaves the choice (batch = 0): the most whose id and depth rows, list ids
// and depths (4 bytes a column each), seen_rel (16 bytes a column) and count (4 bytes an eye) stay together at or below 64 MiB --
// 2 047 eyes at width 1024 --, whole sets below that.
static uint32_t located_default_batch(uint32_t n, uint32_t width)
{
    const size_t per_eye = (size_t)width * 32u + 4u;
    const size_t most = ((size_t)64 << 20) / per_eye;   // >= 511 (width 4096)
    return (uint32_t)std::min<size_t>(n, most);
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
    int rc = eyes_range_check(fn, count, 0, count, width, false, 0, &g_tls_error);
    if (rc == NB_OK) rc = located_cp_check(fn, cp16, &g_tls_error);
    if (rc != NB_OK) return rc;
    const size_t cells = (size_t)count * width;
    const ByteRange in[9] = {{ids_rows, cells * 4u},   {depth_rows, cells * 4u},          {seen_count, (size_t)count * 4u},
                             {seen_ids, cells * 4u},   {seen_depth, cells * 4u},          {eyes, (size_t)count * 16u},
                             {dirs, (size_t)count * 16u}, {up_xyz, 3 * sizeof(float)},    {cp16, 16 * sizeof(float)}};
    const ByteRange out[2] = {{seen_col, cells * 4u}, {seen_rel, cells * 16u}};
    if (located_alias(out, 2, in, 9)) {
        g_tls_error = std::string(fn) + kSeenAlias;
        return NB_ERR_INVALID;
    }
    if (count == 0) return NB_OK;
    rc = device_for_launch(ids_rows, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    return launch_status(nbk::launch_located(located_args(count, width, ids_rows, depth_rows, seen_count, seen_ids, seen_depth, dirs, up_xyz,
                                                          cp16, seen_col, seen_rel),
                                             (hipStream_t)stream),
                         "nb: located kernel launch failed: ", &g_tls_error);
}

// the context's located rows for `cells` slots (col: wanted or not)
static int grow_located(nb_ctx *ctx, size_t cells, bool col)
{
    if (col) NB_HIP(ctx, grow_row(&ctx->loc_col, &ctx->loc_col_cap, cells, sizeof(uint32_t)));
    NB_HIP(ctx, grow_row(&ctx->loc_rel, &ctx->loc_rel_cap, cells, sizeof(float4)));
    return NB_OK;
}

NB_EXPORT int nb_eyes_located(nb_ctx *ctx, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16, uint32_t width,
                              uint32_t flags, uint32_t *seen_count, uint32_t *seen_ids, float *seen_depth, uint32_t *seen_cols,
                              uint32_t *seen_col, float *seen_rel)
{
    static const char fn[] = "nb_eyes_located";
    if (!ctx) {
        g_tls_error = std::string(fn) + ": ctx is null";
        return NB_ERR_INVALID;
    }
    if (!up_xyz || !cp16) {
        ctx->err = std::string(fn) + ": null argument";
        return NB_ERR_INVALID;
    }
    int rc = eyes_range_check(fn, ctx->n, first, count, width, false, flags, &ctx->err);
    if (rc == NB_OK) rc = located_cp_check(fn, cp16, &ctx->err);
    if (rc != NB_OK) return rc;
    if (!seen_count && !seen_ids && !seen_depth && !seen_cols && !seen_col && !seen_rel) {
        ctx->err = std::string(fn) + ": seen_count, seen_ids, seen_depth, seen_cols, seen_col and seen_rel are all NULL";
        return NB_ERR_INVALID;
    }
    const size_t cells = (size_t)count * width;
    const ByteRange in[2] = {{up_xyz, 3 * sizeof(float)}, {cp16, 16 * sizeof(float)}};
    const ByteRange out[6] = {{seen_count, (size_t)count * 4u}, {seen_ids, cells * 4u}, {seen_depth, cells * 4u},
                              {seen_cols, cells * 4u},          {seen_col, cells * 4u}, {seen_rel, cells * 16u}};
    if (located_alias(out, 6, in, 2)) {
        ctx->err = std::string(fn) + kSeenAlias;
        return NB_ERR_INVALID;
    }
    if (!ctx->uploaded) {
        ctx->err = std::string(fn) + ": no state uploaded";
        return NB_ERR_STATE;
    }
    if (count == 0) return NB_OK;
    rc = grow_rows(ctx, ctx, ctx, nullptr, nullptr, cells, cells);   // the id and the depth rows: L1 compares both
    if (rc == NB_OK) rc = grow_seen(ctx, count, cells, true, seen_cols != nullptr);
    if (rc == NB_OK) rc = grow_located(ctx, cells, seen_col != nullptr);
    if (rc == NB_OK) rc = stage_matrices(ctx, first, count, up_xyz, cp16);
    if (rc != NB_OK) return rc;
    NB_HIP(ctx, nbk::launch_eyes(ctx->n, first, count, (const float *)ctx->cams, (const float *)ctx->inst, width, flags, ctx->eye_ids,
                                 ctx->eye_depth, ctx->stream));
    NB_HIP(ctx, nbk::launch_seen(count, width, ctx->eye_ids, ctx->eye_depth, ctx->seen_count, ctx->seen_ids, ctx->seen_depth,
                                 seen_cols ? ctx->seen_cols : nullptr, ctx->stream));
    NB_HIP(ctx, nbk::launch_located(located_args(count, width, ctx->eye_ids, ctx->eye_depth, ctx->seen_count, ctx->seen_ids, ctx->seen_depth,
                                                 ctx->vel + first, up_xyz, cp16, seen_col ? ctx->loc_col : nullptr, ctx->loc_rel),
                                    ctx->stream));
    if (seen_count) NB_HIP(ctx, hipMemcpyAsync(seen_count, ctx->seen_count, (size_t)count * 4u, hipMemcpyDeviceToHost, ctx->stream));
    if (seen_ids) NB_HIP(ctx, hipMemcpyAsync(seen_ids, ctx->seen_ids, cells * 4u, hipMemcpyDeviceToHost, ctx->stream));
    if (seen_depth) NB_HIP(ctx, hipMemcpyAsync(seen_depth, ctx->seen_depth, cells * 4u, hipMemcpyDeviceToHost, ctx->stream));
    if (seen_cols) NB_HIP(ctx, hipMemcpyAsync(seen_cols, ctx->seen_cols, cells * 4u, hipMemcpyDeviceToHost, ctx->stream));
    if (seen_col) NB_HIP(ctx, hipMemcpyAsync(seen_col, ctx->loc_col, cells * 4u, hipMemcpyDeviceToHost, ctx->stream));
    if (seen_rel) NB_HIP(ctx, hipMemcpyAsync(seen_rel, ctx->loc_rel, cells * 16u, hipMemcpyDeviceToHost, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NB_OK;
}

NB_EXPORT int nb_nbody_located_step_launch(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                                           const void *vel_in, const void *seen_count, const void *seen_rel, uint32_t stride, void *pos_out,
                                           void *vel_out, void *stream)
{
    static const char fn[] = "nb_nbody_located_step_launch";
    const nb_params p = params_or_default(params);
    if (!pos_in || !vel_in || !pos_out || !vel_out || !seen_count || !seen_rel || pos_in == pos_out || vel_in == vel_out) {
        g_tls_error = std::string(fn) + ": buffers must be non-null and the outputs must not alias the inputs";
        return NB_ERR_INVALID;
    }
    if (stride == 0) {
        g_tls_error = std::string(fn) + ": stride must be at least 1";
        return NB_ERR_INVALID;
    }
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
    const ByteRange lists[2] = {{seen_count, (size_t)count * 4u}, {seen_rel, (size_t)count * stride * 16u}};
    const void *outs[2] = {(const char *)pos_out + (size_t)first * sizeof(float4), (const char *)vel_out + (size_t)first * sizeof(float4)};
    for (const void *o : outs)
        for (const ByteRange &l : lists)
            if (ranges_overlap(o, (size_t)count * sizeof(float4), l.p, l.bytes)) {
                g_tls_error = std::string(fn) + ": the outputs must not alias the lists";
                return NB_ERR_INVALID;
            }
    int rc = device_for_launch(pos_in, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    nbk::LocatedStepArgs a;
    a.pos_in = (const float4 *)pos_in, a.vel_in = (const float4 *)vel_in, a.pos_out = (float4 *)pos_out, a.vel_out = (float4 *)vel_out;
    a.first = first, a.count = count;
    a.dt = p.dt, a.G = p.G, a.bias = p.bias;
    return launch_status(nbk::launch_nbody_located(a, (const uint32_t *)seen_count, (const float4 *)seen_rel, stride, (hipStream_t)stream),
                         "nb: gravity kernel launch failed (located form): ", &g_tls_error);
}

NB_EXPORT int nb_step_nbody_located(nb_ctx *ctx, uint32_t k, const float *up_xyz, const float *cp16, uint32_t width, uint32_t batch)
{
    static const char fn[] = "nb_step_nbody_located";
    if (!ctx) {
        g_tls_error = std::string(fn) + ": ctx is null";
        return NB_ERR_INVALID;
    }
    if (!up_xyz || !cp16) {
        ctx->err = std::string(fn) + ": null argument";
        return NB_ERR_INVALID;
    }
    int rc = eyes_range_check(fn, ctx->n, 0, ctx->n, width, false, 0, &ctx->err);
    if (rc == NB_OK) rc = located_cp_check(fn, cp16, &ctx->err);
    if (rc != NB_OK) return rc;
    if (!ctx->uploaded) {
        ctx->err = std::string(fn) + ": no state uploaded (call nb_upload first)";
        return NB_ERR_STATE;
    }
    if (k == 0) return NB_OK;
    const uint32_t per = std::min(batch ? batch : located_default_batch(ctx->n, width), ctx->n);
    const size_t cells = (size_t)per * width;
    rc = grow_rows(ctx, ctx, ctx, nullptr, nullptr, cells, cells);
    if (rc == NB_OK) rc = grow_seen(ctx, per, cells, true, false);
    if (rc == NB_OK) rc = grow_located(ctx, cells, false);
    if (rc != NB_OK) return rc;
    if (!ctx->vel_alt) NB_HIP(ctx, hipMalloc((void **)&ctx->vel_alt, (size_t)ctx->n * sizeof(float4)));
    if (!ctx->cams) NB_HIP(ctx, hipMalloc((void **)&ctx->cams, (size_t)ctx->n * 16 * sizeof(float)));
    if (!ctx->inst) NB_HIP(ctx, hipMalloc((void **)&ctx->inst, (size_t)ctx->n * 16 * sizeof(float)));
    nbk::LocatedStepArgs a;
    a.dt = ctx->p.dt, a.G = ctx->p.G, a.bias = ctx->p.bias;
    RoctxRange range("nb_step_nbody_located");
    for (uint32_t s = 0; s < k; ++s) {
        a.pos_in = ctx->pos[ctx->cur];
        a.pos_out = ctx->pos[ctx->cur ^ 1];
        a.vel_in = ctx->vel;
        a.vel_out = ctx->vel_alt;
        // G1: the snapshot's model matrices once a step; then per batch its cameras, rows, seen sets and located sets, and the fold (G2-G3)
        NB_HIP(ctx, nbk::launch_instances(ctx->n, a.pos_in, a.vel_in, ctx->inst, ctx->stream, overrides().inst_device_libm.on() ? 1u : 0u));
        for (uint32_t b0 = 0; b0 < ctx->n; b0 += per) {
            const uint32_t cnt = std::min(per, ctx->n - b0);
            NB_HIP(ctx, nbk::launch_cameras(cnt, a.pos_in + b0, a.vel_in + b0, up_xyz, cp16, ctx->cams, ctx->stream));
            NB_HIP(ctx, nbk::launch_eyes(ctx->n, b0, cnt, (const float *)ctx->cams, (const float *)ctx->inst, width, 0u, ctx->eye_ids,
                                         ctx->eye_depth, ctx->stream));
            NB_HIP(ctx, nbk::launch_seen(cnt, width, ctx->eye_ids, ctx->eye_depth, ctx->seen_count, ctx->seen_ids, ctx->seen_depth, nullptr,
                                         ctx->stream));
            NB_HIP(ctx, nbk::launch_located(located_args(cnt, width, ctx->eye_ids, ctx->eye_depth, ctx->seen_count, ctx->seen_ids,
                                                         ctx->seen_depth, a.vel_in + b0, up_xyz, cp16, nullptr, ctx->loc_rel),
                                            ctx->stream));
            a.first = b0;
            a.count = cnt;
            NB_HIP(ctx, nbk::launch_nbody_located(a, ctx->seen_count, ctx->loc_rel, width, ctx->stream));
        }
        ctx->cur ^= 1;
        std::swap(ctx->vel, ctx->vel_alt);
        ctx->steps++;
    }
    return NB_OK;
}
