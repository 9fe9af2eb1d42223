// nb_scenes_api.inc -- the C ABI of DESIGN.md section 14: scene batches; include/nenbody.h and the nenbody_scenes_*.h behind it name
// and document every entry.  Section 14: k gravity or boids steps of caller-owned records in place, stateless, and the context
// nb_scenes, which owns a batch and a stream.  Section 14.1: the boids step over what each body sees, and the seen sets.  Section 14.2:
// gravity from located vision, and the located sets.  Section 14.4: a neural policy over each eye row, and its observable.  Section
// 14.5: the score of every scene, accumulated on the device.  Section 14.6: an evolution-strategies generation, with keep and rewind.
// Section 14.8: a recurrent policy with per-body memory, its memory's entries and the search over it.  Sections 14.3 and 14.7: the
// helpers the entries share.  Included by nb_api.hip behind nb_vision_api.inc.  Every check runs before
// anything touches the device and has its own message naming the entry.

static_assert(NB_SCENES_MAX_BODIES == nbk::kScenesMaxBodies, "the header's limit is the kernels'");
constexpr uint64_t kScenesMaxRecords = 1ull << 27;   // scenes * n

// the shape of a batch: scenes >= 1, 1 <= n <= NB_SCENES_MAX_BODIES, scenes * n <= 2^27
static int scenes_shape_check(const char *fn, uint32_t scenes, uint32_t n, std::string *err)
{
    if (scenes == 0) {
        *err = std::string(fn) + ": scenes must be at least 1";
        return NB_ERR_INVALID;
    }
    if (n == 0 || n > NB_SCENES_MAX_BODIES) {
        *err = std::string(fn) + ": n must be 1 .. NB_SCENES_MAX_BODIES (2048)";
        return NB_ERR_INVALID;
    }
    if ((uint64_t)scenes * n > kScenesMaxRecords) {
        *err = std::string(fn) + ": scenes * n must be at most 2^27";
        return NB_ERR_UNSUPPORTED;
    }
    return NB_OK;
}

// the nb_params of a batch -- the stateless gravity entry's and the context's, whose located step takes dt, G and bias from them too --:
// a mode there is, then STRICT only (NB_MODE_FAST is NB_ERR_UNSUPPORTED); the tile is validated as elsewhere and otherwise unused
static int scenes_params_check(const char *fn, const nb_params &p, std::string *err)
{
    if (p.mode != NB_MODE_STRICT && p.mode != NB_MODE_FAST) {
        *err = std::string(fn) + ": params.mode must be NB_MODE_STRICT or NB_MODE_FAST";
        return NB_ERR_INVALID;
    }
    if (p.mode != NB_MODE_STRICT) {
        *err = std::string(fn) + ": a scene batch steps STRICT only (params.mode is NB_MODE_FAST)";
        return NB_ERR_UNSUPPORTED;
    }
    if (p.tile != 0 && !valid_tile(p.tile)) {
        *err = std::string(fn) + ": params.tile must be 0, 256, 512 or 1024";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

static int scenes_boids_params_check(const char *fn, const nb_boids_params &p, std::string *err)
{
    if (p.tile != 0 && !valid_tile(p.tile)) {
        *err = std::string(fn) + ": params.tile must be 0, 256, 512 or 1024";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// every pointer of the list there; `tail` is the message behind the entry's name
static int scenes_null_check(const char *fn, std::initializer_list<const void *> ptrs, std::string *err, const char *tail = ": null argument")
{
    for (const void *p : ptrs)
        if (!p) {
            *err = std::string(fn) + tail;
            return NB_ERR_INVALID;
        }
    return NB_OK;
}

// every pointer of the list aligned to `align` bytes, a power of two; `subject` names them in the message
static int scenes_aligned_check(const char *fn, uint32_t align, std::initializer_list<const void *> ptrs, const char *subject, std::string *err)
{
    uintptr_t bits = 0;
    for (const void *p : ptrs) bits |= (uintptr_t)p;
    if (bits & (align - 1u)) {
        *err = std::string(fn) + ": " + subject + " must be " + std::to_string(align) + "-byte aligned";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// the records of a stateless entry: there, 16-byte aligned, not overlapping
static int scenes_records_check(const char *fn, uint32_t scenes, uint32_t n, const void *pos, const void *vel, std::string *err)
{
    const int rc = scenes_aligned_check(fn, 16, {pos, vel}, "pos and vel", err);
    if (rc != NB_OK) return rc;
    const size_t bytes = (size_t)scenes * n * sizeof(float4);
    if (ranges_overlap(pos, bytes, vel, bytes)) {
        *err = std::string(fn) + ": pos and vel must not overlap";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// the launch arguments of k gravity steps: the guard and the forced paths as the planner gives them to a set of n bodies
static int scenes_nbody_args(const nb_params &p, uint32_t scenes, uint32_t n, uint32_t k, void *pos, void *vel, nbk::ScenesNbodyArgs *out,
                             std::string *err)
{
    Plan plan;
    const int rc = make_plan(p, n, n, &plan, err);
    if (rc != NB_OK) return rc;
    const nbk::StepArgs sa = step_args(p, plan, n, 0, n, pos, pos, vel);
    nbk::ScenesNbodyArgs a{};
    a.pos = (float4 *)pos, a.vel = (float4 *)vel;
    a.scenes = scenes, a.n = n, a.k = k;
    a.dt = sa.dt, a.G = sa.G, a.bias = sa.bias;
    a.lo_bits = sa.lo_bits, a.hi_bits = sa.hi_bits, a.force_ieee = sa.force_ieee, a.force_3d = sa.force_3d;
    *out = a;
    return NB_OK;
}

// ---- the stateless entries ----------------------------------------------------------------------------------------------------------------
NB_EXPORT int nb_scenes_nbody_step_launch(const nb_params *params, uint32_t scenes, uint32_t n, uint32_t k, void *pos, void *vel, void *stream)
{
    static const char fn[] = "nb_scenes_nbody_step_launch";
    const nb_params p = params_or_default(params);
    int rc = scenes_null_check(fn, {pos, vel}, &g_tls_error, ": pos and vel must be non-null");
    if (rc == NB_OK) rc = scenes_shape_check(fn, scenes, n, &g_tls_error);
    if (rc == NB_OK) rc = scenes_params_check(fn, p, &g_tls_error);
    if (rc == NB_OK) rc = scenes_records_check(fn, scenes, n, pos, vel, &g_tls_error);
    nbk::ScenesNbodyArgs a;
    if (rc == NB_OK) rc = scenes_nbody_args(p, scenes, n, k, pos, vel, &a, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (k == 0) return NB_OK;
    rc = device_for_launch(pos, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    return launch_status(nbk::launch_scenes_nbody(a, (hipStream_t)stream), "nb: gravity kernel launch failed (scene batch): ", &g_tls_error);
}

NB_EXPORT int nb_scenes_boids_step_launch(const nb_boids_params *params, uint32_t scenes, uint32_t n, uint32_t k, void *pos, void *vel,
                                          void *stream)
{
    static const char fn[] = "nb_scenes_boids_step_launch";
    const nb_boids_params p = boids_params_or_default(params);
    int rc = scenes_null_check(fn, {pos, vel}, &g_tls_error, ": pos and vel must be non-null");
    if (rc == NB_OK) rc = scenes_shape_check(fn, scenes, n, &g_tls_error);
    if (rc == NB_OK) rc = scenes_boids_params_check(fn, p, &g_tls_error);
    if (rc == NB_OK) rc = scenes_records_check(fn, scenes, n, pos, vel, &g_tls_error);
    nbk::BoidsArgs c;
    uint32_t tile = 0;
    if (rc == NB_OK) rc = make_boids_args(p, n, 0, n, &c, &tile, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (k == 0) return NB_OK;
    rc = device_for_launch(pos, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    return launch_status(nbk::launch_scenes_boids(c, (float4 *)pos, (float4 *)vel, scenes, k, (hipStream_t)stream),
                         "nb: boids kernel launch failed (scene batch): ", &g_tls_error);
}

// ---- the seen boids step (DESIGN.md section 14.1): the stateless entries ------------------------------------------------------------------
static const char kScenesSeenAlias[] = ": the outputs must not overlap each other or an input";

static int scenes_width_check(const char *fn, uint32_t width, std::string *err)
{
    if (width == 0 || width > NB_EYES_MAX_WIDTH) {
        *err = std::string(fn) + ": width must be 1 .. NB_EYES_MAX_WIDTH (4096)";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// what the four stateless vision entries check behind their null test: the batch's shape, the width and, where the entry locates
// (cp16 given), a constant that L2 can invert
static int scenes_vision_check(const char *fn, uint32_t scenes, uint32_t n, uint32_t width, const float *cp16, std::string *err)
{
    int rc = scenes_shape_check(fn, scenes, n, err);
    if (rc == NB_OK) rc = scenes_width_check(fn, width, err);
    if (rc == NB_OK && cp16) rc = located_cp_check(fn, cp16, err);
    return rc;
}

// eyes [first_eye, first_eye + count) of the two stateless sets entries lie in the batch
static int scenes_eye_range_check(const char *fn, uint32_t scenes, uint32_t n, uint32_t first_eye, uint32_t count, std::string *err)
{
    if ((uint64_t)first_eye + count > (uint64_t)scenes * n) {
        *err = std::string(fn) + ": eyes [first_eye, first_eye + count) exceed the batch";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// the buffers of a stateless vision step: 16-byte aligned, pos_out and vel_out clear of each other and of every input (up_xyz and
// cp16: the located step's, NULL otherwise)
static int scenes_step_buffers_check(const char *fn, size_t records, const void *cams_16, const void *inst_16, const void *pos_in,
                                     const void *vel_in, const void *pos_out, const void *vel_out, const float *up_xyz, const float *cp16,
                                     std::string *err)
{
    const int rc = scenes_aligned_check(fn, 16, {cams_16, inst_16, pos_in, vel_in, pos_out, vel_out}, "cams_16, inst_16 and the four record buffers", err);
    if (rc != NB_OK) return rc;
    const size_t bytes = records * sizeof(float4);
    const ByteRange in[6] = {{cams_16, bytes * 4u}, {inst_16, bytes * 4u},          {pos_in, bytes},
                             {vel_in, bytes},       {up_xyz, 3 * sizeof(float)},    {cp16, 16 * sizeof(float)}};
    const ByteRange out[2] = {{pos_out, bytes}, {vel_out, bytes}};
    return outputs_check(fn, out, 0x3u, "", false, in, 6, kScenesSeenAlias, err);
}

// the eyes a per-eye kernel walks: [first_eye, first_eye + count) of a batch whose cameras and model matrices lie at cams and inst
static nbk::ScenesEyes scenes_eyes(uint32_t n, uint32_t first_eye, uint32_t count, const void *cams, const void *inst, uint32_t width)
{
    return {n, first_eye, count, width, (const float4 *)cams, (const float4 *)inst};
}

NB_EXPORT int nb_scenes_boids_seen_step_launch(const nb_boids_params *params, uint32_t scenes, uint32_t n, const void *cams_16,
                                               const void *inst_16, uint32_t width, const void *pos_in, const void *vel_in, void *pos_out,
                                               void *vel_out, void *stream)
{
    static const char fn[] = "nb_scenes_boids_seen_step_launch";
    const nb_boids_params p = boids_params_or_default(params);
    int rc = scenes_null_check(fn, {cams_16, inst_16, pos_in, vel_in, pos_out, vel_out}, &g_tls_error,
                               ": cams_16, inst_16 and the four record buffers must be non-null");
    if (rc == NB_OK) rc = scenes_vision_check(fn, scenes, n, width, nullptr, &g_tls_error);
    if (rc == NB_OK) rc = scenes_boids_params_check(fn, p, &g_tls_error);
    if (rc == NB_OK)
        rc = scenes_step_buffers_check(fn, (size_t)scenes * n, cams_16, inst_16, pos_in, vel_in, pos_out, vel_out, nullptr, nullptr, &g_tls_error);
    nbk::ScenesSeenArgs a{};
    uint32_t tile = 0;
    if (rc == NB_OK) rc = make_boids_args(p, n, 0, n, &a.c, &tile, &g_tls_error);
    if (rc == NB_OK) rc = device_for_launch(pos_in, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    a.eye = scenes_eyes(n, 0u, scenes * n, cams_16, inst_16, width);
    a.c.pos_in = (const float4 *)pos_in, a.c.vel_in = (const float4 *)vel_in, a.c.pos_out = (float4 *)pos_out, a.c.vel_out = (float4 *)vel_out;
    return launch_status(nbk::launch_scenes_boids_seen(a, (hipStream_t)stream), "nb: boids kernel launch failed (scene batch, seen form): ", &g_tls_error);
}

NB_EXPORT int nb_scenes_seen_launch(uint32_t scenes, uint32_t n, uint32_t first_eye, uint32_t count, const void *cams_16, const void *inst_16,
                                    uint32_t width, void *seen_count, void *seen_ids, void *stream)
{
    static const char fn[] = "nb_scenes_seen_launch";
    int rc = scenes_null_check(fn, {cams_16, inst_16}, &g_tls_error, ": cams_16 and inst_16 must be non-null");
    if (rc == NB_OK) rc = scenes_vision_check(fn, scenes, n, width, nullptr, &g_tls_error);
    if (rc == NB_OK) rc = scenes_aligned_check(fn, 16, {cams_16, inst_16}, "cams_16 and inst_16", &g_tls_error);
    if (rc == NB_OK) rc = scenes_eye_range_check(fn, scenes, n, first_eye, count, &g_tls_error);
    if (rc != NB_OK) return rc;
    const size_t matrices = (size_t)scenes * n * 16 * sizeof(float);
    const ByteRange in[2] = {{cams_16, matrices}, {inst_16, matrices}};
    const ByteRange out[2] = {{seen_count, (size_t)count * 4u}, {seen_ids, (size_t)count * width * 4u}};
    rc = outputs_check(fn, out, 0x3u, ": seen_count and seen_ids are both NULL", true, in, 2, kScenesSeenAlias, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (count == 0) return NB_OK;
    rc = device_for_launch(inst_16, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    nbk::ScenesSeenArgs a{};
    a.eye = scenes_eyes(n, first_eye, count, cams_16, inst_16, width);
    a.seen_count = (uint32_t *)seen_count, a.seen_ids = (uint32_t *)seen_ids;
    return launch_status(nbk::launch_scenes_seen(a, (hipStream_t)stream), "nb: seen kernel launch failed (scene batch): ", &g_tls_error);
}

// ---- gravity from located vision (DESIGN.md section 14.2): the stateless entries ----------------------------------------------------------
static const char kNoScenesLocatedOutputs[] = ": seen_count, seen_ids, seen_depth, seen_col and seen_rel are all NULL";

// the kernel's arguments but for its buffers: the eye set-up and the law's constants
static nbk::ScenesLocatedArgs scenes_located_args(const nb_params &p, const nbk::ScenesEyes &eye, const float *up_xyz, const float *cp16)
{
    nbk::ScenesLocatedArgs a{};
    a.eye = eye;
    a.ux = up_xyz[0], a.uy = up_xyz[1], a.uz = up_xyz[2];
    a.cp0 = cp16[0], a.cp10 = cp16[10], a.cp14 = cp16[14];
    a.dt = p.dt, a.G = p.G, a.bias = p.bias;
    return a;
}

NB_EXPORT int nb_scenes_nbody_located_step_launch(const nb_params *params, uint32_t scenes, uint32_t n, const void *cams_16,
                                                  const void *inst_16, const float *up_xyz, const float *cp16, uint32_t width,
                                                  const void *pos_in, const void *vel_in, void *pos_out, void *vel_out, void *stream)
{
    static const char fn[] = "nb_scenes_nbody_located_step_launch";
    const nb_params p = params_or_default(params);
    int rc = scenes_null_check(fn, {cams_16, inst_16, up_xyz, cp16, pos_in, vel_in, pos_out, vel_out}, &g_tls_error);
    if (rc == NB_OK) rc = scenes_vision_check(fn, scenes, n, width, cp16, &g_tls_error);
    const size_t records = (size_t)scenes * n;
    if (rc == NB_OK) rc = scenes_step_buffers_check(fn, records, cams_16, inst_16, pos_in, vel_in, pos_out, vel_out, up_xyz, cp16, &g_tls_error);
    if (rc == NB_OK) rc = device_for_launch(pos_in, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    nbk::ScenesLocatedArgs a = scenes_located_args(p, scenes_eyes(n, 0u, (uint32_t)records, cams_16, inst_16, width), up_xyz, cp16);
    a.pos_in = (const float4 *)pos_in, a.vel_in = (const float4 *)vel_in, a.pos_out = (float4 *)pos_out, a.vel_out = (float4 *)vel_out;
    return launch_status(nbk::launch_scenes_nbody_located(a, (hipStream_t)stream),
                         "nb: gravity kernel launch failed (scene batch, located form): ", &g_tls_error);
}

NB_EXPORT int nb_scenes_located_launch(uint32_t scenes, uint32_t n, uint32_t first_eye, uint32_t count, const void *cams_16,
                                       const void *inst_16, const void *vel_in, const float *up_xyz, const float *cp16, uint32_t width,
                                       void *seen_count, void *seen_ids, void *seen_depth, void *seen_col, void *seen_rel, void *stream)
{
    static const char fn[] = "nb_scenes_located_launch";
    int rc = scenes_null_check(fn, {cams_16, inst_16, vel_in, up_xyz, cp16}, &g_tls_error);
    if (rc == NB_OK) rc = scenes_vision_check(fn, scenes, n, width, cp16, &g_tls_error);
    if (rc == NB_OK) rc = scenes_aligned_check(fn, 16, {cams_16, inst_16, vel_in, seen_rel}, "cams_16, inst_16, vel_in and seen_rel", &g_tls_error);
    if (rc == NB_OK) rc = scenes_eye_range_check(fn, scenes, n, first_eye, count, &g_tls_error);
    if (rc != NB_OK) return rc;
    const size_t records = (size_t)scenes * n, cells = (size_t)count * width;
    const ByteRange in[5] = {{cams_16, records * 64u}, {inst_16, records * 64u}, {vel_in, records * 16u}, {up_xyz, 3 * sizeof(float)},
                             {cp16, 16 * sizeof(float)}};
    const ByteRange out[5] = {{seen_count, (size_t)count * 4u}, {seen_ids, cells * 4u}, {seen_depth, cells * 4u}, {seen_col, cells * 4u},
                              {seen_rel, cells * 16u}};
    rc = outputs_check(fn, out, 0x1Fu, kNoScenesLocatedOutputs, true, in, 5, kScenesSeenAlias, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (count == 0) return NB_OK;
    rc = device_for_launch(inst_16, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    nbk::ScenesLocatedArgs a = scenes_located_args(nb_params{}, scenes_eyes(n, first_eye, count, cams_16, inst_16, width), up_xyz, cp16);
    a.vel_in = (const float4 *)vel_in;
    a.seen_count = (uint32_t *)seen_count, a.seen_ids = (uint32_t *)seen_ids, a.seen_depth = (uint32_t *)seen_depth;
    a.seen_col = (uint32_t *)seen_col, a.seen_rel = (float4 *)seen_rel;
    return launch_status(nbk::launch_scenes_located(a, (hipStream_t)stream), "nb: located kernel launch failed (scene batch): ", &g_tls_error);
}

// ---- the context --------------------------------------------------------------------------------------------------------------------------
struct ScenesPolicyShape {                   // a policy's (F, H) and the limit of its outputs; recurrent (section 14.8): R4's limit too
    uint32_t features = 0, hidden = 0;
    float accel_limit = 0.f;
    bool recurrent = false;
    float memory_limit = 0.f;
    size_t floats() const { return recurrent ? nbk::policy_recurrent_floats(features, hidden) : nbk::policy_floats(features, hidden); }
};

struct nb_scenes {
    uint32_t scenes = 0, n = 0;
    nb_params p{};
    hipStream_t stream = nullptr;
    DeviceBuffer<float4> pos, vel;           // scenes * n records each, stepped in place
    DeviceBuffer<float> stage;               // 6 * scenes * n floats: the stride-3 arrays of an upload or a download
    DeviceBuffer<float4> inst;               // 4 * scenes * n records, allocated on first use
    DeviceBuffer<float4> pos_alt, vel_alt;   // the seen boids step's outputs, allocated on first use: it swaps them with pos and vel
    DeviceBuffer<float4> cams;               // 4 * scenes * n records, likewise: every body's eye camera
    DeviceBuffer<uint32_t> seen_count, seen_ids;   // nb_scenes_eyes_seen's lists for one range of scenes, likewise and grown on demand
    DeviceBuffer<uint32_t> seen_depth, seen_col;   // nb_scenes_eyes_located's further lists, likewise: depth bits and columns
    DeviceBuffer<uint32_t> seen_rel;               // and its located points, four words a slot
    DeviceBuffer<float> policy;                    // nb_scenes_set_policy's weights: policies * nb_policy_floats floats
    ScenesPolicyShape pol;                         // their shape
    uint32_t policies = 0;                         // 0: no policy set
    DeviceBuffer<uint32_t> pol_feat, pol_act;      // nb_scenes_eyes_policy's features and outputs for one range of scenes, grown on demand
    DeviceBuffer<uint32_t> pol_mem;                // nb_scenes_eyes_policy_memory's next memory for one range of scenes, likewise
    DeviceBuffer<float> memory;                    // a recurrent policy's memory (R2): scenes * n * hidden floats, stepped in place
    size_t memory_words = 0;                       // the floats of it in use; 0: no recurrent policy or search is set
    DeviceBuffer<nbk::SceneScore> score;           // nb_scenes_set_score's records, one a scene
    nb_score_params sp{};                          // its parameters
    bool score_set = false;
    DeviceBuffer<float> es_mean;                   // nb_scenes_es_set's mean: es_pol.floats() floats, updated in place
    DeviceBuffer<uint32_t> es_rank;                // what the last nb_scenes_es_update left: scenes ranks,
    DeviceBuffer<float> es_fitness;                // scenes fitnesses
    DeviceBuffer<uint32_t> es_report;              // and the four words of nb_es_report
    nb_es_params ep{};                             // its parameters; the shape of the population's policies
    ScenesPolicyShape es_pol;
    uint32_t es_generation = 0;
    bool es_set = false, es_updated = false;
    DeviceBuffer<float4> pos_kept, vel_kept;       // nb_scenes_keep's copy of pos and vel
    uint64_t steps_kept = 0;                       // and of the step counter
    bool kept = false;
    bool uploaded = false;
    uint64_t steps = 0;
    std::string err;
};

NB_EXPORT const char *nb_scenes_last_error(const nb_scenes *ctx) { return ctx ? ctx->err.c_str() : g_tls_error.c_str(); }

NB_EXPORT void nb_scenes_destroy(nb_scenes *ctx)
{
    if (!ctx) return;
    const hipStream_t stream = ctx->stream;
    if (stream) (void)hipStreamSynchronize(stream);
    delete ctx;  // frees its buffers: behind the wait, in front of the stream's end
    if (stream) (void)hipStreamDestroy(stream);
}

static int scenes_create_impl(nb_scenes *c)
{
    const size_t records = (size_t)c->scenes * c->n;
    NB_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    NB_HIP(c, c->pos.reserve(records));
    NB_HIP(c, c->vel.reserve(records));
    NB_HIP(c, c->stage.reserve(records * 6));
    return NB_OK;
}

NB_EXPORT int nb_scenes_create(uint32_t scenes, uint32_t n, const nb_params *params, nb_scenes **out)
{
    static const char fn[] = "nb_scenes_create";
    int rc = scenes_null_check(fn, {out}, &g_tls_error, ": out is null");
    if (rc != NB_OK) return rc;
    *out = nullptr;
    const nb_params p = params_or_default(params);
    rc = scenes_shape_check(fn, scenes, n, &g_tls_error);
    if (rc == NB_OK) rc = scenes_params_check(fn, p, &g_tls_error);
    if (rc == NB_OK) rc = check_device(&g_tls_error);
    if (rc != NB_OK) return rc;
    nb_scenes *c = new (std::nothrow) nb_scenes();
    if (!c) {
        g_tls_error = std::string(fn) + ": out of host memory";
        return NB_ERR_ALLOC;
    }
    c->scenes = scenes, c->n = n, c->p = p;
    rc = scenes_create_impl(c);
    if (rc != NB_OK) {
        g_tls_error = c->err;
        nb_scenes_destroy(c);
        return rc;
    }
    *out = c;
    return NB_OK;
}

NB_EXPORT int nb_scenes_upload(nb_scenes *ctx, const float *pos_xyz, const float *vel_xyz)
{
    int rc = ctx_check(ctx, "nb_scenes_upload");
    if (rc == NB_OK) rc = scenes_null_check("nb_scenes_upload", {pos_xyz, vel_xyz}, &ctx->err, ": null array");
    if (rc != NB_OK) return rc;
    const size_t records = (size_t)ctx->scenes * ctx->n, bytes = records * 3 * sizeof(float);
    NB_HIP(ctx, hipMemcpyAsync(ctx->stage.p, pos_xyz, bytes, hipMemcpyHostToDevice, ctx->stream));
    NB_HIP(ctx, hipMemcpyAsync(ctx->stage.p + 3 * records, vel_xyz, bytes, hipMemcpyHostToDevice, ctx->stream));
    NB_HIP(ctx, nbk::launch_import((uint32_t)records, ctx->stage.p, ctx->stage.p + 3 * records, ctx->pos.p, ctx->vel.p, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the host arrays are not retained
    ctx->uploaded = true;
    ctx->steps = 0;
    return NB_OK;
}

NB_EXPORT int nb_scenes_step(nb_scenes *ctx, uint32_t k)
{
    int rc = ctx_check(ctx, "nb_scenes_step", kCallScenesUpload);
    if (rc != NB_OK) return rc;
    nbk::ScenesNbodyArgs a;
    rc = scenes_nbody_args(ctx->p, ctx->scenes, ctx->n, k, ctx->pos.p, ctx->vel.p, &a, &ctx->err);
    if (rc != NB_OK) return rc;
    if (k == 0) return NB_OK;
    RoctxRange range("nb_scenes_step");
    NB_HIP(ctx, nbk::launch_scenes_nbody(a, ctx->stream));
    ctx->steps += k;
    return NB_OK;
}

NB_EXPORT int nb_scenes_step_boids(nb_scenes *ctx, uint32_t k, const nb_boids_params *params)
{
    static const char fn[] = "nb_scenes_step_boids";
    int rc = ctx_check(ctx, fn);
    if (rc != NB_OK) return rc;
    const nb_boids_params p = boids_params_or_default(params);
    rc = scenes_boids_params_check(fn, p, &ctx->err);
    if (rc == NB_OK) rc = ctx_check(ctx, fn, kCallScenesUpload);
    nbk::BoidsArgs c;
    uint32_t tile = 0;
    if (rc == NB_OK) rc = make_boids_args(p, ctx->n, 0, ctx->n, &c, &tile, &ctx->err);
    if (rc != NB_OK) return rc;
    if (k == 0) return NB_OK;
    RoctxRange range(fn);
    NB_HIP(ctx, nbk::launch_scenes_boids(c, ctx->pos.p, ctx->vel.p, ctx->scenes, k, ctx->stream));
    ctx->steps += k;
    return NB_OK;
}

// the eye set-up of the context's two seen entries: there, and the width
static int scenes_eye_setup_check(nb_scenes *ctx, const char *fn, const float *up_xyz, const float *cp16, uint32_t width)
{
    const int rc = scenes_null_check(fn, {up_xyz, cp16}, &ctx->err);
    return rc != NB_OK ? rc : scenes_width_check(fn, width, &ctx->err);
}

// a check of the context's state: `have`, or NB_ERR_STATE with `tail` behind the entry's name
static int scenes_state_check(nb_scenes *ctx, const char *fn, bool have, const char *tail)
{
    if (!have) {
        ctx->err = std::string(fn) + tail;
        return NB_ERR_STATE;
    }
    return NB_OK;
}

// scenes [first_scene, first_scene + scene_count) lie in the context's batch
static int scenes_range_check(nb_scenes *ctx, const char *fn, uint32_t first_scene, uint32_t scene_count)
{
    if ((uint64_t)first_scene + scene_count > ctx->scenes) {
        ctx->err = std::string(fn) + ": scenes [first_scene, first_scene + scene_count) exceed the batch";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// eyes [first_eye, first_eye + count) of the context's batch, as scenes_stage_eyes leaves their cameras and matrices
static nbk::ScenesEyes scenes_eyes(const nb_scenes *ctx, uint32_t first_eye, uint32_t count, uint32_t width)
{
    return scenes_eyes(ctx->n, first_eye, count, ctx->cams.p, ctx->inst.p, width);
}

// the model matrices and the eye cameras of every body of the current state, on the context's stream
static int scenes_stage_eyes(nb_scenes *ctx, const float *up_xyz, const float *cp16)
{
    const size_t records = (size_t)ctx->scenes * ctx->n;
    NB_HIP(ctx, ctx->cams.reserve(records * 4));
    NB_HIP(ctx, launch_matrices((uint32_t)records, ctx->pos.p, ctx->vel.p, &ctx->inst, ctx->stream));
    NB_HIP(ctx, nbk::launch_cameras((uint32_t)records, ctx->pos.p, ctx->vel.p, up_xyz, cp16, ctx->cams.p, ctx->stream));
    return NB_OK;
}

// k steps of a controller that sees (sections 14.1, 14.2), the entry's checks behind it: per step the eyes of the current state, ONE
// fused kernel -- launch(ctx) issues it from pos / vel into pos_alt / vel_alt and returns a status -- and the swap
template <typename Launch>
static int scenes_vision_step(nb_scenes *ctx, const char *fn, uint32_t k, const float *up_xyz, const float *cp16, Launch launch)
{
    if (k == 0) return NB_OK;
    const size_t records = (size_t)ctx->scenes * ctx->n;
    NB_HIP(ctx, ctx->pos_alt.reserve(records));
    NB_HIP(ctx, ctx->vel_alt.reserve(records));
    RoctxRange range(fn);
    for (uint32_t s = 0; s < k; ++s) {
        int rc = scenes_stage_eyes(ctx, up_xyz, cp16);
        if (rc == NB_OK) rc = launch(ctx);
        if (rc != NB_OK) return rc;
        ctx->pos.swap(ctx->pos_alt);
        ctx->vel.swap(ctx->vel_alt);
        ctx->steps++;
    }
    return NB_OK;
}

// One output of nb_scenes_eyes_seen / nb_scenes_eyes_located: the caller's array (NULL: not asked for), the context's buffer behind
// it and the 4-byte words an eye has in it.  Row 0 of an entry's table is the count, which the kernel writes whether asked for or not.
struct ScenesEyesOutput {
    void *host;
    DeviceBuffer<uint32_t> *dev;
    size_t words;
};

// The sets of scenes [first_scene, first_scene + scene_count), the entry's eye set-up checked: the range, the outputs (none_msg: none is
// asked for) and the state; then the eyes staged once and as many scenes per launch as keep the outputs asked for (4 bytes of count
// an eye and 4 bytes a word) at or below 64 MiB, one at least.  launch(ctx, first_eye, count) issues the kernel for one such chunk
// into the context's buffers and returns a status.
template <int N, typename Launch>
static int scenes_eyes_download(nb_scenes *ctx, const char *fn, uint32_t first_scene, uint32_t scene_count, const float *up_xyz,
                                const float *cp16, const ScenesEyesOutput (&out)[N], const char *none_msg, Launch launch)
{
    int rc = scenes_range_check(ctx, fn, first_scene, scene_count);
    if (rc != NB_OK) return rc;
    const ByteRange in[2] = {{up_xyz, 3 * sizeof(float)}, {cp16, 16 * sizeof(float)}};
    ByteRange user[N];
    for (int r = 0; r < N; ++r) user[r] = {out[r].host, (size_t)scene_count * ctx->n * out[r].words * 4u};
    rc = outputs_check(fn, user, (1u << N) - 1u, none_msg, false, in, 2, kScenesSeenAlias, &ctx->err);
    if (rc == NB_OK) rc = ctx_check(ctx, fn, kCallScenesUpload);
    if (rc != NB_OK) return rc;
    if (scene_count == 0) return NB_OK;
    const auto wanted = [&out](int r) { return r == 0 || out[r].host; };
    size_t per_eye = 0;
    for (int r = 0; r < N; ++r) per_eye += wanted(r) ? out[r].words * 4u : 0u;
    const uint32_t per = (uint32_t)std::min<size_t>(scene_count, std::max<size_t>(1, ((size_t)64 << 20) / (ctx->n * per_eye)));
    for (int r = 0; r < N; ++r)
        if (wanted(r)) NB_HIP(ctx, out[r].dev->reserve((size_t)per * ctx->n * out[r].words));
    rc = scenes_stage_eyes(ctx, up_xyz, cp16);
    if (rc != NB_OK) return rc;
    for (uint32_t s0 = 0; s0 < scene_count; s0 += per) {
        const uint32_t cnt = std::min(per, scene_count - s0) * ctx->n;
        const size_t at = (size_t)s0 * ctx->n;
        rc = launch(ctx, (first_scene + s0) * ctx->n, cnt);
        if (rc != NB_OK) return rc;
        for (int r = 0; r < N; ++r)
            if (out[r].host)
                NB_HIP(ctx, hipMemcpyAsync((uint32_t *)out[r].host + at * out[r].words, out[r].dev->p, cnt * out[r].words * 4u,
                                           hipMemcpyDeviceToHost, ctx->stream));
    }
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NB_OK;
}

NB_EXPORT int nb_scenes_step_boids_seen(nb_scenes *ctx, uint32_t k, const nb_boids_params *params, const float *up_xyz, const float *cp16,
                                        uint32_t width)
{
    static const char fn[] = "nb_scenes_step_boids_seen";
    int rc = ctx_check(ctx, fn);
    if (rc != NB_OK) return rc;
    const nb_boids_params p = boids_params_or_default(params);
    rc = scenes_eye_setup_check(ctx, fn, up_xyz, cp16, width);
    if (rc == NB_OK) rc = scenes_boids_params_check(fn, p, &ctx->err);
    if (rc == NB_OK) rc = ctx_check(ctx, fn, kCallScenesUpload);
    nbk::ScenesSeenArgs a{};
    uint32_t tile = 0;
    if (rc == NB_OK) rc = make_boids_args(p, ctx->n, 0, ctx->n, &a.c, &tile, &ctx->err);
    if (rc != NB_OK) return rc;
    return scenes_vision_step(ctx, fn, k, up_xyz, cp16, [&a, width](nb_scenes *ctx) -> int {
        a.eye = scenes_eyes(ctx, 0u, ctx->scenes * ctx->n, width);
        a.c.pos_in = ctx->pos.p, a.c.vel_in = ctx->vel.p, a.c.pos_out = ctx->pos_alt.p, a.c.vel_out = ctx->vel_alt.p;
        NB_HIP(ctx, nbk::launch_scenes_boids_seen(a, ctx->stream));
        return NB_OK;
    });
}

NB_EXPORT int nb_scenes_eyes_seen(nb_scenes *ctx, uint32_t first_scene, uint32_t scene_count, const float *up_xyz, const float *cp16,
                                  uint32_t width, uint32_t *seen_count, uint32_t *seen_ids)
{
    static const char fn[] = "nb_scenes_eyes_seen";
    int rc = ctx_check(ctx, fn);
    if (rc != NB_OK) return rc;
    rc = scenes_eye_setup_check(ctx, fn, up_xyz, cp16, width);
    if (rc != NB_OK) return rc;
    const ScenesEyesOutput lists[2] = {{seen_count, &ctx->seen_count, 1}, {seen_ids, &ctx->seen_ids, width}};
    const auto launch = [=](nb_scenes *ctx, uint32_t first_eye, uint32_t cnt) -> int {
        nbk::ScenesSeenArgs a{};
        a.eye = scenes_eyes(ctx, first_eye, cnt, width);
        a.seen_count = ctx->seen_count.p, a.seen_ids = seen_ids ? ctx->seen_ids.p : nullptr;
        NB_HIP(ctx, nbk::launch_scenes_seen(a, ctx->stream));
        return NB_OK;
    };
    return scenes_eyes_download(ctx, fn, first_scene, scene_count, up_xyz, cp16, lists, ": seen_count and seen_ids are both NULL", launch);
}

// ---- gravity from located vision (DESIGN.md section 14.2): the context's entries ----------------------------------------------------------
NB_EXPORT int nb_scenes_step_nbody_located(nb_scenes *ctx, uint32_t k, const float *up_xyz, const float *cp16, uint32_t width)
{
    static const char fn[] = "nb_scenes_step_nbody_located";
    int rc = ctx_check(ctx, fn);
    if (rc != NB_OK) return rc;
    rc = scenes_eye_setup_check(ctx, fn, up_xyz, cp16, width);
    if (rc == NB_OK) rc = located_cp_check(fn, cp16, &ctx->err);
    if (rc == NB_OK) rc = ctx_check(ctx, fn, kCallScenesUpload);
    if (rc != NB_OK) return rc;
    return scenes_vision_step(ctx, fn, k, up_xyz, cp16, [=](nb_scenes *ctx) -> int {
        nbk::ScenesLocatedArgs a = scenes_located_args(ctx->p, scenes_eyes(ctx, 0u, ctx->scenes * ctx->n, width), up_xyz, cp16);
        a.pos_in = ctx->pos.p, a.vel_in = ctx->vel.p, a.pos_out = ctx->pos_alt.p, a.vel_out = ctx->vel_alt.p;
        NB_HIP(ctx, nbk::launch_scenes_nbody_located(a, ctx->stream));
        return NB_OK;
    });
}

NB_EXPORT int nb_scenes_eyes_located(nb_scenes *ctx, uint32_t first_scene, uint32_t scene_count, const float *up_xyz, const float *cp16,
                                     uint32_t width, uint32_t *seen_count, uint32_t *seen_ids, float *seen_depth, uint32_t *seen_col,
                                     float *seen_rel)
{
    static const char fn[] = "nb_scenes_eyes_located";
    int rc = ctx_check(ctx, fn);
    if (rc != NB_OK) return rc;
    rc = scenes_eye_setup_check(ctx, fn, up_xyz, cp16, width);
    if (rc == NB_OK) rc = located_cp_check(fn, cp16, &ctx->err);
    if (rc != NB_OK) return rc;
    const ScenesEyesOutput lists[5] = {{seen_count, &ctx->seen_count, 1},     {seen_ids, &ctx->seen_ids, width},
                                       {seen_depth, &ctx->seen_depth, width}, {seen_col, &ctx->seen_col, width},
                                       {seen_rel, &ctx->seen_rel, (size_t)width * 4u}};   // 28 width + 4 bytes an eye with all five
    const auto launch = [=](nb_scenes *ctx, uint32_t first_eye, uint32_t cnt) -> int {
        nbk::ScenesLocatedArgs a = scenes_located_args(ctx->p, scenes_eyes(ctx, first_eye, cnt, width), up_xyz, cp16);
        a.vel_in = ctx->vel.p;
        a.seen_count = ctx->seen_count.p, a.seen_ids = seen_ids ? ctx->seen_ids.p : nullptr;
        a.seen_depth = seen_depth ? ctx->seen_depth.p : nullptr, a.seen_col = seen_col ? ctx->seen_col.p : nullptr;
        a.seen_rel = seen_rel ? (float4 *)ctx->seen_rel.p : nullptr;
        NB_HIP(ctx, nbk::launch_scenes_located(a, ctx->stream));
        return NB_OK;
    };
    return scenes_eyes_download(ctx, fn, first_scene, scene_count, up_xyz, cp16, lists, kNoScenesLocatedOutputs, launch);
}

// ---- a neural policy over each eye row (DESIGN.md section 14.4) ---------------------------------------------------------------------------
static_assert(NB_POLICY_MAX_FEATURES == nbk::kPolicyMaxFeatures && NB_POLICY_MAX_HIDDEN == nbk::kPolicyMaxHidden, "the header's limits are the kernels'");
static const char kNoPolicyOutputs[] = ": feat_out and act_out are both NULL";
static const char kCallSetPolicy[] = ": no policy set (call nb_scenes_set_policy first)";

NB_EXPORT size_t nb_policy_floats(uint32_t features, uint32_t hidden)
{
    if (features == 0 || features > NB_POLICY_MAX_FEATURES || hidden == 0 || hidden > NB_POLICY_MAX_HIDDEN) return 0;
    return nbk::policy_floats(features, hidden);
}

// the shape of a policy against the eye's width (0: the entry has no width yet), the number of policies against the batch's scenes
// and the limit
static int policy_check(const char *fn, uint32_t features, uint32_t hidden, uint32_t width, uint32_t policies, uint32_t scenes,
                        float accel_limit, std::string *err)
{
    if (features == 0 || features > NB_POLICY_MAX_FEATURES) {
        *err = std::string(fn) + ": features must be 1 .. NB_POLICY_MAX_FEATURES (256)";
        return NB_ERR_INVALID;
    }
    if (hidden == 0 || hidden > NB_POLICY_MAX_HIDDEN) {
        *err = std::string(fn) + ": hidden must be 1 .. NB_POLICY_MAX_HIDDEN (64)";
        return NB_ERR_INVALID;
    }
    if (width % features != 0) {
        *err = std::string(fn) + ": width must be a multiple of features";
        return NB_ERR_INVALID;
    }
    if (policies != 1 && policies != scenes) {
        *err = std::string(fn) + ": policies must be 1 or scenes";
        return NB_ERR_INVALID;
    }
    if (!(accel_limit >= 0.0f)) {
        *err = std::string(fn) + ": accel_limit must be at least 0 (+inf: no limit)";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// the kernel's arguments but for its buffers: the eye set-up and the policies
static nbk::ScenesPolicyArgs scenes_policy_args(const nbk::ScenesEyes &eye, const ScenesPolicyShape &shape, uint32_t policies, const void *weights)
{
    nbk::ScenesPolicyArgs a{};
    a.eye = eye;
    a.features = shape.features, a.hidden = shape.hidden;
    a.stride = policies == 1 ? 0u : (uint32_t)nbk::policy_floats(shape.features, shape.hidden);
    a.weights = (const float *)weights, a.limit = shape.accel_limit;
    return a;
}

NB_EXPORT int nb_scenes_policy_step_launch(const nb_params *params, uint32_t scenes, uint32_t n, const void *cams_16, const void *inst_16,
                                           uint32_t width, const float *up_xyz, uint32_t features, uint32_t hidden, uint32_t policies,
                                           const void *weights, float accel_limit, const void *pos_in, const void *vel_in, void *pos_out,
                                           void *vel_out, void *stream)
{
    static const char fn[] = "nb_scenes_policy_step_launch";
    const nb_params p = params_or_default(params);
    int rc = scenes_null_check(fn, {cams_16, inst_16, up_xyz, weights, pos_in, vel_in, pos_out, vel_out}, &g_tls_error);
    if (rc == NB_OK) rc = scenes_vision_check(fn, scenes, n, width, nullptr, &g_tls_error);
    if (rc == NB_OK) rc = policy_check(fn, features, hidden, width, policies, scenes, accel_limit, &g_tls_error);
    if (rc == NB_OK) rc = scenes_params_check(fn, p, &g_tls_error);
    if (rc == NB_OK) rc = scenes_aligned_check(fn, 4, {weights}, "weights", &g_tls_error);
    const size_t records = (size_t)scenes * n;
    if (rc == NB_OK) rc = scenes_step_buffers_check(fn, records, cams_16, inst_16, pos_in, vel_in, pos_out, vel_out, up_xyz, nullptr, &g_tls_error);
    if (rc != NB_OK) return rc;
    const size_t wbytes = (size_t)policies * nbk::policy_floats(features, hidden) * sizeof(float);
    if (ranges_overlap(pos_out, records * sizeof(float4), weights, wbytes) || ranges_overlap(vel_out, records * sizeof(float4), weights, wbytes)) {
        g_tls_error = std::string(fn) + kScenesSeenAlias;
        return NB_ERR_INVALID;
    }
    rc = device_for_launch(pos_in, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    nbk::ScenesPolicyArgs a =
        scenes_policy_args(scenes_eyes(n, 0u, (uint32_t)records, cams_16, inst_16, width), {features, hidden, accel_limit}, policies, weights);
    a.pos_in = (const float4 *)pos_in, a.vel_in = (const float4 *)vel_in, a.pos_out = (float4 *)pos_out, a.vel_out = (float4 *)vel_out;
    a.ux = up_xyz[0], a.uy = up_xyz[1], a.uz = up_xyz[2], a.dt = p.dt;
    return launch_status(nbk::launch_scenes_policy(a, (hipStream_t)stream), "nb: policy kernel launch failed (scene batch): ", &g_tls_error);
}

NB_EXPORT int nb_scenes_policy_observe_launch(uint32_t scenes, uint32_t n, uint32_t first_eye, uint32_t count, const void *cams_16,
                                              const void *inst_16, uint32_t width, uint32_t features, uint32_t hidden, uint32_t policies,
                                              const void *weights, float accel_limit, void *feat_out, void *act_out, void *stream)
{
    static const char fn[] = "nb_scenes_policy_observe_launch";
    int rc = scenes_null_check(fn, {cams_16, inst_16, weights}, &g_tls_error);
    if (rc == NB_OK) rc = scenes_vision_check(fn, scenes, n, width, nullptr, &g_tls_error);
    if (rc == NB_OK) rc = policy_check(fn, features, hidden, width, policies, scenes, accel_limit, &g_tls_error);
    if (rc == NB_OK) rc = scenes_aligned_check(fn, 4, {weights}, "weights", &g_tls_error);
    if (rc == NB_OK) rc = scenes_aligned_check(fn, 16, {cams_16, inst_16}, "cams_16 and inst_16", &g_tls_error);
    if (rc == NB_OK) rc = scenes_eye_range_check(fn, scenes, n, first_eye, count, &g_tls_error);
    if (rc != NB_OK) return rc;
    const size_t matrices = (size_t)scenes * n * 16 * sizeof(float);
    const ByteRange in[3] = {{cams_16, matrices}, {inst_16, matrices}, {weights, (size_t)policies * nbk::policy_floats(features, hidden) * sizeof(float)}};
    const ByteRange out[2] = {{feat_out, (size_t)count * features * 4u}, {act_out, (size_t)count * 8u}};
    rc = outputs_check(fn, out, 0x3u, kNoPolicyOutputs, true, in, 3, kScenesSeenAlias, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (count == 0) return NB_OK;
    rc = device_for_launch(inst_16, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    nbk::ScenesPolicyArgs a =
        scenes_policy_args(scenes_eyes(n, first_eye, count, cams_16, inst_16, width), {features, hidden, accel_limit}, policies, weights);
    a.feat_out = (uint32_t *)feat_out, a.act_out = (uint32_t *)act_out;
    return launch_status(nbk::launch_scenes_policy_observe(a, (hipStream_t)stream), "nb: policy kernel launch failed (scene batch, observe form): ",
                         &g_tls_error);
}

// ---- a recurrent policy with per-body memory (DESIGN.md section 14.8): the stateless entries ---------------------------------------------
static const char kNoPolicyMemoryOutputs[] = ": feat_out, act_out and mem_out are all NULL";
static const char kCallSetPolicyRecurrent[] = ": no recurrent policy set (call nb_scenes_set_policy_recurrent first)";
static_assert(NB_ES_MAX_FLOATS == nbk::policy_recurrent_floats(NB_POLICY_MAX_FEATURES, NB_POLICY_MAX_HIDDEN), "the longest mean is the largest recurrent policy");

NB_EXPORT size_t nb_policy_recurrent_floats(uint32_t features, uint32_t hidden)
{
    if (features == 0 || features > NB_POLICY_MAX_FEATURES || hidden == 0 || hidden > NB_POLICY_MAX_HIDDEN) return 0;
    return nbk::policy_recurrent_floats(features, hidden);
}

// policy_check, then R4's limit
static int policy_recurrent_check(const char *fn, uint32_t features, uint32_t hidden, uint32_t width, uint32_t policies, uint32_t scenes,
                                  float accel_limit, float memory_limit, std::string *err)
{
    const int rc = policy_check(fn, features, hidden, width, policies, scenes, accel_limit, err);
    if (rc != NB_OK) return rc;
    if (!(memory_limit >= 0.0f)) {
        *err = std::string(fn) + ": memory_limit must be at least 0 (+inf: no limit)";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// the recurrent kernel's arguments but for its buffers: scenes_policy_args with the longer policies, and R4's limit
static nbk::ScenesPolicyRecurrentArgs scenes_policy_recurrent_args(const nbk::ScenesEyes &eye, const ScenesPolicyShape &shape, uint32_t policies,
                                                                   const void *weights)
{
    nbk::ScenesPolicyRecurrentArgs a{};
    a.p = scenes_policy_args(eye, shape, policies, weights);
    a.p.stride = policies == 1 ? 0u : (uint32_t)nbk::policy_recurrent_floats(shape.features, shape.hidden);
    a.mem_limit = shape.memory_limit;
    return a;
}

NB_EXPORT int nb_scenes_policy_recurrent_step_launch(const nb_params *params, uint32_t scenes, uint32_t n, const void *cams_16,
                                                     const void *inst_16, uint32_t width, const float *up_xyz, uint32_t features,
                                                     uint32_t hidden, uint32_t policies, const void *weights, float accel_limit,
                                                     float memory_limit, const void *pos_in, const void *vel_in, const void *mem_in,
                                                     void *pos_out, void *vel_out, void *mem_out, void *stream)
{
    static const char fn[] = "nb_scenes_policy_recurrent_step_launch";
    const nb_params p = params_or_default(params);
    int rc = scenes_null_check(fn, {cams_16, inst_16, up_xyz, weights, pos_in, vel_in, mem_in, pos_out, vel_out, mem_out}, &g_tls_error);
    if (rc == NB_OK) rc = scenes_vision_check(fn, scenes, n, width, nullptr, &g_tls_error);
    if (rc == NB_OK) rc = policy_recurrent_check(fn, features, hidden, width, policies, scenes, accel_limit, memory_limit, &g_tls_error);
    if (rc == NB_OK) rc = scenes_params_check(fn, p, &g_tls_error);
    if (rc == NB_OK) rc = scenes_aligned_check(fn, 4, {weights}, "weights", &g_tls_error);
    if (rc == NB_OK) rc = scenes_aligned_check(fn, 4, {mem_in, mem_out}, "mem_in and mem_out", &g_tls_error);
    const size_t records = (size_t)scenes * n;
    if (rc == NB_OK) rc = scenes_step_buffers_check(fn, records, cams_16, inst_16, pos_in, vel_in, pos_out, vel_out, up_xyz, nullptr, &g_tls_error);
    if (rc != NB_OK) return rc;
    const size_t wbytes = (size_t)policies * nbk::policy_recurrent_floats(features, hidden) * sizeof(float);
    const size_t mbytes = records * hidden * sizeof(float), rbytes = records * sizeof(float4);
    const bool in_place = mem_out == mem_in;   // R7: an eye reads and writes only its own words
    if (!in_place && ranges_overlap(mem_out, mbytes, mem_in, mbytes)) {
        g_tls_error = std::string(fn) + ": mem_out must be mem_in itself or clear of it";
        return NB_ERR_INVALID;
    }
    const ByteRange in[7] = {{cams_16, rbytes * 4u}, {inst_16, rbytes * 4u}, {pos_in, rbytes}, {vel_in, rbytes}, {weights, wbytes},
                             {in_place ? nullptr : mem_in, mbytes}, {up_xyz, 3 * sizeof(float)}};
    const ByteRange out[3] = {{pos_out, rbytes}, {vel_out, rbytes}, {mem_out, mbytes}};
    rc = outputs_check(fn, out, 0x7u, "", false, in, 7, kScenesSeenAlias, &g_tls_error);
    if (rc != NB_OK) return rc;
    rc = device_for_launch(pos_in, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    ScenesPolicyShape shape{features, hidden, accel_limit, true, memory_limit};
    nbk::ScenesPolicyRecurrentArgs a = scenes_policy_recurrent_args(scenes_eyes(n, 0u, (uint32_t)records, cams_16, inst_16, width), shape, policies, weights);
    a.p.pos_in = (const float4 *)pos_in, a.p.vel_in = (const float4 *)vel_in, a.p.pos_out = (float4 *)pos_out, a.p.vel_out = (float4 *)vel_out;
    a.p.ux = up_xyz[0], a.p.uy = up_xyz[1], a.p.uz = up_xyz[2], a.p.dt = p.dt;
    a.mem_in = (const float *)mem_in, a.mem_out = (float *)mem_out;
    return launch_status(nbk::launch_scenes_policy_recurrent(a, (hipStream_t)stream), "nb: recurrent policy kernel launch failed (scene batch): ",
                         &g_tls_error);
}

NB_EXPORT int nb_scenes_policy_recurrent_observe_launch(uint32_t scenes, uint32_t n, uint32_t first_eye, uint32_t count, const void *cams_16,
                                                        const void *inst_16, uint32_t width, uint32_t features, uint32_t hidden,
                                                        uint32_t policies, const void *weights, float accel_limit, float memory_limit,
                                                        const void *mem, void *feat_out, void *act_out, void *mem_out, void *stream)
{
    static const char fn[] = "nb_scenes_policy_recurrent_observe_launch";
    int rc = scenes_null_check(fn, {cams_16, inst_16, weights, mem}, &g_tls_error);
    if (rc == NB_OK) rc = scenes_vision_check(fn, scenes, n, width, nullptr, &g_tls_error);
    if (rc == NB_OK) rc = policy_recurrent_check(fn, features, hidden, width, policies, scenes, accel_limit, memory_limit, &g_tls_error);
    if (rc == NB_OK) rc = scenes_aligned_check(fn, 4, {weights}, "weights", &g_tls_error);
    if (rc == NB_OK) rc = scenes_aligned_check(fn, 4, {mem}, "mem", &g_tls_error);
    if (rc == NB_OK) rc = scenes_aligned_check(fn, 16, {cams_16, inst_16}, "cams_16 and inst_16", &g_tls_error);
    if (rc == NB_OK) rc = scenes_eye_range_check(fn, scenes, n, first_eye, count, &g_tls_error);
    if (rc != NB_OK) return rc;
    const size_t matrices = (size_t)scenes * n * 16 * sizeof(float);
    const ByteRange in[4] = {{cams_16, matrices},
                             {inst_16, matrices},
                             {weights, (size_t)policies * nbk::policy_recurrent_floats(features, hidden) * sizeof(float)},
                             {mem, (size_t)scenes * n * hidden * sizeof(float)}};
    const ByteRange out[3] = {{feat_out, (size_t)count * features * 4u}, {act_out, (size_t)count * 8u}, {mem_out, (size_t)count * hidden * 4u}};
    rc = outputs_check(fn, out, 0x7u, kNoPolicyMemoryOutputs, true, in, 4, kScenesSeenAlias, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (count == 0) return NB_OK;
    rc = device_for_launch(inst_16, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    ScenesPolicyShape shape{features, hidden, accel_limit, true, memory_limit};
    nbk::ScenesPolicyRecurrentArgs a = scenes_policy_recurrent_args(scenes_eyes(n, first_eye, count, cams_16, inst_16, width), shape, policies, weights);
    a.p.feat_out = (uint32_t *)feat_out, a.p.act_out = (uint32_t *)act_out;
    a.mem_in = (const float *)mem, a.mem_obs = (uint32_t *)mem_out;
    return launch_status(nbk::launch_scenes_policy_recurrent_observe(a, (hipStream_t)stream),
                         "nb: recurrent policy kernel launch failed (scene batch, observe form): ", &g_tls_error);
}

// the context's policies from the host: what nb_scenes_set_policy and nb_scenes_set_policy_recurrent do behind their checks
static int scenes_policies_upload(nb_scenes *ctx, const ScenesPolicyShape &shape, uint32_t policies, const float *weights_host)
{
    const size_t floats = (size_t)policies * shape.floats();
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a step in flight may still read the policies in place
    ctx->policies = 0;
    NB_HIP(ctx, ctx->policy.reserve(floats));
    NB_HIP(ctx, hipMemcpyAsync(ctx->policy.p, weights_host, floats * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the host array is not retained
    ctx->pol = shape, ctx->policies = policies;
    return NB_OK;
}

// The context's memory for a recurrent policy of `hidden` units: there and in use.  A memory of another size (none, or another H) is
// replaced and cleared to +0 on the context's stream; one of this size keeps its words unless `clear`.
static int scenes_memory_ensure(nb_scenes *ctx, uint32_t hidden, bool clear)
{
    const size_t words = (size_t)ctx->scenes * ctx->n * hidden;
    if (!clear && ctx->memory_words == words && ctx->memory.cells >= words) return NB_OK;
    if (ctx->memory.cells < words) {
        NB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a step in flight may still use the memory that is replaced
        NB_HIP(ctx, ctx->memory.reserve(words));
    }
    NB_HIP(ctx, hipMemsetAsync(ctx->memory.p, 0, words * sizeof(float), ctx->stream));
    ctx->memory_words = words;
    return NB_OK;
}

NB_EXPORT int nb_scenes_set_policy(nb_scenes *ctx, uint32_t features, uint32_t hidden, uint32_t policies, const float *weights_host,
                                   float accel_limit)
{
    static const char fn[] = "nb_scenes_set_policy";
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_null_check(fn, {weights_host}, &ctx->err);
    if (rc == NB_OK) rc = policy_check(fn, features, hidden, 0u, policies, ctx->scenes, accel_limit, &ctx->err);
    if (rc != NB_OK) return rc;
    rc = scenes_policies_upload(ctx, {features, hidden, accel_limit}, policies, weights_host);
    // a feedforward policy: the memory's entries are NB_ERR_STATE again, unless a search over a recurrent policy still owns the memory
    if (rc == NB_OK && !(ctx->es_set && ctx->es_pol.recurrent)) ctx->memory_words = 0;
    return rc;
}

NB_EXPORT int nb_scenes_set_policy_recurrent(nb_scenes *ctx, uint32_t features, uint32_t hidden, uint32_t policies, const float *weights_host,
                                             float accel_limit, float memory_limit)
{
    static const char fn[] = "nb_scenes_set_policy_recurrent";
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_null_check(fn, {weights_host}, &ctx->err);
    if (rc == NB_OK) rc = policy_recurrent_check(fn, features, hidden, 0u, policies, ctx->scenes, accel_limit, memory_limit, &ctx->err);
    if (rc != NB_OK) return rc;
    rc = scenes_policies_upload(ctx, {features, hidden, accel_limit, true, memory_limit}, policies, weights_host);
    if (rc != NB_OK) return rc;
    ctx->policies = 0;                               // none is set until the memory is there
    rc = scenes_memory_ensure(ctx, hidden, true);
    if (rc == NB_OK) ctx->policies = policies;
    return rc;
}

// what the context's two policy entries check behind their eye set-up: a policy is there and its features divide the width
static int scenes_policy_set_check(nb_scenes *ctx, const char *fn, uint32_t width)
{
    const int rc = scenes_state_check(ctx, fn, ctx->policies != 0, kCallSetPolicy);
    return rc != NB_OK ? rc : policy_check(fn, ctx->pol.features, ctx->pol.hidden, width, ctx->policies, ctx->scenes, ctx->pol.accel_limit, &ctx->err);
}

// what nb_scenes_step_policy checks behind the context: the eye set-up, a state, a policy
static int scenes_step_policy_check(nb_scenes *ctx, const char *fn, const float *up_xyz, const float *cp16, uint32_t width)
{
    int rc = scenes_eye_setup_check(ctx, fn, up_xyz, cp16, width);
    if (rc == NB_OK) rc = ctx_check(ctx, fn, kCallScenesUpload);
    if (rc == NB_OK) rc = scenes_policy_set_check(ctx, fn, width);
    return rc;
}

// k policy steps as nb_scenes_step_policy issues them, the checks done
static int scenes_policy_steps(nb_scenes *ctx, const char *fn, uint32_t k, const float *up_xyz, const float *cp16, uint32_t width)
{
    return scenes_vision_step(ctx, fn, k, up_xyz, cp16, [=](nb_scenes *ctx) -> int {
        const nbk::ScenesEyes eyes = scenes_eyes(ctx, 0u, ctx->scenes * ctx->n, width);
        nbk::ScenesPolicyRecurrentArgs r{};
        if (ctx->pol.recurrent) r = scenes_policy_recurrent_args(eyes, ctx->pol, ctx->policies, ctx->policy.p);
        nbk::ScenesPolicyArgs &a = r.p;
        if (!ctx->pol.recurrent) a = scenes_policy_args(eyes, ctx->pol, ctx->policies, ctx->policy.p);
        a.pos_in = ctx->pos.p, a.vel_in = ctx->vel.p, a.pos_out = ctx->pos_alt.p, a.vel_out = ctx->vel_alt.p;
        a.ux = up_xyz[0], a.uy = up_xyz[1], a.uz = up_xyz[2], a.dt = ctx->p.dt;
        if (ctx->pol.recurrent) {
            r.mem_in = r.mem_out = ctx->memory.p;    // in place (R7)
            NB_HIP(ctx, nbk::launch_scenes_policy_recurrent(r, ctx->stream));
        } else {
            NB_HIP(ctx, nbk::launch_scenes_policy(a, ctx->stream));
        }
        return NB_OK;
    });
}

NB_EXPORT int nb_scenes_step_policy(nb_scenes *ctx, uint32_t k, const float *up_xyz, const float *cp16, uint32_t width)
{
    static const char fn[] = "nb_scenes_step_policy";
    int rc = ctx_check(ctx, fn);
    if (rc != NB_OK) return rc;
    rc = scenes_step_policy_check(ctx, fn, up_xyz, cp16, width);
    if (rc != NB_OK) return rc;
    return scenes_policy_steps(ctx, fn, k, up_xyz, cp16, width);
}

// P8 or R8 for eyes [first_eye, first_eye + cnt) of the staged state into the context's buffers, whichever kind of policy is set
static int scenes_policy_observe(nb_scenes *ctx, uint32_t first_eye, uint32_t cnt, uint32_t width, bool feat, bool act, bool mem_next)
{
    const nbk::ScenesEyes eyes = scenes_eyes(ctx, first_eye, cnt, width);
    nbk::ScenesPolicyRecurrentArgs r{};
    if (ctx->pol.recurrent) r = scenes_policy_recurrent_args(eyes, ctx->pol, ctx->policies, ctx->policy.p);
    nbk::ScenesPolicyArgs &a = r.p;
    if (!ctx->pol.recurrent) a = scenes_policy_args(eyes, ctx->pol, ctx->policies, ctx->policy.p);
    a.feat_out = feat ? ctx->pol_feat.p : nullptr, a.act_out = act ? ctx->pol_act.p : nullptr;
    if (ctx->pol.recurrent) {
        r.mem_in = ctx->memory.p, r.mem_obs = mem_next ? ctx->pol_mem.p : nullptr;
        NB_HIP(ctx, nbk::launch_scenes_policy_recurrent_observe(r, ctx->stream));
    } else {
        NB_HIP(ctx, nbk::launch_scenes_policy_observe(a, ctx->stream));
    }
    return NB_OK;
}

NB_EXPORT int nb_scenes_eyes_policy(nb_scenes *ctx, uint32_t first_scene, uint32_t scene_count, const float *up_xyz, const float *cp16,
                                    uint32_t width, float *feat, float *act)
{
    static const char fn[] = "nb_scenes_eyes_policy";
    int rc = ctx_check(ctx, fn);
    if (rc != NB_OK) return rc;
    rc = scenes_eye_setup_check(ctx, fn, up_xyz, cp16, width);
    if (rc == NB_OK) rc = scenes_policy_set_check(ctx, fn, width);
    if (rc != NB_OK) return rc;
    const ScenesEyesOutput rows[2] = {{feat, &ctx->pol_feat, ctx->pol.features}, {act, &ctx->pol_act, 2}};
    const auto launch = [=](nb_scenes *ctx, uint32_t first_eye, uint32_t cnt) -> int {
        return scenes_policy_observe(ctx, first_eye, cnt, width, feat != nullptr, act != nullptr, false);
    };
    return scenes_eyes_download(ctx, fn, first_scene, scene_count, up_xyz, cp16, rows, kNoPolicyOutputs, launch);
}

// ---- a recurrent policy with per-body memory (DESIGN.md section 14.8): the context's entries -------------------------------------------
// a memory is in use: a recurrent policy or a search over one is set
static int scenes_memory_set_check(nb_scenes *ctx, const char *fn) { return scenes_state_check(ctx, fn, ctx->memory_words != 0, kCallSetPolicyRecurrent); }

NB_EXPORT int nb_scenes_eyes_policy_memory(nb_scenes *ctx, uint32_t first_scene, uint32_t scene_count, const float *up_xyz, const float *cp16,
                                           uint32_t width, float *feat, float *act, float *mem_next)
{
    static const char fn[] = "nb_scenes_eyes_policy_memory";
    int rc = ctx_check(ctx, fn);
    if (rc != NB_OK) return rc;
    rc = scenes_eye_setup_check(ctx, fn, up_xyz, cp16, width);
    if (rc == NB_OK) rc = scenes_state_check(ctx, fn, ctx->policies != 0 && ctx->pol.recurrent, kCallSetPolicyRecurrent);
    if (rc == NB_OK) rc = scenes_policy_set_check(ctx, fn, width);
    if (rc != NB_OK) return rc;
    const ScenesEyesOutput rows[3] = {{feat, &ctx->pol_feat, ctx->pol.features}, {act, &ctx->pol_act, 2}, {mem_next, &ctx->pol_mem, ctx->pol.hidden}};
    const auto launch = [=](nb_scenes *ctx, uint32_t first_eye, uint32_t cnt) -> int {
        return scenes_policy_observe(ctx, first_eye, cnt, width, feat != nullptr, act != nullptr, mem_next != nullptr);
    };
    return scenes_eyes_download(ctx, fn, first_scene, scene_count, up_xyz, cp16, rows, kNoPolicyMemoryOutputs, launch);
}

NB_EXPORT int nb_scenes_memory_reset(nb_scenes *ctx)
{
    static const char fn[] = "nb_scenes_memory_reset";
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_memory_set_check(ctx, fn);
    if (rc != NB_OK) return rc;
    NB_HIP(ctx, hipMemsetAsync(ctx->memory.p, 0, ctx->memory_words * sizeof(float), ctx->stream));
    return NB_OK;
}

NB_EXPORT int nb_scenes_memory(nb_scenes *ctx, uint32_t first_scene, uint32_t scene_count, float *out_host)
{
    static const char fn[] = "nb_scenes_memory";
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_null_check(fn, {out_host}, &ctx->err);
    if (rc == NB_OK) rc = scenes_range_check(ctx, fn, first_scene, scene_count);
    if (rc == NB_OK) rc = scenes_memory_set_check(ctx, fn);
    if (rc != NB_OK) return rc;
    const size_t per_scene = ctx->memory_words / ctx->scenes;   // n * hidden
    if (scene_count)
        NB_HIP(ctx, hipMemcpyAsync(out_host, ctx->memory.p + first_scene * per_scene, scene_count * per_scene * sizeof(float), hipMemcpyDeviceToHost,
                                   ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NB_OK;
}

NB_EXPORT int nb_scenes_set_memory(nb_scenes *ctx, const float *mem_host)
{
    static const char fn[] = "nb_scenes_set_memory";
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_null_check(fn, {mem_host}, &ctx->err);
    if (rc == NB_OK) rc = scenes_memory_set_check(ctx, fn);
    if (rc != NB_OK) return rc;
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a step in flight may still use the memory
    NB_HIP(ctx, hipMemcpyAsync(ctx->memory.p, mem_host, ctx->memory_words * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the host array is not retained
    return NB_OK;
}

// ---- the score of every scene, accumulated on the device (DESIGN.md section 14.5) -----------------------------------------------------------
static_assert(sizeof(nb_scene_score) == 32 && sizeof(nbk::SceneScore) == 32 && alignof(nbk::SceneScore) == 8, "Q7's record");
static_assert(offsetof(nb_scene_score, spread) == offsetof(nbk::SceneScore, spread) && offsetof(nb_scene_score, steps) == offsetof(nbk::SceneScore, steps) &&
                  offsetof(nb_scene_score, nonfinite) == offsetof(nbk::SceneScore, nonfinite),
              "the header's record is the kernel's");
static const char kCallSetScore[] = ": no score set (call nb_scenes_set_score first)";

// Q2's radius and Q5's goal
static int score_params_check(const char *fn, const nb_score_params &sp, std::string *err)
{
    if (!(sp.radius_sq >= 0.0f)) {
        *err = std::string(fn) + ": radius_sq must be at least 0 (+inf: every pair)";
        return NB_ERR_INVALID;
    }
    if (!(std::isfinite(sp.goal[0]) && std::isfinite(sp.goal[1]) && std::isfinite(sp.goal[2]))) {
        *err = std::string(fn) + ": goal must be finite";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

static nbk::ScenesScoreArgs scenes_score_args(const nb_score_params &sp, uint32_t scenes, uint32_t n, const void *pos, const void *vel, void *score)
{
    nbk::ScenesScoreArgs a{};
    a.pos = (const float4 *)pos, a.vel = (const float4 *)vel, a.score = (nbk::SceneScore *)score;
    a.scenes = scenes, a.n = n;
    a.radius_sq = sp.radius_sq, a.gx = sp.goal[0], a.gy = sp.goal[1], a.gz = sp.goal[2];
    return a;
}

NB_EXPORT int nb_scenes_score_launch(const nb_score_params *sp, uint32_t scenes, uint32_t n, const void *pos, const void *vel, void *score,
                                     void *stream)
{
    static const char fn[] = "nb_scenes_score_launch";
    int rc = scenes_null_check(fn, {sp, pos, vel, score}, &g_tls_error);
    if (rc == NB_OK) rc = scenes_shape_check(fn, scenes, n, &g_tls_error);
    if (rc == NB_OK) rc = score_params_check(fn, *sp, &g_tls_error);
    if (rc == NB_OK) rc = scenes_records_check(fn, scenes, n, pos, vel, &g_tls_error);
    if (rc == NB_OK) rc = scenes_aligned_check(fn, 8, {score}, "score", &g_tls_error);
    if (rc != NB_OK) return rc;
    const size_t bytes = (size_t)scenes * n * sizeof(float4), sbytes = (size_t)scenes * sizeof(nb_scene_score);
    if (ranges_overlap(score, sbytes, pos, bytes) || ranges_overlap(score, sbytes, vel, bytes)) {
        g_tls_error = std::string(fn) + ": score must not overlap pos or vel";
        return NB_ERR_INVALID;
    }
    rc = device_for_launch(pos, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    return launch_status(nbk::launch_scenes_score(scenes_score_args(*sp, scenes, n, pos, vel, score), (hipStream_t)stream),
                         "nb: score kernel launch failed (scene batch): ", &g_tls_error);
}

NB_EXPORT int nb_scenes_set_score(nb_scenes *ctx, const nb_score_params *sp)
{
    static const char fn[] = "nb_scenes_set_score";
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_null_check(fn, {sp}, &ctx->err);
    if (rc == NB_OK) rc = score_params_check(fn, *sp, &ctx->err);
    if (rc != NB_OK) return rc;
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a score in flight runs under the parameters it was issued with
    ctx->score_set = false;
    NB_HIP(ctx, ctx->score.reserve(ctx->scenes));
    NB_HIP(ctx, hipMemsetAsync(ctx->score.p, 0, (size_t)ctx->scenes * sizeof(nb_scene_score), ctx->stream));
    ctx->sp = *sp;
    ctx->score_set = true;
    return NB_OK;
}

// the context holds a score
static int scenes_score_set_check(nb_scenes *ctx, const char *fn) { return scenes_state_check(ctx, fn, ctx->score_set, kCallSetScore); }

// the current snapshot into the context's records, the checks done
static int scenes_score_now(nb_scenes *ctx)
{
    NB_HIP(ctx, nbk::launch_scenes_score(scenes_score_args(ctx->sp, ctx->scenes, ctx->n, ctx->pos.p, ctx->vel.p, ctx->score.p), ctx->stream));
    return NB_OK;
}

NB_EXPORT int nb_scenes_score(nb_scenes *ctx)
{
    static const char fn[] = "nb_scenes_score";
    int rc = ctx_check(ctx, fn, kCallScenesUpload);
    if (rc == NB_OK) rc = scenes_score_set_check(ctx, fn);
    if (rc != NB_OK) return rc;
    RoctxRange range(fn);
    return scenes_score_now(ctx);
}

NB_EXPORT int nb_scenes_score_reset(nb_scenes *ctx)
{
    static const char fn[] = "nb_scenes_score_reset";
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_score_set_check(ctx, fn);
    if (rc != NB_OK) return rc;
    NB_HIP(ctx, hipMemsetAsync(ctx->score.p, 0, (size_t)ctx->scenes * sizeof(nb_scene_score), ctx->stream));
    return NB_OK;
}

NB_EXPORT int nb_scenes_scores(nb_scenes *ctx, uint32_t first_scene, uint32_t scene_count, nb_scene_score *out_host)
{
    static const char fn[] = "nb_scenes_scores";
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_null_check(fn, {out_host}, &ctx->err);
    if (rc == NB_OK) rc = scenes_range_check(ctx, fn, first_scene, scene_count);
    if (rc == NB_OK) rc = scenes_score_set_check(ctx, fn);
    if (rc != NB_OK) return rc;
    if (scene_count == 0) return NB_OK;
    NB_HIP(ctx, hipMemcpyAsync(out_host, ctx->score.p + first_scene, (size_t)scene_count * sizeof(nb_scene_score), hipMemcpyDeviceToHost, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NB_OK;
}

NB_EXPORT int nb_scenes_step_policy_scored(nb_scenes *ctx, uint32_t k, const float *up_xyz, const float *cp16, uint32_t width)
{
    static const char fn[] = "nb_scenes_step_policy_scored";
    int rc = ctx_check(ctx, fn);
    if (rc != NB_OK) return rc;
    rc = scenes_step_policy_check(ctx, fn, up_xyz, cp16, width);
    if (rc == NB_OK) rc = scenes_score_set_check(ctx, fn);
    if (rc != NB_OK) return rc;
    for (uint32_t s = 0; s < k; ++s) {
        rc = scenes_policy_steps(ctx, fn, 1u, up_xyz, cp16, width);
        if (rc == NB_OK) rc = scenes_score_now(ctx);
        if (rc != NB_OK) return rc;
    }
    return NB_OK;
}

// ---- an evolution-strategies generation on the device (DESIGN.md section 14.6) --------------------------------------------------------------
static_assert(NB_ES_MAX_POPULATION == nbk::kEsMaxPopulation, "the header's limit is the kernels'");
static_assert(sizeof(nb_es_params) == 40 && offsetof(nb_es_params, seed) == 32 && sizeof(nb_es_report) == 16, "E1-E7's parameters and the report");
static const char kCallEsSet[] = ": no search set (call nb_scenes_es_set first)";
static const char kCallEsUpdate[] = ": no generation updated (call nb_scenes_es_update first)";
static const char kCallKeep[] = ": no state kept (call nb_scenes_keep first)";

// E3's sigma, E7's step and E4's coefficients
static int es_params_check(const char *fn, const nb_es_params &ep, std::string *err)
{
    if (!(ep.sigma >= 0.0f) || std::isinf(ep.sigma)) {
        *err = std::string(fn) + ": sigma must be at least 0 and finite";
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(ep.step)) {
        *err = std::string(fn) + ": step must be finite";
        return NB_ERR_INVALID;
    }
    for (const float c : ep.coef)
        if (!std::isfinite(c)) {
            *err = std::string(fn) + ": coef must be finite";
            return NB_ERR_INVALID;
        }
    return NB_OK;
}

// the policy shape of a search: policy_check's two bounds, with nothing else of it in play
static int es_shape_check(const char *fn, uint32_t features, uint32_t hidden, std::string *err)
{
    return policy_check(fn, features, hidden, 0u, 1u, 1u, 0.0f, err);
}

// the length of a stateless launch's mean: by_shape, nb_policy_floats of a policy shape within the limits; otherwise `floats` itself
static int es_floats_check(const char *fn, bool by_shape, uint32_t features, uint32_t hidden, uint32_t floats, size_t *m, std::string *err)
{
    if (by_shape) {
        *m = nbk::policy_floats(features, hidden);
        return es_shape_check(fn, features, hidden, err);
    }
    *m = floats;
    if (floats == 0 || floats > NB_ES_MAX_FLOATS) {
        *err = std::string(fn) + ": floats must be 1 .. NB_ES_MAX_FLOATS (20674)";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

static nbk::EsArgs es_args(const nb_es_params &ep, size_t m, uint32_t generation, uint32_t scenes)
{
    nbk::EsArgs a{};
    a.seed = ep.seed, a.g = generation, a.scenes = scenes, a.m = (uint32_t)m;
    a.sigma = ep.sigma, a.step = ep.step;
    a.c0 = ep.coef[0], a.c1 = ep.coef[1], a.c2 = ep.coef[2], a.c3 = ep.coef[3], a.c4 = ep.coef[4], a.c5 = ep.coef[5];
    return a;
}

// nb_scenes_es_perturb_launch and nb_scenes_es_perturb_floats_launch: E1-E3 depend on the weight index alone, so the mean's length is
// all the kernel takes of the shape
static int es_perturb_launch(const char *fn, const nb_es_params *ep, bool by_shape, uint32_t features, uint32_t hidden, uint32_t floats,
                             uint32_t generation, uint32_t first_scene, uint32_t count, const void *mean, void *theta_out, void *stream)
{
    size_t m = 0;
    int rc = scenes_null_check(fn, {ep, mean, theta_out}, &g_tls_error);
    if (rc == NB_OK) rc = es_floats_check(fn, by_shape, features, hidden, floats, &m, &g_tls_error);
    if (rc == NB_OK) rc = es_params_check(fn, *ep, &g_tls_error);
    if (rc != NB_OK) return rc;
    if ((uint64_t)first_scene + count > NB_ES_MAX_POPULATION) {
        g_tls_error = std::string(fn) + ": scenes [first_scene, first_scene + count) must lie in 0 .. NB_ES_MAX_POPULATION (4096)";
        return NB_ERR_INVALID;
    }
    rc = scenes_aligned_check(fn, 4, {mean, theta_out}, "mean and theta_out", &g_tls_error);
    if (rc != NB_OK) return rc;
    if (ranges_overlap(theta_out, (size_t)count * m * sizeof(float), mean, m * sizeof(float))) {
        g_tls_error = std::string(fn) + ": theta_out must not overlap mean";
        return NB_ERR_INVALID;
    }
    if (count == 0) return NB_OK;
    rc = device_for_launch(mean, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    static_assert((uint64_t)(NB_ES_MAX_POPULATION / 2u) * ((NB_ES_MAX_FLOATS + 1u) / 2u) < (1ull << 25), "the flat perturb grid: 2 048 x 10 337 lanes");
    return launch_status(nbk::launch_es_perturb(es_args(*ep, m, generation, 0u), first_scene, count, (const float *)mean, (float *)theta_out,
                                                (hipStream_t)stream),
                         "nb: perturb kernel launch failed (scene batch, search): ", &g_tls_error);
}

NB_EXPORT int nb_scenes_es_perturb_launch(const nb_es_params *ep, uint32_t features, uint32_t hidden, uint32_t generation, uint32_t first_scene,
                                          uint32_t count, const void *mean, void *theta_out, void *stream)
{
    return es_perturb_launch("nb_scenes_es_perturb_launch", ep, true, features, hidden, 0u, generation, first_scene, count, mean, theta_out, stream);
}

NB_EXPORT int nb_scenes_es_perturb_floats_launch(const nb_es_params *ep, uint32_t floats, uint32_t generation, uint32_t first_scene, uint32_t count,
                                                 const void *mean, void *theta_out, void *stream)
{
    return es_perturb_launch("nb_scenes_es_perturb_floats_launch", ep, false, 0u, 0u, floats, generation, first_scene, count, mean, theta_out, stream);
}

// nb_scenes_es_update_launch and nb_scenes_es_update_floats_launch, likewise
static int es_update_launch(const char *fn, const nb_es_params *ep, bool by_shape, uint32_t features, uint32_t hidden, uint32_t floats,
                            uint32_t generation, uint32_t scenes, const void *score, const void *mean, void *mean_out, void *rank_out,
                            void *fitness_out, void *report_out, void *stream)
{
    size_t m = 0;
    int rc = scenes_null_check(fn, {ep, score, mean, mean_out, rank_out}, &g_tls_error);
    if (rc == NB_OK) rc = es_floats_check(fn, by_shape, features, hidden, floats, &m, &g_tls_error);
    if (rc == NB_OK) rc = es_params_check(fn, *ep, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (scenes == 0 || scenes > NB_ES_MAX_POPULATION) {
        g_tls_error = std::string(fn) + ": scenes must be 1 .. NB_ES_MAX_POPULATION (4096)";
        return NB_ERR_INVALID;
    }
    rc = scenes_aligned_check(fn, 8, {score}, "score", &g_tls_error);
    if (rc == NB_OK) rc = scenes_aligned_check(fn, 4, {mean}, "mean", &g_tls_error);
    if (rc != NB_OK) return rc;
    const size_t mbytes = m * sizeof(float);
    const bool in_place = mean_out == mean;   // the update may be in place: a weight's word is read and written by one lane
    const ByteRange in[2] = {{score, (size_t)scenes * sizeof(nb_scene_score)}, {in_place ? nullptr : mean, mbytes}};
    const ByteRange out[4] = {{mean_out, mbytes}, {rank_out, (size_t)scenes * 4u}, {fitness_out, (size_t)scenes * 4u}, {report_out, sizeof(nb_es_report)}};
    rc = outputs_check(fn, out, 0xFu, "", true, in, 2, kScenesSeenAlias, &g_tls_error);
    if (rc != NB_OK) return rc;
    rc = device_for_launch(score, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    const nbk::EsArgs a = es_args(*ep, m, generation, scenes);
    rc = launch_status(nbk::launch_es_rank(a, (const nbk::SceneScore *)score, (uint32_t *)rank_out, (float *)fitness_out, (uint32_t *)report_out,
                                           (hipStream_t)stream),
                       "nb: rank kernel launch failed (scene batch, search): ", &g_tls_error);
    if (rc != NB_OK) return rc;
    return launch_status(nbk::launch_es_update(a, (const uint32_t *)rank_out, (const float *)mean, (float *)mean_out, (hipStream_t)stream),
                         "nb: update kernel launch failed (scene batch, search): ", &g_tls_error);
}

NB_EXPORT int nb_scenes_es_update_launch(const nb_es_params *ep, uint32_t features, uint32_t hidden, uint32_t generation, uint32_t scenes,
                                         const void *score, const void *mean, void *mean_out, void *rank_out, void *fitness_out,
                                         void *report_out, void *stream)
{
    return es_update_launch("nb_scenes_es_update_launch", ep, true, features, hidden, 0u, generation, scenes, score, mean, mean_out, rank_out,
                            fitness_out, report_out, stream);
}

NB_EXPORT int nb_scenes_es_update_floats_launch(const nb_es_params *ep, uint32_t floats, uint32_t generation, uint32_t scenes, const void *score,
                                                const void *mean, void *mean_out, void *rank_out, void *fitness_out, void *report_out,
                                                void *stream)
{
    return es_update_launch("nb_scenes_es_update_floats_launch", ep, false, 0u, 0u, floats, generation, scenes, score, mean, mean_out, rank_out,
                            fitness_out, report_out, stream);
}

// the context holds a search
static int scenes_es_set_check(nb_scenes *ctx, const char *fn) { return scenes_state_check(ctx, fn, ctx->es_set, kCallEsSet); }

// nb_scenes_es_set and nb_scenes_es_set_recurrent: the search over policies of `shape`, whose mean has shape.floats() floats
static int scenes_es_set(nb_scenes *ctx, const char *fn, const ScenesPolicyShape &shape, const float *mean_host, const nb_es_params *ep)
{
    const uint32_t features = shape.features, hidden = shape.hidden;
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_null_check(fn, {mean_host, ep}, &ctx->err);
    if (rc == NB_OK && !shape.recurrent) rc = policy_check(fn, features, hidden, 0u, ctx->scenes, ctx->scenes, shape.accel_limit, &ctx->err);
    if (rc == NB_OK && shape.recurrent)
        rc = policy_recurrent_check(fn, features, hidden, 0u, ctx->scenes, ctx->scenes, shape.accel_limit, shape.memory_limit, &ctx->err);
    if (rc == NB_OK) rc = es_params_check(fn, *ep, &ctx->err);
    if (rc != NB_OK) return rc;
    if (ctx->scenes > NB_ES_MAX_POPULATION) {
        ctx->err = std::string(fn) + ": a search takes a batch of at most NB_ES_MAX_POPULATION (4096) scenes";
        return NB_ERR_INVALID;
    }
    const size_t m = shape.floats();
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a step or an update in flight may still read the policies and the mean
    ctx->es_set = ctx->es_updated = false;
    ctx->policies = 0;                               // the policies' buffer may be replaced: none is set until nb_scenes_es_perturb
    NB_HIP(ctx, ctx->policy.reserve((size_t)ctx->scenes * m));
    NB_HIP(ctx, ctx->es_mean.reserve(m));
    NB_HIP(ctx, ctx->es_rank.reserve(ctx->scenes));
    NB_HIP(ctx, ctx->es_fitness.reserve(ctx->scenes));
    NB_HIP(ctx, ctx->es_report.reserve(4));
    NB_HIP(ctx, hipMemcpyAsync(ctx->es_mean.p, mean_host, m * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the host array is not retained
    ctx->es_pol = shape, ctx->ep = *ep;
    ctx->es_generation = 0;
    if (shape.recurrent) {                           // the memory the population will step: there from here on, so that a reset may precede the first perturb
        rc = scenes_memory_ensure(ctx, hidden, false);
        if (rc != NB_OK) return rc;
    } else {
        ctx->memory_words = 0;                       // no policy is set and the search needs none
    }
    ctx->es_set = true;
    return NB_OK;
}

NB_EXPORT int nb_scenes_es_set(nb_scenes *ctx, uint32_t features, uint32_t hidden, const float *mean_host, float accel_limit, const nb_es_params *ep)
{
    return scenes_es_set(ctx, "nb_scenes_es_set", {features, hidden, accel_limit}, mean_host, ep);
}

NB_EXPORT int nb_scenes_es_set_recurrent(nb_scenes *ctx, uint32_t features, uint32_t hidden, const float *mean_host, float accel_limit,
                                         float memory_limit, const nb_es_params *ep)
{
    return scenes_es_set(ctx, "nb_scenes_es_set_recurrent", {features, hidden, accel_limit, true, memory_limit}, mean_host, ep);
}

NB_EXPORT int nb_scenes_es_perturb(nb_scenes *ctx)
{
    static const char fn[] = "nb_scenes_es_perturb";
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_es_set_check(ctx, fn);
    if (rc != NB_OK) return rc;
    RoctxRange range(fn);
    if (ctx->es_pol.recurrent) {                     // the policies become recurrent: their memory, if the context has none of that size
        rc = scenes_memory_ensure(ctx, ctx->es_pol.hidden, false);
        if (rc != NB_OK) return rc;
    } else {
        ctx->memory_words = 0;
    }
    NB_HIP(ctx, nbk::launch_es_perturb(es_args(ctx->ep, ctx->es_pol.floats(), ctx->es_generation, ctx->scenes), 0u, ctx->scenes, ctx->es_mean.p,
                                       ctx->policy.p, ctx->stream));
    ctx->pol = ctx->es_pol, ctx->policies = ctx->scenes;
    return NB_OK;
}

NB_EXPORT int nb_scenes_es_update(nb_scenes *ctx)
{
    static const char fn[] = "nb_scenes_es_update";
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_es_set_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_score_set_check(ctx, fn);
    if (rc != NB_OK) return rc;
    RoctxRange range(fn);
    const nbk::EsArgs a = es_args(ctx->ep, ctx->es_pol.floats(), ctx->es_generation, ctx->scenes);
    NB_HIP(ctx, nbk::launch_es_rank(a, ctx->score.p, ctx->es_rank.p, ctx->es_fitness.p, ctx->es_report.p, ctx->stream));
    NB_HIP(ctx, nbk::launch_es_update(a, ctx->es_rank.p, ctx->es_mean.p, ctx->es_mean.p, ctx->stream));
    ctx->es_generation += 1u;
    ctx->es_updated = true;
    return NB_OK;
}

NB_EXPORT int nb_scenes_es_mean(nb_scenes *ctx, float *out_host)
{
    static const char fn[] = "nb_scenes_es_mean";
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_null_check(fn, {out_host}, &ctx->err);
    if (rc == NB_OK) rc = scenes_es_set_check(ctx, fn);
    if (rc != NB_OK) return rc;
    const size_t m = ctx->es_pol.floats();
    NB_HIP(ctx, hipMemcpyAsync(out_host, ctx->es_mean.p, m * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NB_OK;
}

NB_EXPORT int nb_scenes_es_result(nb_scenes *ctx, nb_es_report *report, float *fitness, uint32_t *rank)
{
    static const char fn[] = "nb_scenes_es_result";
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_es_set_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_state_check(ctx, fn, ctx->es_updated, kCallEsUpdate);
    if (rc != NB_OK) return rc;
    if (report) NB_HIP(ctx, hipMemcpyAsync(report, ctx->es_report.p, sizeof(nb_es_report), hipMemcpyDeviceToHost, ctx->stream));
    if (fitness) NB_HIP(ctx, hipMemcpyAsync(fitness, ctx->es_fitness.p, (size_t)ctx->scenes * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (rank) NB_HIP(ctx, hipMemcpyAsync(rank, ctx->es_rank.p, (size_t)ctx->scenes * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NB_OK;
}

NB_EXPORT uint32_t nb_scenes_es_generation(const nb_scenes *ctx) { return ctx ? ctx->es_generation : 0u; }

NB_EXPORT int nb_scenes_keep(nb_scenes *ctx)
{
    static const char fn[] = "nb_scenes_keep";
    int rc = ctx_check(ctx, fn, kCallScenesUpload);
    if (rc != NB_OK) return rc;
    const size_t records = (size_t)ctx->scenes * ctx->n;
    NB_HIP(ctx, ctx->pos_kept.reserve(records));   // allocated by the first keep
    NB_HIP(ctx, ctx->vel_kept.reserve(records));
    NB_HIP(ctx, hipMemcpyAsync(ctx->pos_kept.p, ctx->pos.p, records * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
    NB_HIP(ctx, hipMemcpyAsync(ctx->vel_kept.p, ctx->vel.p, records * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
    ctx->steps_kept = ctx->steps;
    ctx->kept = true;
    return NB_OK;
}

NB_EXPORT int nb_scenes_rewind(nb_scenes *ctx)
{
    static const char fn[] = "nb_scenes_rewind";
    int rc = ctx_check(ctx, fn);
    if (rc == NB_OK) rc = scenes_state_check(ctx, fn, ctx->kept, kCallKeep);
    if (rc != NB_OK) return rc;
    const size_t records = (size_t)ctx->scenes * ctx->n;
    NB_HIP(ctx, hipMemcpyAsync(ctx->pos.p, ctx->pos_kept.p, records * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
    NB_HIP(ctx, hipMemcpyAsync(ctx->vel.p, ctx->vel_kept.p, records * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
    ctx->steps = ctx->steps_kept;
    return NB_OK;
}

NB_EXPORT int nb_scenes_device_state(nb_scenes *ctx, const void **pos_rec, const void **vel_rec, const void **inst_16n)
{
    int rc = ctx_check(ctx, "nb_scenes_device_state", kCallScenesUpload);
    if (rc != NB_OK) return rc;
    const size_t records = (size_t)ctx->scenes * ctx->n;
    if (inst_16n) {
        NB_HIP(ctx, launch_matrices((uint32_t)records, ctx->pos.p, ctx->vel.p, &ctx->inst, ctx->stream));
        *inst_16n = ctx->inst.p;
    }
    if (pos_rec) *pos_rec = ctx->pos.p;
    if (vel_rec) *vel_rec = ctx->vel.p;
    return NB_OK;
}

NB_EXPORT int nb_scenes_sync(nb_scenes *ctx)
{
    int rc = ctx_check(ctx, "nb_scenes_sync");
    if (rc != NB_OK) return rc;
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NB_OK;
}

NB_EXPORT uint64_t nb_scenes_steps(const nb_scenes *ctx) { return ctx ? ctx->steps : 0; }

NB_EXPORT int nb_scenes_download(nb_scenes *ctx, float *pos_xyz, float *vel_xyz, float *inst_16)
{
    static const char fn[] = "nb_scenes_download";
    int rc = ctx_check(ctx, fn);
    if (rc != NB_OK) return rc;
    if (!pos_xyz && !vel_xyz && !inst_16) {
        ctx->err = std::string(fn) + ": pos_xyz, vel_xyz and inst_16 are all NULL";
        return NB_ERR_INVALID;
    }
    rc = ctx_check(ctx, fn, kCallScenesUpload);
    if (rc != NB_OK) return rc;
    const size_t records = (size_t)ctx->scenes * ctx->n, bytes = records * 3 * sizeof(float);
    if (pos_xyz) {
        NB_HIP(ctx, nbk::launch_unpack((uint32_t)records, ctx->pos.p, ctx->stage.p, ctx->stream));
        NB_HIP(ctx, hipMemcpyAsync(pos_xyz, ctx->stage.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (vel_xyz) {
        NB_HIP(ctx, nbk::launch_unpack((uint32_t)records, ctx->vel.p, ctx->stage.p + 3 * records, ctx->stream));
        NB_HIP(ctx, hipMemcpyAsync(vel_xyz, ctx->stage.p + 3 * records, bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (inst_16) {
        NB_HIP(ctx, launch_matrices((uint32_t)records, ctx->pos.p, ctx->vel.p, &ctx->inst, ctx->stream));
        NB_HIP(ctx, hipMemcpyAsync(inst_16, ctx->inst.p, records * 16 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NB_OK;
}
