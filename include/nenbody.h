/*
 * nenbody.h -- C ABI of libnenbody_hip.so: nenbody's all-pairs gravity + Euler step on MI355X (gfx950).
 *
 * This is the drop-in boundary for the per-frame simulation update of Dasch0/nenbody: `update_instance_nbody`
 * (reference src/main.rs:404-441) -- the path this library exists for -- and, as the first row beyond it, the
 * controller the binary actually runs, `update_instance_boids` (src/main.rs:443-526).  Both are bodies of the
 * `Scene::step()` the reference's empty `src/scene.rs` (src/scene.rs:1, declared at src/main.rs:2) was evidently
 * meant to hold.
 * The reference has no FFI of its own; each entry point below cites the reference
 * interface it stands in for.  INTEGRATION.md shows the Rust `extern "C"` block and the
 * `Scene` shim a maintainer would add.  Only what a host binds is declared here; the library's self-tests and the test
 * suite's switches are in nenbody_diag.h.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch types.
 *  - every function returns NB_OK (0) or a negative nb_status; nothing unwinds across the boundary.
 *  - host arrays are caller-allocated, caller-freed, and never retained past the call.
 *  - positions / velocities cross as AoS stride-3 float arrays (x,y,z): the in-memory form of
 *    Vec<cgmath::Point3<f32>> / Vec<cgmath::Vector3<f32>>, so `positions.as_ptr() as *const f32` needs no repack.
 *  - instance matrices cross as 16 floats per body, column-major: the in-memory form of
 *    Vec<[[f32; 4]; 4]> consumed as `mat4 model[]` by shaders/scene.vert:12-14,18.
 *  - a context is single-owner and not re-entrant (the reference calls the update on the winit main
 *    thread, src/main.rs:925); work is queued on a HIP stream and nb_step may return before it finishes.
 *  - there is NO CPU fallback: without a HIP device every compute entry point fails with NB_ERR_NO_DEVICE.
 */
#ifndef NENBODY_H
#define NENBODY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NB_ABI_VERSION 2

typedef enum nb_status {
    NB_OK = 0,
    NB_ERR_INVALID = -1,     /* bad argument (null pointer, zero bodies, range outside the set, bad mode/tile) */
    NB_ERR_NO_DEVICE = -2,   /* no HIP device visible / HIP runtime failed to initialise */
    NB_ERR_HIP = -3,         /* a HIP call failed; nb_last_error() has the HIP error string */
    NB_ERR_ALLOC = -4,       /* device or host allocation failed */
    NB_ERR_STATE = -5,       /* call sequence error (e.g. nb_step before nb_upload) */
    NB_ERR_UNSUPPORTED = -6  /* e.g. n_devices != 1: one process drives one GPU; see nb_launch_step for sharding */
} nb_status;

/* Arithmetic variants of the pair fold (src/main.rs:425-432). */
typedef enum nb_mode {
    /* Bit-identical to the reference's binary32 arithmetic: sequential j = 0..N-1 per body, no FMA
     * contraction, correctly rounded (vec*G)/dist per component.  The parity path. */
    NB_MODE_STRICT = 0,
    /* Same law, reassociated for speed: r2 by FMA chain, v_rcp_f32 instead of the divide (one reciprocal shared by two
     * pairs where their product cannot leave the normal range), G hoisted out of the sum, j range may be split and
     * partial sums combined in a fixed (deterministic) order.
     * Per-step relative force error ~1e-6; NOT bit-identical to the reference. */
    NB_MODE_FAST = 1
} nb_mode;

/* Constants of the step.  Defaults are the reference's: src/main.rs:411-413. */
typedef struct nb_params {
    float dt;       /* 0.1       main.rs:411 (velocity update only; position advances by v with no dt, main.rs:436) */
    float G;        /* 0.001     main.rs:412 */
    float bias;     /* 0.0000001 main.rs:413, added to the squared distance */
    uint32_t tile;  /* bodies staged through LDS per tile; 0 = library default; else 256, 512 or 1024 */
    uint32_t mode;  /* nb_mode */
} nb_params;

/* Constants of the boids controller, update_instance_boids (src/main.rs:443-526) -- the controller the reference's
 * event loop calls (src/main.rs:925).  Defaults are the reference's: src/main.rs:450-456. */
typedef struct nb_boids_params {
    float dt;               /* 0.04   main.rs:450 */
    float rule_1_distance;  /* 1000.0 main.rs:451; compared with the SQUARED distance (main.rs:474-475) */
    float rule_2_distance;  /* 5.0    main.rs:452 */
    float rule_3_distance;  /* 500.0  main.rs:453; a distance between VELOCITIES (main.rs:497) */
    float rule_1_scale;     /* 0.02   main.rs:454 */
    float rule_2_scale;     /* 0.05   main.rs:455 */
    float rule_3_scale;     /* 0.5    main.rs:456 */
    uint32_t tile;          /* bodies staged through LDS per tile; 0 = library default; else 256, 512 or 1024 */
} nb_boids_params;

typedef struct nb_ctx nb_ctx; /* opaque; owns the device buffers and the stream */

/* -- library ------------------------------------------------------------------------------------------- */
int nb_abi_version(void);
/* Fills *p with the reference constants (main.rs:411-413), tile 0, NB_MODE_STRICT. */
void nb_default_params(nb_params *p);
/* Number of HIP devices this process can see, or a negative nb_status. */
int nb_device_count(void);
/* Message of the last failure on `ctx`, or (ctx == NULL) of the calling thread's last failed
 * context-free call.  Never NULL; valid until the next call on the same ctx / thread. */
const char *nb_last_error(const nb_ctx *ctx);

/* Seeded stand-in for the reference's unseeded rand::thread_rng() initial state (src/main.rs:736-747):
 * same distributions and draw order (all velocities (U[0,0.1),U[0,0.1),0) first, then all positions
 * (U[-100,100),U[-100,100),0)).  Host-side; pos_xyz / vel_xyz hold 3*n floats. */
int nb_init_state(uint64_t seed, uint32_t n, float *pos_xyz, float *vel_xyz);

/* -- context API: what a Scene owns -------------------------------------------------------------------- *
 * Stands in for the state the reference keeps in main(): positions, velocities, old_positions,
 * old_velocities, instance_data (src/main.rs:738-750) -- here device-resident.                            */

/* Create a context for n bodies on the current HIP device.  n_devices must be 1 (one process per GPU;
 * multi-GPU hosts shard with nb_launch_step + an all-gather, see below).  params == NULL -> defaults. */
int nb_create(uint32_t n, uint32_t n_devices, const nb_params *params, nb_ctx **out);
void nb_destroy(nb_ctx *ctx);

/* Host -> device.  pos_xyz, vel_xyz: 3*n floats each (the Vec<Point3>/Vec<Vector3> the reference's
 * update function receives, src/main.rs:406-408). */
int nb_upload(nb_ctx *ctx, const float *pos_xyz, const float *vel_xyz);

/* k applications of update_instance_nbody (src/main.rs:404-441), device-resident, asynchronous.
 * old_positions (main.rs:415) is the ping-pong buffer; old_velocities (main.rs:416) is never read by
 * the reference's function and has no counterpart. */
int nb_step(nb_ctx *ctx, uint32_t k);

/* Fills *p with the reference constants (main.rs:450-456), tile 0. */
void nb_boids_default_params(nb_boids_params *p);

/* k applications of update_instance_boids (src/main.rs:443-526) to the context's state, device-resident,
 * asynchronous; bit-identical to the reference's binary32 arithmetic (the three folds run in index order, the
 * sqrt-based radius tests are evaluated exactly).  params == NULL -> defaults.  May be mixed freely with nb_step. */
int nb_step_boids(nb_ctx *ctx, uint32_t k, const nb_boids_params *params);

/* k applications of the random-walk controller update_instance_random (src/main.rs:381-402): vel += (U[-1e-4,1e-4),
 * U[-1e-4,1e-4), 0); pos += vel.  The reference draws from an unseeded thread_rng, so only the distribution is kept:
 * the stream here is counter based on (seed, step index since nb_upload, body index). */
int nb_step_random(nb_ctx *ctx, uint32_t k, uint64_t seed);

/* Device-resident hand-off: pointers to the context's CURRENT device buffers -- 16-byte position
 * and velocity records and, when inst is non-NULL, the model matrices of the current state (16 floats per body,
 * produced now on the context's stream) -- for a consumer that reads them on the GPU instead of through nb_download
 * (the reference re-uploads instance_data every frame, src/main.rs:932-936).  Valid until the next nb_step*, nb_upload
 * or nb_destroy on ctx; call nb_sync first if the consumer does not run on a stream ordered after ctx's. */
int nb_device_state(nb_ctx *ctx, const void **pos_rec, const void **vel_rec, const void **inst_16n);

/* CameraArray::update (src/gfx.rs:397-408, build_camera :358-369) for the context's current state: per body
 * out = cp * look_at_dir(eye = position, dir = velocity, up), where cp16 = OPENGL_TO_WGPU_MATRIX * perspective(...) is the
 * array's constant (16 floats, column-major; nb_camera_constant below, or the caller's own cgmath::perspective).  out_16n: host, 16n floats. */
int nb_cameras(nb_ctx *ctx, const float *up_xyz, const float *cp16, float *out_16n);

/* That constant: cp16 = OPENGL_TO_WGPU_MATRIX * cgmath::perspective(Deg(vertical_fov_deg), aspect_ratio, near, far), 16 floats,
 * column-major (src/gfx.rs:12-17, 365, 367; the reference passes near = 1, far = 10000 and vertical_fov = horizontal_fov /
 * aspect_ratio, src/gfx.rs:381).  Host arithmetic, no device needed; NB_ERR_INVALID where cgmath's assertions would panic. */
int nb_camera_constant(float vertical_fov_deg, float aspect_ratio, float near_plane, float far_plane, float *cp16);

/* Every entity's eye view: what the reference's depth attachment holds after its eye pass -- one 1 x width
 * layer per entity, the camera on the entity looking along its velocity (src/main.rs:939, 585-647, 962-998), every instance drawn
 * in index order as the LineStrip 0-1-2-0 of its triangle (:130-138, 249), Depth32Float cleared to 1.0, compare Less (:256-260,
 * 626) -- and which instance wrote each pixel.  Per column: the nearest body's id (ties: the lower index) and its depth, or
 * NB_EYES_NONE and 1.0f.  The eye's own body is skipped unless NB_EYES_SEE_SELF (the `n != i` of the controllers).  The colour
 * attachment is nb_eyes_colour's, below.  MSAA is not reproduced here: one sample at the column centre (the 8-sample rows are
 * nb_eyes_msaa's, further below).  Bit-exact: a fixed binary32 rule, clip = cp * view * (model * vertex). */
#define NB_EYES_NONE 0xFFFFFFFFu
#define NB_EYES_SEE_SELF 1u
#define NB_EYES_MAX_WIDTH 4096u
/* eyes of bodies [first, first+count) of the context's current state: cameras from (up, cp16) as nb_cameras (the reference's eye
 * constant: nb_camera_constant(90.0f / width, width / 1.0f, 1, 10000)), the rule above; ids / depth: host, count*width each,
 * either may be NULL (not both).  count = 0 is a no-op.  Device rows are allocated on the context at first use. */
int nb_eyes(nb_ctx *ctx, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16, uint32_t width, uint32_t flags,
            uint32_t *ids, float *depth);

/* The colour row of the same pass: what `resolved_eyes` and the viewport's imgui texture hold
 * (src/main.rs:585-647, 962-998), one 1 x width Bgra8UnormSrgb layer per entity.  The fragment of a column is that of the FIRST
 * edge (draw order 0-1, 1-2, 2-0; Less keeps the first of equal depths) of the winning body that covers the column with the winning
 * depth; its texture coordinate is interpolated perspective-correctly along the clipped edge from the vertices' (0,0), (0,1), (1,1)
 * (shaders/scene.vert:17, src/main.rs:131-135), one texel of the skin is fetched, the vignette c = tex * (1 - |uv - 0.5|^2) applied
 * (shaders/scene.frag:15-16), alpha = 1; an empty column holds the clear colour (0.1, 0.2, 0.3, 1) (:613-618).
 *   rgba    4 floats per column, linear: what the shader writes
 *   bgra8   one uint32 per column whose bytes in memory are B, G, R, A: the texel the sRGB target stores (nb_srgb_encode below)
 * NOT reproduced: the MSAA resolve (one sample at the column centre, as for the depth; nb_eyes_msaa below resolves 8) and the
 * sampler's linear minification (src/main.rs:362) -- which fragments count as minified depends on screen-space derivatives that a line primitive in a one-pixel-
 * high target does not define portably; the texel is ClampToEdge with ONE nearest sample, ix = min(tw - 1, floor(u * tw)),
 * iy = min(th - 1, floor(v * th)). */
#define NB_EYES_MAX_SKIN 2048u
/* The skin the context's colour rows sample: tw x th texels of linear RGBA floats, row 0 first as the image file stores it
 * (1 <= tw, th <= NB_EYES_MAX_SKIN), copied to the device and kept by the context.  NULL, or never called: a 1 x 1 white skin,
 * which gives the pure vignette (tw, th are ignored).  An 8-bit sRGB image (Rgba8UnormSrgb, src/main.rs:338) becomes linear
 * through nb_srgb_decode_table. */
int nb_eyes_skin(nb_ctx *ctx, const float *rgba_linear, uint32_t tw, uint32_t th);
/* nb_eyes with the colour row: ids / depth as nb_eyes gives them, bit for bit; rgba: host, count*width*4 floats; bgra8: host,
 * count*width words.  Any of the four may be NULL, but not both rgba and bgra8 (that call is nb_eyes).  count = 0 is a no-op. */
int nb_eyes_colour(nb_ctx *ctx, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16, uint32_t width, uint32_t flags,
                   uint32_t *ids, float *depth, float *rgba, uint32_t *bgra8);
/* The two sRGB tables behind bgra8 and an 8-bit skin; host arithmetic on committed constants, no device needed.
 * decode = the sRGB EOTF: e / 12.92 for e <= 0.04045, else ((e + 0.055) / 1.055)^2.4.
 *   nb_srgb_decode_table   out256[b] = binary32(decode(b / 255))
 *   nb_srgb_encode         out[i] = the number of thresholds T[1..255] that are <= linear[i], T[b] = binary32(decode((b - 0.5) / 255)):
 *                          the exact nearest byte; a NaN gives 0, anything >= T[255] gives 255 */
int nb_srgb_decode_table(float *out256);
int nb_srgb_encode(const float *linear, size_t n, uint8_t *out);

/* The eye rows through 8 samples per column, resolved: the reference renders every target
 * with msaa_samples = 8 and resolves it (src/main.rs:652, 263, 547, 611), so a span end covers a fraction of its column and a
 * column where two bodies meet holds a mix of both.  Sample k of column c lies at x = c + o[k], o = (9, 7, 13, 5, 3, 1, 11, 15) / 16
 * (the x coordinates of Vulkan's standard 8-sample pattern; nb_eyes_sample_offsets); coverage, depth, the winning body and its edge
 * are nb_eyes' and nb_eyes_colour's rule per sample; there is one fragment per column, body and edge, shaded at the column centre
 * c + 0.5 whether or not the centre is covered (no sample-rate shading); the column is the mean of its eight samples' colours, the
 * clear colour where a sample is empty, summed as a tree: (((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7))) * 0.125f.
 *   ids8, depth8   count*width*8 words each, sample k of column c of eye e at (e*width + c)*8 + k; empty: NB_EYES_NONE and 1.0f
 *   rgba, bgra8    the resolved rows, shaped as nb_eyes_colour's
 * Any output may be NULL, one at least.  The skin is the context's (nb_eyes_skin).  1 <= width <= NB_EYES_MSAA_MAX_WIDTH: an eye's
 * samples are resolved in the 160 KB of LDS of one compute unit.  count = 0 is a no-op.  Bit-exact, the same bits from run to run. */
#define NB_EYES_SAMPLES 8u
#define NB_EYES_MSAA_MAX_WIDTH 2048u
int nb_eyes_sample_offsets(float *out8);   /* host arithmetic, no device */
int nb_eyes_msaa(nb_ctx *ctx, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16, uint32_t width, uint32_t flags,
                 uint32_t *ids8, float *depth8, float *rgba, uint32_t *bgra8);

/* What a controller makes of the eye rows.  The SEEN SET of an eye is formed from its resolved row (ids[c],
 * depth[c] as nb_eyes leaves them): the values other than NB_EYES_NONE that occur in ids, compared as unsigned 32-bit numbers.
 *   seen_count[e]          their number, at most width
 *   seen_ids[e*width + k]  k < count: the members in ascending order; the other slots read NB_EYES_NONE
 *   seen_depth[...]        the value whose bit pattern is the unsigned minimum of the bit patterns of depth[c] over the member's
 *                          columns: on a resolved row the nearest depth at which e sees the body; the other slots read 1.0f
 *   seen_cols[...]         the number of columns holding the member; the other slots read 0
 * A function of the row alone: the same bits from run to run.
 * nb_eyes_seen: the seen sets of the eyes of bodies [first, first+count) of the context's current state, rows as nb_eyes forms them
 * (flags may be NB_EYES_SEE_SELF).  Host outputs: seen_count count words, the others count*width; any may be NULL, not all.
 * count = 0 is a no-op. */
int nb_eyes_seen(nb_ctx *ctx, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16, uint32_t width, uint32_t flags,
                 uint32_t *seen_count, uint32_t *seen_ids, float *seen_depth, uint32_t *seen_cols);

/* k applications of update_instance_boids (src/main.rs:443-526) restricted to what each entity SEES, device-resident and
 * asynchronous on the context's stream; may be mixed freely with the other steps.  One application to the state (P, V):
 *   V1  the eye rows of every body as nb_eyes forms them from (P, V) with flags = 0 (cameras from up_xyz, cp16 as nb_cameras; an eye
 *       does not see its own body), and their seen sets
 *   V2  body n runs the three folds of main.rs:471-504 with the same operations, operand order and predicates over the entries of
 *       its seen list in list order (ascending body index) instead of over old_positions / old_velocities .iter().enumerate()
 *   V3  the epilogue of main.rs:506-521, unchanged
 * A body that sees nobody gets velocity (0, 0, 0) and stays where it is -- the reference's law applied to an empty fold.
 * Eyes are processed `batch` at a time, which bounds the device rows and lists; every batch size gives the same bits.  batch = 0:
 * the library's choice, the most eyes whose id rows and lists (8 bytes a column, 4 bytes of count an eye) stay together at or below
 * 64 MiB -- 8 188 at width 1024.  params == NULL -> defaults.  1 <= width <= NB_EYES_MAX_WIDTH. */
int nb_step_boids_seen(nb_ctx *ctx, uint32_t k, const nb_boids_params *params, const float *up_xyz, const float *cp16, uint32_t width,
                       uint32_t batch);

/* WHERE an eye sees what it sees.  A resolved row holds a bearing (the column) and a range (the depth): the
 * LOCATED seen set of eye e gives, per member of its seen set, the column at which the member is nearest and the seen point relative
 * to the eye in world axes -- formed from the eye's own row, its own heading (its velocity record), `up` and the eyes' camera constant,
 * from no body's position, not even its own.  Every step one binary32 operation, round to nearest, in the order written:
 *   L1  seen_col[e*width + k], k < count: the least column c with ids[c] == seen_ids[k] and bits(depth[c]) == bits(seen_depth[k]);
 *       no such column (a list that is not of this row): NB_EYES_NONE, and seen_rel[k] = four +0 words
 *   L2  h = width*0.5; xc = c + 0.5; xn = (xc - h)/h; r = cp16[14] / (d + cp16[10]), d = seen_depth[k]; xv = (xn*r) / cp16[0]
 *   L3  f = normalize(dir), s = normalize(f x up) as nb_cameras forms them (products first, one subtraction per component;
 *       normalize(x) = x * (1 / sqrt((x0*x0 + x1*x1) + x2*x2)))
 *   L4  seen_rel[(e*width + k)*4 ..] = (r*f0 + xv*s0, r*f1 + xv*s1, r*f2 + xv*s2, r): two products and one sum per component
 *   L5  the slots k >= count: seen_col = NB_EYES_NONE, seen_rel = (+0, +0, +0, +0)
 *   L6  L2 inverts cp16 * view only for a perspective constant of the shape nb_camera_constant produces: cp16[11] == -1,
 *       cp16[1,2,3,4,6,7,8,9,12,13,15] all zero, cp16[0] != 0, cp16[14] != 0; any other constant is NB_ERR_INVALID (the eye rows
 *       themselves accept any matrix: only the located entries refuse)
 * A row is one pixel high: the estimate lies in the plane through the eye spanned by f and s -- on planar data the data's plane, where
 * it is a point of the seen body's outline (within sqrt(2) of its centre, plus the depth buffer's resolution at that range).  A
 * function of the row and the list: the same bits from run to run.
 * nb_eyes_located: rows, seen sets and located sets of the eyes of bodies [first, first+count) of the context's current state, checks
 * and staging as nb_eyes_seen.  Host outputs: seen_count count words; seen_ids, seen_depth, seen_cols, seen_col count*width words;
 * seen_rel count*width*4 floats; any may be NULL, not all.  count = 0 is a no-op. */
int nb_eyes_located(nb_ctx *ctx, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16, uint32_t width, uint32_t flags,
                    uint32_t *seen_count, uint32_t *seen_ids, float *seen_depth, uint32_t *seen_cols, uint32_t *seen_col, float *seen_rel);

/* k applications of update_instance_nbody (src/main.rs:404-441) from VISION ALONE, device-resident and asynchronous on the context's
 * stream; may be mixed freely with the other steps.  One application to the state (P, V), with the context's nb_params (dt, G, bias):
 *   G1  cameras, model matrices, eye rows with flags = 0 (ids and depth), seen sets with depth and located sets of every body, as
 *       nb_eyes_located forms them from (P, V)
 *   G2  body n starts sum = (0, 0, 0) and walks its slots in slot order: vec = seen_rel[k].xyz;
 *       dist = ((vec.x*vec.x + vec.y*vec.y) + vec.z*vec.z) + bias; sum = sum + (vec*G)/dist per component -- the operations and
 *       operand order of main.rs:428-430 with vec supplied by the row instead of p_i - p_n
 *   G3  v = v + sum*dt; p = v + p (main.rs:434-436)
 * A body that sees nobody coasts.  Eyes are processed `batch` at a time; every batch size gives the same bits.  batch = 0: the
 * library's choice, the most eyes whose id and depth rows, list ids and depths, seen_rel and count (32 bytes a column, 4 bytes an eye)
 * stay together at or below 64 MiB -- 2 047 at width 1024.  1 <= width <= NB_EYES_MAX_WIDTH; cp16 as L6 asks. */
int nb_step_nbody_located(nb_ctx *ctx, uint32_t k, const float *up_xyz, const float *cp16, uint32_t width, uint32_t batch);

/* ---- scene batches ------------------------------------------------------------------------------------
 * A scene batch is `scenes` >= 1 independent scenes of n bodies each, 1 <= n <= NB_SCENES_MAX_BODIES; body i of scene s is record
 * s*n + i of the 16-byte position and velocity records (and of the 16-float model matrices).  scenes*n <= 2^27, more is
 * NB_ERR_UNSUPPORTED.  One launch steps every scene k times, one workgroup per scene, the scene's state on chip between the steps:
 *   B1  gravity: scene s gets exactly the records nb_step(ctx, k) gives a context of n bodies created with the same nb_params and
 *       uploaded with scene s's records -- every bit.  STRICT only: NB_MODE_FAST is NB_ERR_UNSUPPORTED.  params.tile is validated
 *       and otherwise unused.
 *   B2  boids: the same against nb_step_boids(ctx, k, params) (the radius thresholds are those of a set of n bodies)
 *   B3  no scene's result depends on another scene's records, on `scenes`, or on whether k steps come as one launch or as k
 *   B4  the stateless entries update pos and vel in place */
#define NB_SCENES_MAX_BODIES 2048u

/* k steps of a batch on caller-owned device memory, in place, one kernel on `stream`: pos, vel: scenes*n records each, 16-byte
 * aligned, not overlapping.  params == NULL -> defaults.  k = 0 is a checked no-op. */
int nb_scenes_nbody_step_launch(const nb_params *params, uint32_t scenes, uint32_t n, uint32_t k, void *pos, void *vel, void *stream);
int nb_scenes_boids_step_launch(const nb_boids_params *params, uint32_t scenes, uint32_t n, uint32_t k, void *pos, void *vel, void *stream);

typedef struct nb_scenes nb_scenes; /* opaque; owns a batch's device buffers and its stream */

/* params == NULL -> defaults; checked as B1 asks.  Errors from a NULL context or from nb_scenes_create are read with
 * nb_scenes_last_error(NULL), a context's own with nb_scenes_last_error(ctx). */
int nb_scenes_create(uint32_t scenes, uint32_t n, const nb_params *params, nb_scenes **out);
void nb_scenes_destroy(nb_scenes *ctx);
/* pos_xyz, vel_xyz: stride-3 host arrays of 3*scenes*n floats, scene after scene, as nb_upload takes one set's */
int nb_scenes_upload(nb_scenes *ctx, const float *pos_xyz, const float *vel_xyz);
/* k steps of every scene, asynchronous on the context's stream; the two may be mixed freely.  NB_ERR_STATE before an upload. */
int nb_scenes_step(nb_scenes *ctx, uint32_t k);
int nb_scenes_step_boids(nb_scenes *ctx, uint32_t k, const nb_boids_params *params);
/* any output may be NULL, but not all three; inst_16: 16*scenes*n floats, the model matrices of every body (nb_download's) */
int nb_scenes_download(nb_scenes *ctx, float *pos_xyz, float *vel_xyz, float *inst_16);
/* the batch's device records, as nb_device_state hands out a set's (valid until the next step or upload; work on another stream
 * orders itself behind nb_scenes_sync): scene s starts s*n records (s*n matrices) behind each pointer, so nb_launch_cameras /
 * nb_launch_eyes run on one scene with n_total = n and offset pointers.  Any of the three may be NULL. */
int nb_scenes_device_state(nb_scenes *ctx, const void **pos_rec, const void **vel_rec, const void **inst_16);
int nb_scenes_sync(nb_scenes *ctx);
uint64_t nb_scenes_steps(const nb_scenes *ctx); /* steps applied since the last upload */
const char *nb_scenes_last_error(const nb_scenes *ctx);

/* ---- scene batches: the boids step over what each body sees -----------------------------------------
 * The eye set-up is (up_xyz, cp16, width) as nb_step_boids_seen takes it, 1 <= width <= NB_EYES_MAX_WIDTH.  One kernel per step
 * for the whole batch: the eye's row and its seen set stay on chip, no row and no list is written to device memory.
 *   SV1  k applications give scene s exactly the records nb_step_boids_seen(ctx, k, params, up_xyz, cp16, width, 0) gives a context
 *        of n bodies uploaded with scene s's records -- every bit.  An eye sees only bodies of its own scene, ids are scene-local
 *        (0 .. n-1), an eye does not see its own body (flags = 0), the radius thresholds are those of a set of n bodies; a body that
 *        sees nobody gets velocity (0, 0, 0) and stays where it is
 *   SV2  no scene's result depends on another scene's records, on `scenes`, on the grid, on the launch shape chosen for n, or on how
 *        k steps are split over calls
 *   SV3  the seen sets the step folds over are observable: eye i of scene s has seen_count and width slots of seen_ids, the words
 *        nb_eyes_seen gives a context holding that scene (S1-S3): members ascending, NB_EYES_NONE behind the count.  seen_depth and
 *        seen_cols are NOT offered: the step keeps only which ids occur in a row (a bitmap), not their depths or column counts
 *   SV4  the same bits from run to run */

/* The four entries are declared in nenbody_scenes_seen.h, which this header includes: nb_scenes_boids_seen_step_launch and
 * nb_scenes_seen_launch on caller-owned device memory, nb_scenes_step_boids_seen and nb_scenes_eyes_seen on a context. */
#include "nenbody_scenes_seen.h"

/* ---- scene batches: gravity from located vision ----------------------------------------------------
 * The eye set-up is (up_xyz, cp16, width) as nb_step_nbody_located takes it, 1 <= width <= NB_EYES_MAX_WIDTH; dt, G and bias are
 * nb_params'.  One kernel per step for the whole batch: the eye's row, its members' depths and columns, the located points and the
 * quotients stay on chip.
 *   SL1  k applications give scene s exactly the records nb_step_nbody_located(ctx, k, up_xyz, cp16, width, batch) gives a context of
 *        n bodies uploaded with scene s's records -- every bit, for any batch.  An eye sees only bodies of its own scene, ids are
 *        scene-local (0 .. n-1), an eye does not draw its own body (flags = 0); a body that sees nobody coasts (G3); a body with
 *        zero or non-finite velocity sees nobody, and its own record still takes G3
 *   SL2  no scene's result depends on another scene's records, on `scenes`, on the grid, on the launch shape chosen for n, or on how
 *        k steps are split over calls
 *   SL3  the located sets the step folds over are observable: eye i of scene s has seen_count and width slots each of seen_ids,
 *        seen_depth, seen_col and seen_rel (16 bytes a slot), the words nb_eyes_located gives a context holding that scene (S1-S3,
 *        L1-L5), padding included: NB_EYES_NONE for ids and col, 1.0f for depth, four +0 words for rel.  seen_cols, the column
 *        count, is NOT offered: the step keeps a member's nearest depth and its column, not how many columns hold it
 *   SL4  the same bits from run to run
 *   SL5  L6 holds: a cp16 that cannot be inverted is refused on the host, with L6's texts behind the entry's name, before the
 *        device is touched */

/* The four entries are declared in nenbody_scenes_located.h, which this header includes: nb_scenes_nbody_located_step_launch and
 * nb_scenes_located_launch on caller-owned device memory, nb_scenes_step_nbody_located and nb_scenes_eyes_located on a context. */
#include "nenbody_scenes_located.h"

/* ---- scene batches: a neural policy over each body's eye row ----------------------------------------
 * A controller of the caller's own: a small two-layer network reads a pooled depth row and outputs thrust and turn in the eye's own
 * frame; either one network is shared or each scene has its own.  One kernel per step for the whole batch: the row, the features and
 * the hidden layer stay on chip.  Every step below is one binary32 operation, round to nearest, in the order written; there is no
 * contraction: a product is rounded before it is added.
 * The eye set-up is (up_xyz, cp16, width) as nb_scenes_step_boids_seen takes it.  A policy shape (F, H) has
 * 1 <= F <= NB_POLICY_MAX_FEATURES, F dividing width, 1 <= H <= NB_POLICY_MAX_HIDDEN.  One policy is F*H + H + 2*H + 2 floats:
 * w1[f*H + j], b1[j], w2[k*H + j] for k = 0, 1, b2[k].  `policies` is 1 (every scene uses policy 0) or `scenes` (scene s uses policy
 * s).  A limit L >= 0 (accel_limit) applies to the outputs; +inf means no limit.  For body i of scene s, from the snapshot (P, V):
 *   P1  row: the eye row as nb_eyes forms it with flags = 0; it covers the bodies of its own scene only (SV1's first sentence)
 *   P2  features: bin f covers columns [f*W/F, (f+1)*W/F); d_f is the value whose bits are the unsigned minimum of the depth bits
 *       over the bin's non-empty columns, 1.0f if the bin has none; x_f = 1.0f - d_f: an empty bin gives +0, nearer gives larger
 *   P3  hidden: t_j = b1[j]; then for f = 0 .. F-1 in order t_j = t_j + (w1[f*H + j] * x_f); h_j = (t_j > 0) ? t_j : +0, so a NaN
 *       gives +0
 *   P4  outputs: o_k = b2[k]; then for j = 0 .. H-1 in order o_k = o_k + (w2[k*H + j] * h_j); then
 *       o_k = (o_k < -L) ? -L : ((o_k > L) ? L : o_k), so a NaN passes through
 *   P5  actuation: f and s of the eye are as L3 forms them from the body's velocity record and up.  If any of their six components
 *       is not finite -- a zero velocity, a non-finite velocity, a velocity parallel to up -- a = (+0, +0, +0) and the body coasts;
 *       otherwise a_c = (o_0 * f_c) + (o_1 * s_c)
 *   P6  integration: v = v + a*dt; p = v + p, with dt from nb_params.  G, bias and mode do not enter, but are validated as the
 *       other entries validate them
 *   P7  no scene's result depends on another scene's records or policy, on `scenes`, on the grid, on the launch shape chosen for n,
 *       or on how k steps are split over calls; the same bits from run to run
 *   P8  per eye the F words of x and the two words of o (behind the limit) are observable without stepping */
#define NB_POLICY_MAX_FEATURES 256u
#define NB_POLICY_MAX_HIDDEN 64u

/* The six entries are declared in nenbody_scenes_policy.h, which this header includes: nb_policy_floats, the stateless
 * nb_scenes_policy_step_launch and nb_scenes_policy_observe_launch on caller-owned device memory, and nb_scenes_set_policy,
 * nb_scenes_step_policy and nb_scenes_eyes_policy on a context. */
#include "nenbody_scenes_policy.h"

/* ---- scene batches: the score of every scene, accumulated on the device -------------------------------
 * What a tuner compares between the policies of a population: per scene, the current snapshot reduced to a fixed record of metrics
 * and added to a record the scene keeps in device memory; the host reads 32 bytes a scene when the rollout ends.  Every float
 * operation below is one binary32 operation, round to nearest, in the order written; there is no contraction, and subnormals are
 * kept.  There is no square root and no library function.  Which NaN an operation gives is not part of the rule: a field that is a
 * NaN is a NaN, of any sign and payload.
 * Inputs: a batch as above; the snapshot (P, V) of scene s, of which only x, y, z of a record enter; radius_sq >= 0 (not a NaN; +inf
 * admitted) and goal[3], finite.
 *   Q1:  the tree sum T(u) of n leaves: P is the smallest power of two >= n; u_i = +0 for n <= i < P; for stride = P/2, P/4, .., 1:
 *        u_i = u_i + u_{i+stride} for every i < stride; T = u_0.  An add whose right operand is padding may be skipped, and a tree
 *        over a larger power of two may be run: either changes at most the sign of a zero sum, which Q3-Q6 cannot observe
 *   Q2:  near = the number of unordered pairs i < j with d2 < radius_sq, d2 = ((dx*dx) + (dy*dy)) + (dz*dz), dx = p_i.x - p_j.x and
 *        likewise dy, dz: bitwise symmetric in i and j; a NaN compares false
 *   Q3:  spread: c_x = T(p.x) / (float)n, the IEEE quotient, likewise c_y, c_z; e_i = ((ex*ex) + (ey*ey)) + (ez*ez), ex = p_i.x - c_x
 *        and likewise ey, ez; spread = T(e)
 *   Q4:  speed2 = T(((vx*vx) + (vy*vy)) + (vz*vz)); m_c = T(v.c) for the three components; momentum2 = ((m_x*m_x) + (m_y*m_y)) +
 *        (m_z*m_z)
 *   Q5:  goal2 = T of Q3's squared distance with goal in place of c
 *   Q6:  nonfinite = the number of bodies with a non-finite component among the six of (P, V)
 *   Q7:  accumulation into the scene's nb_scene_score: near += near, exact; every float field acc = acc + term, one add, in call
 *        order; steps += 1 and nonfinite += nonfinite, modulo 2^32.  All-zero bytes are the cleared state.  No scene's record
 *        depends on another scene, on `scenes`, on the grid, on the workgroup shape, or on how the snapshots are split over calls;
 *        the same bits from run to run */
typedef struct nb_score_params {
    float radius_sq; /* Q2 */
    float goal[3];   /* Q5 */
} nb_score_params;
typedef struct nb_scene_score {
    uint64_t near;
    float spread, speed2, momentum2, goal2;
    uint32_t steps, nonfinite;
} nb_scene_score; /* 32 bytes */

/* The six entries are declared in nenbody_scenes_score.h, which this header includes: the stateless nb_scenes_score_launch on
 * caller-owned device memory, and nb_scenes_set_score, nb_scenes_score, nb_scenes_score_reset, nb_scenes_scores and
 * nb_scenes_step_policy_scored on a context. */
#include "nenbody_scenes_score.h"

/* ---- scene batches: an evolution-strategies generation on the device ----------------------------------
 * The tuner behind the policy and the score: the population of a generation drawn from a mean by a counter-based generator, the
 * scenes' score records ranked, the mean moved along the rank-weighted sum of the draws.  Every step is asynchronous on a stream;
 * every float operation below is one binary32 operation, round to nearest, in the order written, with no contraction and subnormals
 * kept; every sum is an exact integer.  The bits depend on (seed, generation, scene, weight index) and on nothing else.
 * M = nb_policy_floats(F, H) for a policy shape (F, H) within the limits; B = scenes, 1 <= B <= NB_ES_MAX_POPULATION.  Parameters
 * nb_es_params: sigma >= 0 and finite; step finite; coef[6] finite; seed, 64 bits.  g is the generation, a 32-bit word.  All words
 * below are unsigned 32-bit words unless said otherwise; hi and lo are the halves of a 64-bit product.
 *   E1:  the generator is Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011).  M0 = 0xD2511F53, M1 = 0xCD9E8D57; the key (k0, k1) starts
 *        as (seed & 0xFFFFFFFF, seed >> 32).  One round maps the counter (c0, c1, c2, c3) to
 *        (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)).  Ten rounds; between two rounds (nine times) the key is
 *        bumped: k0 += 0x9E3779B9, k1 += 0xBB67AE85, modulo 2^32.  For scene s and weight m the counter is (m >> 1, s >> 1, g, 0);
 *        the output is (x0, x1, x2, x3).  Counter 0 under key 0 gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *   E2:  the draw: (a, b) = (x0, x1) for even m, (x2, x3) for odd m; k = (a & 0xFFFF) + (a >> 16) + (b & 0xFFFF) + (b >> 16) - 131070,
 *        an integer in [-131070, 131070], a centred sum of four 16-bit uniforms.  Scenes 2q and 2q+1 are mirrored:
 *        k(s, m) = (s & 1) ? -k : k.  e = (float)k * C, C the binary32 value with the bits 0x37DDB3D7 (sqrt(3) * 2^-16, one over the
 *        standard deviation of k); (float)k is exact
 *   E3:  the population: theta[s*M + m] = mean[m] + (sigma * e): two operations
 *   E4:  the fitness of scene s from its nb_scene_score, larger is better: phi = +0; then over the fields in the order (float)near,
 *        spread, speed2, momentum2, goal2, (float)nonfinite: phi = phi + (coef[i] * field_i).  A term whose coefficient is +0 or -0 is
 *        skipped, so a field the caller does not weigh may be infinite or a NaN.  (float)near and (float)nonfinite are the integer
 *        rounded to nearest even ONCE; a route through binary64 rounds near twice above 2^53 and is wrong.  As the sum starts from
 *        +0, phi is never -0: a -0 term gives +0.  Which NaN a NaN phi is, is not part of the rule
 *   E5:  the rank: key32 = 0 for a NaN phi; otherwise, w being the bits of phi, key32 = ~w where w has its sign bit set and
 *        w | 0x80000000 where it has not: monotone in phi, -0 below +0, a NaN below everything.  key64 = key32 << 32 | s.
 *        r_s = the number of scenes t with key64_t < key64_s: a permutation of 0 .. B-1, ties broken by scene index
 *   E6:  the utility: u_s = 2*r_s - (B - 1), an integer; the utilities sum to 0
 *   E7:  the update: A_m = the sum over s of u_s * k(s, m), an EXACT integer, |A_m| < 2^42, in any order;
 *        mean'[m] = mean[m] + (step * ((float)A_m * C)), (float)A_m rounded to nearest even once.  The caller folds the learning
 *        rate, 1/(B*sigma) and the scale of the utilities into step.  B = 1 has u_0 = 0 and leaves the mean as it is but for -0,
 *        which becomes +0 under a step of +0 or above
 *   E8:  theta of scene s does not depend on B; no word depends on the grid, the workgroup shape, on how scenes or weights are split
 *        over launches, or on the run
 * The ranking also writes a report: best_scene is the scene of rank B-1, best_fitness its phi, nan_count the number of scenes whose
 * phi is a NaN, generation the g it ranked.
 * Decisions where the rule's source left a choice: the stateless update takes the mean it reads and the mean it writes as two
 * arguments, which may be the same pointer (in place) and may otherwise not overlap; nb_scenes_es_result before the first
 * nb_scenes_es_update is NB_ERR_STATE; the context's generation counts modulo 2^32. */
#define NB_ES_MAX_POPULATION 4096u
typedef struct nb_es_params {
    float sigma;   /* E3 */
    float step;    /* E7 */
    float coef[6]; /* E4: near, spread, speed2, momentum2, goal2, nonfinite */
    uint64_t seed; /* E1 */
} nb_es_params;    /* 40 bytes */
typedef struct nb_es_report {
    uint32_t best_scene;
    float best_fitness;
    uint32_t nan_count;
    uint32_t generation;
} nb_es_report; /* 16 bytes */

/* The ten entries are declared in nenbody_scenes_es.h, which this header includes: the stateless nb_scenes_es_perturb_launch and
 * nb_scenes_es_update_launch on caller-owned device memory, and nb_scenes_es_set, nb_scenes_es_perturb, nb_scenes_es_update,
 * nb_scenes_es_mean, nb_scenes_es_result, nb_scenes_es_generation, nb_scenes_keep and nb_scenes_rewind on a context. */
#include "nenbody_scenes_es.h"

/* ---- scene batches: a recurrent policy with per-body memory -------------------------------------------
 * The policy of P1-P8 sees one pooled depth row: bearing and range, no rate, and nothing of a neighbour that has left the slit.
 * Here every body also owns H words of memory in device memory; the hidden layer reads the features and the memory, and the
 * memory of the next step is the hidden layer, limited.  One kernel per step for the whole batch, as there.  Every step below is
 * one binary32 operation, round to nearest, in the order written; there is no contraction: a product is rounded before it is
 * added.  The notation, the limits on (F, H), the eye set-up and `policies` in {1, scenes} are those of P1-P8.
 *   R1  one recurrent policy of shape (F, H) is nb_policy_recurrent_floats(F, H) = F*H + H*H + H + 2*H + 2 floats, in this order:
 *       w1[f*H + j], wr[r*H + j], b1[j], w2[k*H + j] for k = 0, 1, b2[k].  wr[r*H + j] weighs memory word r into hidden unit j: it
 *       is source-major, as w1 is.  At the limits (256, 64) this is 20 674 floats
 *   R2  memory: every body owns H binary32 words m_r; the batch's memory is scenes*n*H words, body b = s*n + i at b*H.  It is all +0
 *       initially and after a reset.  The features x_f are those of P1-P2
 *   R3  hidden: t_j = b1[j]; then for f = 0 .. F-1 in order t_j = t_j + (w1[f*H + j] * x_f); then for r = 0 .. H-1 in order
 *       t_j = t_j + (wr[r*H + j] * m_r); then h_j = (t_j > 0) ? t_j : +0, so a NaN gives +0
 *   R4  new memory: m'_j = (h_j > S) ? S : h_j, with a memory limit S >= 0 (memory_limit; +inf: none).  R3 never yields a NaN, so
 *       m' lies in [+0, S] whatever the old memory held
 *   R5  outputs and motion: o_k comes from h (NOT from m') exactly as in P4; the acceleration and the integration are exactly P5-P6.
 *       A body that coasts under P5 still takes its new memory
 *   R6  (a consequence, stated and tested) with every word of wr equal to +0 and every memory word finite, positions and velocities
 *       are those of the P-rule policy (w1, b1, w2, b2), bit for bit: t + (+0 * m) leaves every t except -0 alone, and -0 and +0
 *       both give h = +0
 *   R7  P7; additionally k steps in one call equal any split of them over calls with the memory carried.  The memory may be updated
 *       in place: an eye reads and writes only its own H words
 *   R8  per eye the F words of x, the two words of o and the H words of m' are observable without stepping and without changing
 *       the memory
 * Decisions where the rule left a choice.  nb_scenes_keep and nb_scenes_rewind are unchanged and do NOT touch the memory, so a
 * generation of a search over a recurrent policy is six asynchronous calls: nb_scenes_rewind, nb_scenes_memory_reset,
 * nb_scenes_score_reset, nb_scenes_es_perturb, nb_scenes_step_policy_scored(k), nb_scenes_es_update.  nb_scenes_upload does not
 * clear the memory.  nb_scenes_step and the other laws leave the memory alone. */
#define NB_ES_MAX_FLOATS 20674u /* nb_policy_recurrent_floats at the limits: the longest mean of a search */

/* The eleven entries are declared in nenbody_scenes_policy_recurrent.h, which this header includes: nb_policy_recurrent_floats,
 * the stateless nb_scenes_policy_recurrent_step_launch, nb_scenes_policy_recurrent_observe_launch,
 * nb_scenes_es_perturb_floats_launch and nb_scenes_es_update_floats_launch on caller-owned device memory, and
 * nb_scenes_set_policy_recurrent, nb_scenes_eyes_policy_memory, nb_scenes_memory_reset, nb_scenes_memory, nb_scenes_set_memory and
 * nb_scenes_es_set_recurrent on a context. */
#include "nenbody_scenes_policy_recurrent.h"

/* The scene camera's frame: what the reference's display pass leaves in its width x height target
 * (src/main.rs:948-960) -- every instance's LineStrip triangle through ONE camera, the eye passes' pipeline otherwise: depth test
 * Less against a clear of 1.0, the skin (nb_eyes_skin) under the vignette, the clear colour, a Bgra8UnormSrgb target -- and which
 * instance wrote each pixel.  The eye rule carries over (clip, projection, depth, key, texture coordinate, vignette, sRGB byte) with a
 * second screen axis, ys = H/2 - (y / w) * H/2, row 0 the top: an edge is walked along its major axis (x iff |dx| >= |dy|), one
 * pixel per column (or row) whose centre lies in the half-open interval between the projected ends.  There is no "self" to skip, so
 * flags must be 0.  An empty pixel reads NB_EYES_NONE and 1.0f and the clear colour.  One sample per pixel, at its centre: no MSAA resolve
 * HERE (the frame resolved from 8 samples per pixel, as the reference's is, is nb_frame_msaa's, below, as the eyes' rows are
 * nb_eyes_msaa's), no linear minification.  Bit-exact, and the same bits from run to run. */
#define NB_FRAME_MAX_DIM 4096u
/* One camera from a host-supplied eye and direction, out16 = cp16 * look_at_dir(eye, dir, up), through the kernel nb_cameras runs
 * (its count 1): the reference's scene camera is eye (p.x, p.y, 990) above the body it follows, dir (0, 0, -1), up (1, 0, 0),
 * cp16 = nb_camera_constant(90.0f / a, a, 1, 10000) with a = (float)width / (float)height (src/main.rs:753-762, 940-942). */
int nb_camera_at(nb_ctx *ctx, const float *eye_xyz, const float *dir_xyz, const float *up_xyz, const float *cp16, float *out16);
/* The frame of the context's current state through cam16 (host, 16 floats, column-major), with the context's skin.  ids / depth /
 * bgra8: host, height*width each, row 0 first; rgba: host, height*width*4 floats.  Any may be NULL, one at least.  The device rows
 * and the key plane are the context's, allocated at first use and grown on demand. */
int nb_frame(nb_ctx *ctx, const float *cam16, uint32_t width, uint32_t height, uint32_t flags, uint32_t *ids, float *depth, float *rgba,
             uint32_t *bgra8);

/* The frame through 8 samples per pixel, resolved: the reference builds its display target
 * with msaa_samples = 8 and resolves it into the swapchain image (src/main.rs:652, 685-690, 545-548), so a width-1 line that
 * crosses a pixel off-centre still shows there, and a pixel where two bodies meet holds a mix of both.  Sample k of pixel (c, r)
 * lies at (c + ox[k], r + oy[k]), ox = (9, 7, 13, 5, 3, 1, 11, 15) / 16 (nb_eyes_sample_offsets'), oy = (5, 11, 9, 3, 13, 7, 15, 1) / 16:
 * Vulkan's standard 8-sample pattern (nb_frame_sample_offsets).  nb_frame's clip, projection and major axis are unchanged; along
 * its major axis an edge tries sample k of step m iff m + oa[k] lies between the projected ends, and the sample belongs to the
 * pixel whose minor index is floor(o + 0.5 - ob[k]), o the line's minor coordinate there: the line is one pixel wide.  Depth, the
 * winning body and its edge are nb_frame's rule per sample; there is one fragment per pixel, body and edge, shaded at the pixel
 * centre whether or not the centre is covered; the pixel is the mean of its eight samples' colours, the clear colour where a
 * sample is empty, summed as a tree: (((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7))) * 0.125f.
 *   ids8, depth8   height*width*8 words each, sample k of pixel (c, r) at (r*width + c)*8 + k; empty: NB_EYES_NONE and 1.0f
 *   rgba, bgra8    the resolved frame, shaped as nb_frame's
 * Any output may be NULL, one at least.  flags must be 0.  1 <= width, height <= NB_FRAME_MSAA_MAX_DIM: at most 256 MiB of keys and
 * 128 MiB per sample output.  The device rows and the key plane are the context's, grown on demand as nb_frame's.  Bit-exact, and
 * the same bits from run to run. */
#define NB_FRAME_MSAA_MAX_DIM 2048u
int nb_frame_sample_offsets(float *out16);   /* ox[0..7] then oy[0..7]; host arithmetic, no device */
int nb_frame_msaa(nb_ctx *ctx, const float *cam16, uint32_t width, uint32_t height, uint32_t flags, uint32_t *ids8, float *depth8,
                  float *rgba, uint32_t *bgra8);

/* Device -> host, after waiting for queued steps.  Any of the three may be NULL.
 * inst_16n, when given, receives the model matrices of the current state (src/main.rs:437-439),
 * produced on demand by a separate kernel: they never feed back into the dynamics. */
int nb_download(nb_ctx *ctx, float *pos_xyz, float *vel_xyz, float *inst_16n);

/* Block until all queued work of ctx has finished. */
int nb_sync(nb_ctx *ctx);

/* Steps taken since nb_upload. */
uint64_t nb_steps_done(const nb_ctx *ctx);

/* -- one-call drop-ins: the reference's free functions themselves ------------------------------------- *
 * `update_instance_nbody(instances, positions, old_positions, velocities, old_velocities)` (src/main.rs:404-410) and
 * `update_instance_boids` (src/main.rs:443-449) with their own five slices, updated in place; every length is the
 * slice's len() in elements (bodies).  A maintainer replaces each function body by one call.
 * Kept from the reference:
 *   - old_positions / old_velocities receive copies of positions / velocities first (main.rs:415-416, 459-460);
 *     unequal lengths are NB_ERR_INVALID, where copy_from_slice panics;
 *   - instances.zip(positions).zip(velocities) stops at the shortest (main.rs:420-423, 465-469): only that many
 *     bodies are written, while the folds still run over all of old_positions;
 *   - boids folds rule 1 and rule 2 over old_positions.iter() (main.rs:471, 482) and rule 3 over old_velocities.iter()
 *     (main.rs:494): each fold has its own slice's length, nothing is indexed by the other's, so positions and
 *     velocities of different lengths are served as the reference serves them (the zip bounds which bodies move).
 * One upload, one step, one download per call.  The device contexts live inside the library between calls: up to three,
 * keyed by controller, body count and constants (a host may alternate controllers or entity counts from frame to frame; only
 * a fourth shape rebuilds one); calls are serialised by an internal lock.
 * The call returns when the results are in the caller's arrays.  Up to 2 048 bodies (the reference's ceiling, main.rs:653) the
 * calling thread SPINS on a word the last kernel writes behind the results (4 us sooner than a stream wait; at most 2 ms, then it
 * falls back to the stream wait); larger sets block in hipStreamSynchronize.
 * params == NULL -> the reference constants. */
int nb_update_instance_nbody(float *instances_16n, size_t n_instances, float *positions_xyz, size_t n_positions,
                             float *old_positions_xyz, size_t n_old_positions, float *velocities_xyz, size_t n_velocities,
                             float *old_velocities_xyz, size_t n_old_velocities, const nb_params *params);
int nb_update_instance_boids(float *instances_16n, size_t n_instances, float *positions_xyz, size_t n_positions,
                             float *old_positions_xyz, size_t n_old_positions, float *velocities_xyz, size_t n_velocities,
                             float *old_velocities_xyz, size_t n_old_velocities, const nb_boids_params *params);
/* update_instance_random(instances, positions, velocities) (src/main.rs:381-385) as one call: the reference's three slices,
 * the first min(n_instances, n_positions, n_velocities) bodies move (its zip, :386-389), the rest are not touched.  The
 * reference draws from an unseeded thread_rng; here body n at the library's k-th call draws from the counter-based stream
 * (seed, k, n) of nb_step_random, with the seed and the call counter kept inside the library (nb_update_random_seed sets the
 * seed and restarts the counter; the default seed is fixed, so a run is reproducible): the distribution is the reference's,
 * the draws are not.  nb_update_instance_random_seeded is the same step with the stream position given by the caller
 * (independent of how a run is split across calls or hosts). */
int nb_update_instance_random(float *instances_16n, size_t n_instances, float *positions_xyz, size_t n_positions,
                              float *velocities_xyz, size_t n_velocities);
int nb_update_instance_random_seeded(float *instances_16n, size_t n_instances, float *positions_xyz, size_t n_positions,
                                     float *velocities_xyz, size_t n_velocities, uint64_t seed, uint64_t step);
void nb_update_random_seed(uint64_t seed);

/* Frees the contexts the calls above keep (otherwise they are reclaimed with the process). */
void nb_update_release(void);

/* -- launch API: caller-owned device memory ------------------------------------------------------------ *
 * For hosts that own the device buffers and the exchange step themselves (one process per GPU, RCCL
 * all-gather of positions between steps).  Device layout: one 16-byte record per body,
 * float4 (x, y, z, 0) for positions and (vx, vy, vz, 0) for velocities.
 * `stream` is a hipStream_t (NULL = the default stream).  All launches are asynchronous.                 */

/* Bytes of device scratch nb_launch_step needs for this shape (may be 0): the scalar-load kernels keep x / y / z planes of the
 * position set there (12 B per body of the WHOLE set), FAST its rows of partial sums as well (a whole set in the pairs form:
 * n_total x n_total / 2048 x 12 B -- 100 MB at 131 072 bodies).  Always ask; the number changes with shape and mode. */
size_t nb_scratch_bytes(const nb_params *params, uint32_t n_total, uint32_t count);

/* One step for bodies [first, first+count) of a set of n_total:
 *   pos_in   n_total records, the start-of-step snapshot (old_positions, main.rs:415), read only
 *   pos_out  n_total records; only [first, first+count) is written (the caller gathers the rest)
 *   vel      count records, this shard's velocities, updated in place (local index i - first)
 * pos_out must not alias pos_in. */
int nb_launch_step(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                   void *pos_out, void *vel, void *scratch, size_t scratch_bytes, void *stream);

/* A FAST step in two phases, so that the exchange of a multi-GPU job can overlap with compute (SURVEY.md section 8e,
 * "Overlap"): NB_PHASE_RANGE folds records [j_lo, j_hi) of pos_in only -- e.g. this rank's own slot of the snapshot, which
 * is in place before the all-gather of the other slots has landed -- into `scratch`; NB_PHASE_REST folds the rest of the
 * set, adds every partial sum in a fixed order and integrates (main.rs:434-436).  Both calls take the same arguments; the
 * order of the additions differs from a one-call step (legal in FAST only: STRICT keeps the reference's j = 0..N-1 order
 * and returns NB_ERR_UNSUPPORTED here).  scratch: nb_scratch_bytes_phased() bytes, untouched between the two calls. */
enum { NB_PHASE_RANGE = 0, NB_PHASE_REST = 1 };
size_t nb_scratch_bytes_phased(const nb_params *params, uint32_t n_total, uint32_t count, uint32_t j_lo, uint32_t j_hi);
int nb_launch_step_phase(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, uint32_t j_lo, uint32_t j_hi,
                         int phase, const void *pos_in, void *pos_out, void *vel, void *scratch, size_t scratch_bytes, void *stream);

/* FAST on shards with every UNORDERED pair evaluated once ("half shell").  The term of the pair (a, b) in a's sum is the negative
 * of its term in b's (src/main.rs:428-430), so one evaluation serves both bodies even when they live on different GPUs, provided
 * the other body's half is sent to its owner: a step then has TWO exchanges instead of one, and half the arithmetic.
 * Rank r of P = n_total / count equal ranks (first = r * count) evaluates the pairs of its bodies with the N/2 bodies that follow
 * them on the ring of indices; with D = nb_ring_partners() the ranks r+1 .. r+D (mod P) own those bodies.
 *   nb_launch_ring_fold    pos_in: n_total records (the snapshot, as for nb_launch_step).  sums: (D + 1) * count records
 *                          (x, y, z, 0), written: [0, count) = this rank's own bodies, [d * count, (d + 1) * count) = the
 *                          sums this rank evaluated for the bodies of rank (r + d) mod P.
 *   -- the host's second exchange: chunk d of `sums` goes to rank (r + d) mod P, which stores it as chunk d - 1 of its `recv`
 *      (D * count records; chunk d - 1 comes from rank (r - d) mod P), d = 1..D --
 *   nb_launch_ring_finish  adds sums[0, count) and the D received chunks in ascending distance, then src/main.rs:434-436:
 *                          pos_out[first, first + count) and vel (count records) as nb_launch_step writes them.
 * Every order of addition is fixed (run-to-run identical); FAST only (reassociated sums; STRICT shards keep nb_launch_step).
 * nb_ring_partners: D >= 1; 0 when this shape does not take the form (STRICT, unequal or partial ranks, count not a multiple of
 * 256, or fewer than 2^30 ordered pairs per rank and step -- n_total x count -- where what the form saves no longer pays for its
 * second exchange: use nb_launch_step); or a negative nb_status.  Every rank of a job gets the same answer. */
int nb_ring_partners(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count);
size_t nb_ring_scratch_bytes(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count);
int nb_launch_ring_fold(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in, void *sums,
                        void *scratch, size_t scratch_bytes, void *stream);
int nb_launch_ring_finish(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in, void *pos_out,
                          void *vel, const void *sums, const void *recv, void *stream);

/* The same step in PHASES, so that its exchanges can hide behind compute (round 5; SURVEY.md section 8e "Overlap";
 * src/main.rs:415, 425-432: every pair reads the start-of-step snapshot only).  A rank's pairs fall into those whose two bodies
 * it owns itself -- they need nothing from another GPU -- and those with the bodies of the D ranks in front:
 *   NB_RING_OWN    pairs inside the rank's own slot, as many as one round of workgroups holds (3 068 of the 4 224 own-slot
 *                  sub-tiles of an 8-rank share of 131 072 bodies: 23 us on an MI355X).  Reads ONLY records
 *                  [first, first + count) of pos_in -- which the rank's own nb_launch_ring_finish wrote -- so it may run while
 *                  the all-gather of the other slots of pos_in is still landing.
 *   NB_RING_REST   every other pair (the whole snapshot must be in place), and the sums of the halves that belong to the ranks
 *                  in front: records [count, (D + 1) count) of `sums` are final when it completes -- the second exchange can start.
 *   NB_RING_SUMS   the rank's own sums, records [0, count) of `sums`: it can run beside the second exchange.
 *   then nb_launch_ring_finish as above.
 * One step, with `x` a second stream for the exchanges:
 *     OWN | wait(all-gather of the last step) | REST | [x: second exchange] SUMS | wait(x) | finish | [x: all-gather]
 * (a host whose cross-stream waits are dear keeps the second exchange on the compute stream -- REST | SUMS | exchange | finish --
 * as nb_shard_step does: two waits cost more than the 9 us of SUMS they would hide; the all-gather's two waits hide behind OWN)
 * Same arguments in every call of a step (same scratch, untouched between them: nb_ring_scratch_bytes() covers both forms).
 * The sums are added in another (fixed) order than nb_launch_ring_fold's: run-to-run identical, FAST's tolerances, its own bits.
 * nb_ring_phased: 1 where the shape can run its step this way (nb_ring_partners() > 0 and the rank's rows fit one launch -- every
 * rank count of BASELINE's config 4; config 5's ranks walk their rows in groups and keep nb_launch_ring_fold: two exchanges of
 * 2 MB per peer against 13.6 ms of compute), 0 where it keeps nb_launch_ring_fold; or a negative nb_status. */
enum { NB_RING_OWN = 1, NB_RING_REST = 2, NB_RING_SUMS = 3, NB_RING_OWN_READY = 4 };
int nb_ring_phased(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count);
int nb_launch_ring_fold_phase(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, int phase, const void *pos_in,
                              void *sums, void *scratch, size_t scratch_bytes, void *stream);
/* The finish of a step in phases, FUSED (two launches fewer per step: every small launch of a step costs ~5 us of ramp and drain):
 *   nb_launch_ring_finish_phase  with sums == NULL adds the rank's own records ITSELF -- NB_RING_SUMS is not launched; the same
 *                                additions in the same order, the same bits -- (a host that runs NB_RING_SUMS beside its second
 *                                exchange passes `sums`: records [0, count) are read instead); then the D received chunks and
 *                                src/main.rs:434-436 as nb_launch_ring_finish; and leaves the planes and flag words of the NEW own
 *                                slot (pos_out[first, first + count)) in `scratch`.
 *   NB_RING_OWN_READY            NB_RING_OWN of the NEXT step without the launch that prepares its planes: valid when the last thing
 *                                that touched `scratch` was nb_launch_ring_finish_phase of the same shape and this call's pos_in is
 *                                that call's pos_out.  (pos_in is not read.)
 *     step k:  OWN_READY | wait(all-gather k - 1) | REST | second exchange | finish_phase | [all-gather k] ...
 * The first step of a run, and any step behind something else that used `scratch`, starts with NB_RING_OWN. */
int nb_launch_ring_finish_phase(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in, void *pos_out,
                                void *vel, const void *sums, const void *recv, void *scratch, size_t scratch_bytes, void *stream);

/* One boids step (main.rs:443-526) for bodies [first, first+count) of a set of n_total:
 *   pos_in, vel_in    n_total records each: the snapshots old_positions / old_velocities (main.rs:459-460), read only
 *   pos_out, vel_out  n_total records each; only [first, first+count) is written (a multi-GPU caller all-gathers BOTH)
 * The outputs must not alias the inputs. */
int nb_launch_boids_step(const nb_boids_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                         const void *vel_in, void *pos_out, void *vel_out, void *stream);

/* The same step with the j range cut into slices ("split" form, for shards whose bodies alone cannot fill the chip: a rank of an
 * 8-GPU job): every radius test is evaluated on the reference's operands with the reference's bits, so the neighbour SETS and
 * COUNTS are the reference's, but a body's sums are added slice by slice (in index order inside a slice, then in slice order --
 * the same order every step) instead of in one index-ordered chain: not bit-identical -- as close to the exact sums as the
 * reference's own sequential binary32 sums are (the tests hold it to that, against the same sums carried in binary64), which
 * puts it within ~1e-5 of the bit-exact step's velocities per step on tens of thousands of bodies.  Opt-in: nb_launch_boids_step stays the reference's arithmetic.  scratch: nb_boids_split_scratch_bytes(). */
size_t nb_boids_split_scratch_bytes(const nb_boids_params *params, uint32_t n_total, uint32_t count);
int nb_launch_boids_step_split(const nb_boids_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                               const void *vel_in, void *pos_out, void *vel_out, void *scratch, size_t scratch_bytes, void *stream);

/* Model matrices (main.rs:437-439) for `count` bodies: pos, vel -> inst (16 floats per body). */
int nb_launch_instances(uint32_t count, const void *pos, const void *vel, void *inst_16n, void *stream);

/* Camera matrices (gfx.rs:397-408) for `count` entities on caller-owned device memory: eyes/dirs are 16-byte records,
 * out receives 16 floats per entity. */
int nb_launch_cameras(uint32_t count, const void *eyes, const void *dirs, const float *up_xyz, const float *cp16, void *out_16n,
                      void *stream);

/* nb_eyes' rule, stateless, on caller-owned device memory: cams_16 = count cameras (eye e is body first+e), inst_16n = n_total model
 * matrices (both 16-byte aligned); ids (uint32) / depth (float): count*width each, either may be NULL (not both).  The outputs
 * must not alias each other or an input.  count = 0 is a no-op. */
int nb_launch_eyes(uint32_t n_total, uint32_t first, uint32_t count, const void *cams_16, const void *inst_16n, uint32_t width,
                   uint32_t flags, void *ids, void *depth, void *stream);

/* The seen sets of `count` rows of `width` columns (nb_eyes_seen's rule), stateless, on caller-owned device memory: ids_rows (uint32) /
 * depth_rows (float): count*width each, as nb_launch_eyes leaves them or the caller's own; seen_count: count words; seen_ids, seen_depth,
 * seen_cols: count*width each.  depth_rows, seen_depth and seen_cols may be NULL; seen_depth needs depth_rows.  Everything 4-byte
 * aligned; no output may overlap another output or an input.  1 <= width <= NB_EYES_MAX_WIDTH.  count = 0 is a no-op.  One kernel
 * on `stream`. */
int nb_launch_seen(uint32_t count, uint32_t width, const void *ids_rows, const void *depth_rows, void *seen_count, void *seen_ids,
                   void *seen_depth, void *seen_cols, void *stream);

/* One boids step over seen lists (nb_step_boids_seen's V2-V3) for bodies [first, first+count) of a set of n_total: body first+e folds
 * over the first seen_count[e] entries (at most `stride`) of seen_ids[e*stride ..] in list order.  An entry equal to the body's own
 * index is skipped (the `n != i` test); an entry >= n_total is skipped without being read; a duplicate folds twice.  Buffers as
 * nb_launch_boids_step's; the lists 4-byte aligned, stride >= 1; the outputs must not alias the inputs or the lists. */
int nb_launch_boids_seen_step(const nb_boids_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                              const void *vel_in, const void *seen_count, const void *seen_ids, uint32_t stride, void *pos_out,
                              void *vel_out, void *stream);

/* The located seen sets of `count` rows of `width` columns (nb_eyes_located's rule L1-L6), stateless, on caller-owned device memory:
 * ids_rows (uint32) / depth_rows (float): count*width each, as nb_launch_eyes leaves them; seen_count, seen_ids, seen_depth: as
 * nb_launch_seen leaves them for those rows (ascending, no duplicates; a count above width is taken as width); eyes / dirs: count
 * 16-byte records as nb_launch_cameras takes them (the rule reads dirs alone: the estimate is relative to the eye); up_xyz / cp16:
 * host pointers; seen_col (uint32, may be NULL): count*width; seen_rel: count*width records of 4 floats.  The rows, the lists and
 * seen_col 4-byte aligned, eyes, dirs and seen_rel 16-byte aligned; no output may overlap the other output or an input.
 * 1 <= width <= NB_EYES_MAX_WIDTH.  count = 0 is a no-op.  One kernel on `stream`.  (A stateless launch entry like the nb_launch_* ones;
 * `launch` stands behind its name and that of the fold below.) */
int nb_seen_located_launch(uint32_t count, uint32_t width, const void *ids_rows, const void *depth_rows, const void *seen_count,
                           const void *seen_ids, const void *seen_depth, const void *eyes, const void *dirs, const float *up_xyz,
                           const float *cp16, void *seen_col, void *seen_rel, void *stream);

/* One gravity step over located lists (nb_step_nbody_located's G2-G3) for bodies [first, first+count) of a set of n_total: body
 * first+e folds over the first seen_count[e] records (at most `stride`) of seen_rel[(e*stride + k)*4 ..] in slot order; what lies
 * behind is never read.  pos_in, vel_in, pos_out, vel_out: n_total records each, only [first, first+count) is read and written;
 * params == NULL -> defaults (dt, G and bias are used).  seen_count 4-byte aligned, the records and seen_rel 16-byte aligned,
 * stride >= 1; the outputs must not alias the inputs or the lists. */
int nb_nbody_located_step_launch(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                                 const void *vel_in, const void *seen_count, const void *seen_rel, uint32_t stride, void *pos_out,
                                 void *vel_out, void *stream);

/* nb_eyes_colour's rule, stateless, on caller-owned device memory: as nb_launch_eyes, plus skin = tw x th linear RGBA texels (row 0
 * first, 16-byte aligned, 1 <= tw, th <= NB_EYES_MAX_SKIN), or NULL for the 1 x 1 white skin (tw, th ignored); rgba: count*width*4
 * floats, 16-byte aligned; bgra8: count*width words.  Any of the four outputs may be NULL, but not both rgba and bgra8.  No two
 * outputs may overlap, and none may overlap cams_16, inst_16n or skin.  count = 0 is a no-op. */
int nb_launch_eyes_colour(uint32_t n_total, uint32_t first, uint32_t count, const void *cams_16, const void *inst_16n, uint32_t width,
                          uint32_t flags, const void *skin, uint32_t tw, uint32_t th, void *ids, void *depth, void *rgba, void *bgra8,
                          void *stream);

/* nb_eyes_msaa's rule, stateless, on caller-owned device memory: inputs as nb_launch_eyes_colour's (cams_16, inst_16n and skin 16-byte
 * aligned); ids8 (uint32) / depth8 (float): count*width*8 words each; rgba: count*width*4 floats, 16-byte aligned; bgra8: count*width
 * words.  Any output may be NULL, one at least.  No two outputs may overlap, and none may overlap cams_16, inst_16n or skin.
 * 1 <= width <= NB_EYES_MSAA_MAX_WIDTH.  count = 0 is a no-op.  One kernel on `stream`. */
int nb_launch_eyes_msaa(uint32_t n_total, uint32_t first, uint32_t count, const void *cams_16, const void *inst_16n, uint32_t width,
                        uint32_t flags, const void *skin, uint32_t tw, uint32_t th, void *ids8, void *depth8, void *rgba, void *bgra8,
                        void *stream);

/* nb_frame's rule, stateless, on caller-owned device memory: cam_16 = one camera, inst_16n = n_total model matrices, skin as
 * nb_launch_eyes_colour's (16-byte aligned, all three); scratch = nb_frame_scratch_bytes(width, height) bytes, 8-byte aligned,
 * rewritten by every call; ids / depth / bgra8: height*width words each, rgba: height*width*4 floats, 16-byte aligned.  Any output
 * may be NULL, one at least.  No output may overlap another output, an input or the scratch.  n_total = 0 (inst_16n may then be
 * NULL) gives a frame of clear pixels.  Three kernels on `stream`. */
size_t nb_frame_scratch_bytes(uint32_t width, uint32_t height);   /* width * height * 8; 0 for an invalid extent */
int nb_launch_frame(uint32_t n_total, const void *cam_16, const void *inst_16n, uint32_t width, uint32_t height, uint32_t flags,
                    const void *skin, uint32_t tw, uint32_t th, void *scratch, void *ids, void *depth, void *rgba, void *bgra8,
                    void *stream);

/* nb_frame_msaa's rule, stateless, on caller-owned device memory: inputs as nb_launch_frame's; scratch =
 * nb_frame_msaa_scratch_bytes(width, height) bytes, 8-byte aligned, rewritten by every call; ids8 (uint32) / depth8 (float):
 * height*width*8 words each; rgba: height*width*4 floats, 16-byte aligned; bgra8: height*width words.  Any output may be NULL, one
 * at least.  No output may overlap another output, an input or the scratch.  n_total = 0 (inst_16n may then be NULL) gives a clear
 * frame with every sample empty.  Three kernels on `stream`. */
size_t nb_frame_msaa_scratch_bytes(uint32_t width, uint32_t height);   /* width * height * 64; 0 for an invalid extent */
int nb_launch_frame_msaa(uint32_t n_total, const void *cam_16, const void *inst_16n, uint32_t width, uint32_t height, uint32_t flags,
                         const void *skin, uint32_t tw, uint32_t th, void *scratch, void *ids8, void *depth8, void *rgba, void *bgra8,
                         void *stream);

/* One random-walk step (main.rs:381-402) in place for `count` bodies whose global indices start at `first`. */
int nb_launch_random_step(uint32_t first, uint32_t count, void *pos, void *vel, uint64_t seed, uint64_t step, void *stream);

/* Waits for `stream` and reports a failure a launch-API kernel recorded on the current device since the last call:
 * NB_ERR_STATE when a STRICT block-chain workgroup gave up waiting for its turn (its outputs were written as NaN), NB_OK
 * otherwise.  The context and shard objects make the same check themselves in nb_sync / nb_download / nb_shard_sync /
 * nb_shard_download; a host that drives nb_launch_step directly calls this wherever it waits for the device. */
int nb_launch_status(void *stream);

/* Stride-3 <-> 16-byte record conversion on the device. */
int nb_launch_pack(uint32_t count, const void *xyz, void *rec4, void *stream);
int nb_launch_unpack(uint32_t count, const void *rec4, void *xyz, void *stream);

/* -- the exchanges of a multi-GPU step as PULLS over xGMI (round 5) ---------------------------------------- *
 * No collective library, no second stream, no kernel that polls: every rank registers a few device buffers (the two position
 * replicas, the pairs form's `sums`) and hands the others a blob of IPC memory handles (nb_peers_export; the host moves the blobs:
 * MPI, torch.distributed, a file); after nb_peers_import every rank holds mappings of every other rank's buffers and of a block of
 * flag words.  An exchange is then, on the rank's OWN stream:
 *     nb_peers_signal   hipStreamWriteValue32(my flag[channel] = next count): "what I launched so far is complete"
 *     ... whatever needs no other rank (the pairs inside the rank's own slot: nb_launch_ring_fold_phase(NB_RING_OWN)) ...
 *     nb_peers_gather   hipStreamWaitValue32(peer's flag[channel] >= count) for every peer, then ONE kernel copies slot q of peer q's
 *                       buffer into slot q of this rank's (16-byte loads over xGMI)
 *     nb_peers_ring     the same for the pairs form's second exchange: chunk d of rank (r - d)'s buffer -> chunk d - 1 of `recv`
 * Nobody writes another rank's memory, and a kernel reads a peer's memory only behind that peer's signal.  Buffers may be pieces of
 * larger allocations (a caching allocator's).  Up to 16 ranks (one xGMI domain), all in processes of one node.  Ranks call the
 * same sequence of signals and exchanges per channel (SPMD).  That a buffer is not rewritten while a peer still pulls from it is the
 * CALLER's ordering: alternate the two position replicas (as every host here does) and rewrite `sums` only behind a gather.
 * nb_shard_use_peers / ShardedScene(exchange="peers") wire this into a step.  Measured between two processes on one GPU: a signal +
 * wait + 256 KB pull round trip in ~10 us (profiles/r05/ubench_ipc.log); between GPUs: not run in this build -- verify_exchanges
 * checks a pattern through it before the first step, and falls back. */
#define NB_PEERS_MAX_BUFFERS 4
#define NB_PEERS_CHANNELS 4
typedef struct nb_peers nb_peers;
size_t nb_peers_blob_bytes(void);
int nb_peers_create(int rank, int world, nb_peers **out);
void nb_peers_destroy(nb_peers *p);   /* (after a probe that had to abandon its stream: releases nothing -- every release would wait for that stream) */
const char *nb_peers_last_error(const nb_peers *p);
int nb_peers_export(nb_peers *p, void *const *bufs, const size_t *bytes, int nbufs, void *blob);
int nb_peers_import(nb_peers *p, const void *blobs /* world x nb_peers_blob_bytes(), rank-major */);
/* First contact with a deadline (collective), in two stages: this rank signals and the HOST reads every peer's word through the mapping
 * until it shows the signal or timeout_ms has passed (nothing can block); only then a wait / one-record pull round on a stream of its
 * own, watched for the same time (a wait the command processor cannot satisfy is released by hand).  NB_ERR_STATE: keep the collectives.
 * Hosts call it once after nb_peers_import (ShardedScene.setup_peers and nb_shard_peer_import do). */
int nb_peers_probe(nb_peers *p, uint32_t timeout_ms);
int nb_peers_signal(nb_peers *p, int channel, void *stream);
int nb_peers_gather(nb_peers *p, int channel, int buf, size_t slot_bytes, void *stream);
int nb_peers_ring(nb_peers *p, int channel, int buf, void *recv, size_t chunk_bytes, int partners, void *stream);

/* -- sharded scene: one process (or thread) per GPU ------------------------------------------------------ *
 * The host side of the multi-GPU path in the library itself, for hosts that do not bring torch: rank r of `world`
 * owns bodies [r*slot, r*slot + count) with slot = ceil(n / world) (trailing ranks may be short or empty) and a replica
 * of all positions; one step is the local update followed by ONE exchange in which every rank contributes its slot of
 * the new positions and receives the others' (`old_positions` of src/main.rs:415 is the replica).
 * The boids controller exchanges velocities the same way (it reads every old velocity, src/main.rs:494-504).
 * STRICT results do not depend on `world`.  The exchange is either RCCL (ncclAllGather in place, loaded with dlopen:
 * NENBODY_RCCL, else the librccl.so.1 already in the process, else the system's) or a function the host supplies. */
typedef struct nb_shard nb_shard;

/* The exchange: `buf` is device memory of world*slot_bytes; this rank's slot (offset rank*slot_bytes) is ready on
 * `stream` (a hipStream_t); on return (or: ordered on `stream`) every other slot must hold that rank's contribution.
 * Return 0, or nonzero to fail the step with NB_ERR_STATE. */
typedef int (*nb_gather_fn)(void *user, void *buf, size_t slot_bytes, int rank, int world, void *stream);

#define NB_COMM_ID_BYTES 128
/* A fresh RCCL unique id (ncclGetUniqueId): call on one rank, hand the NB_COMM_ID_BYTES to the others by any channel. */
int nb_comm_id(void *id);

/* Rank `rank` of `world` for n bodies on the current HIP device.  params == NULL -> defaults. */
int nb_shard_create(uint32_t n, int rank, int world, const nb_params *params, nb_shard **out);
void nb_shard_destroy(nb_shard *sh);
/* Choose the exchange (required before stepping when world > 1).  nb_shard_use_rccl is collective over the ranks
 * (ncclCommInitRank with the id from nb_comm_id). */
int nb_shard_use_rccl(nb_shard *sh, const void *id);
int nb_shard_use_gather(nb_shard *sh, nb_gather_fn fn, void *user);
/* FAST with equal ranks of whole blocks takes the pairs form on shards (nb_launch_ring_fold above: every unordered pair once, a
 * second exchange per step) where the second exchange exists: with RCCL it is a group of ncclSend / ncclRecv; a host that brings
 * its own all-gather (nb_shard_use_gather) brings this one too, or keeps the ordered fold.  `send`: `partners` chunks of
 * chunk_bytes, chunk d - 1 for rank (rank + d) % world; `recv`: chunk d - 1 from rank (rank - d) % world; both device memory,
 * `send` ready on `stream`, `recv` must be complete or ordered on `stream` on return.  nb_shard_set_pairs(sh, 0) keeps the
 * ordered fold whatever the shape; nb_shard_pairs_partners: the D a step will use (0: the ordered fold). */
/* Both exchanges as PULLS over xGMI (nb_peers_* above; round 5): nb_shard_peer_export fills this rank's blob of nb_peers_blob_bytes()
 * bytes, the host hands every rank ALL blobs, rank-major (any channel), nb_shard_peer_import maps the others' position replicas and
 * `sums`.  From then on the all-gather and the pairs form's second exchange are a signal, stream waits on the peers' flag words and
 * one copy kernel, all on the shard's own stream; with nb_shard_set_overlap the signal goes out behind the finish kernel and the waits
 * come behind the next step's own-slot pairs -- no second stream, no idle gap.  No RCCL communicator is needed (one may exist beside it:
 * the boids controller, which moves another buffer, uses the exchange chosen before).  All ranks in processes of ONE node, at most 16.
 * nb_shard_use_peers(sh, 0 / 1) switches between this and the exchange chosen before.  Collective in effect: every rank imports
 * before any rank steps.  nb_shard_verify_exchanges checks it on a pattern like any other exchange. */
int nb_shard_peer_export(nb_shard *sh, void *blob);
int nb_shard_peer_import(nb_shard *sh, const void *blobs);
int nb_shard_use_peers(nb_shard *sh, int on);
typedef int (*nb_ring_fn)(void *user, const void *send, void *recv, size_t chunk_bytes, int partners, int rank, int world, void *stream);
int nb_shard_use_ring(nb_shard *sh, nb_ring_fn fn, void *user);
int nb_shard_set_pairs(nb_shard *sh, int on);
int nb_shard_pairs_partners(const nb_shard *sh);
/* on != 0: nb_shard_step_boids takes the split form of the boids step (nb_launch_boids_step_split: the reference's neighbour sets
 * and counts, sums reassociated) -- what lets eight ranks run the controller about eight times as fast as one instead of 3.4
 * times; off (the default): bit-identical to the reference whatever the world size. */
int nb_shard_set_boids_split(nb_shard *sh, int on);
/* FAST only ("Overlap"): with `on` != 0 the exchanges of a step run on a second stream, behind compute that
 * does not need them.  A shard in the ordered fold folds its own slot of the snapshot while the all-gather of the other slots is
 * still in flight, waits for it, then folds the rest (the two phases of nb_launch_step_phase).  A shard in the pairs form
 * (nb_shard_pairs_partners() > 0, nb_ring_phased()) runs the phases of nb_launch_ring_fold_phase: pairs inside its own slot while
 * the all-gather lands on the second stream, every other pair, the sums, the second exchange (on the shard's own stream), finish
 * (round 5).  The order of the
 * additions changes, which FAST may and STRICT may not: a STRICT shard (and a world of one) ignores the request and stays
 * kernel -> exchange in sequence.  Host-supplied exchanges (nb_shard_use_gather / nb_shard_use_ring) receive the second stream
 * and must order their work on it. */
int nb_shard_set_overlap(nb_shard *sh, int on);
/* Both exchanges of a step, ONCE, on a known per-rank pattern, checked on every rank (collective; the ranks agree on every verdict
 * through a third collective: ncclAllReduce, or the host's gather).  A mismatch moves the exchange to its fallback without restarting
 * anything: the all-gather from a copy of the slot (*gather_path 1; 0: in place), the second exchange as one group per distance
 * (*ring_path 1; 0: one group), then not at all (*ring_path 2: the ordered fold and its one exchange); *ring_path -1: no pairs form
 * planned.  A shard that pulls its exchanges over xGMI (nb_shard_peer_import) is checked as such first (*gather_path 2, *ring_path 3)
 * -- TWICE from the same buffers with different patterns: a reader served from lines it cached at the first pull shows the first pattern
 * again -- and goes back to the exchange chosen before on a mismatch.  Either pointer may be NULL.  A world of one answers at once.  With RCCL on more than one rank the first nb_shard_step runs
 * this by itself if the host has not. */
int nb_shard_verify_exchanges(nb_shard *sh, int *gather_path, int *ring_path);
/* Which form should a FAST step take on THIS machine?  Times `steps` steps (0: four) of every form the shard can take -- 1: the pairs
 * form with its two exchanges in sequence, 2: the same in phases with the exchanges behind compute (nb_shard_set_overlap), 0: the
 * ordered fold with its one exchange -- on the state in hand, takes the slowest rank's time of each (collective), keeps the fastest
 * for the steps to come (*chosen) and puts the state back; ms3 (NULL or three doubles): milliseconds per step of forms 0, 1, 2
 * (negative: not offered).  The library's own line for the pairs form (nb_ring_partners) was drawn from one-GPU timings; this asks
 * the machine.  With RCCL on more than one rank the first nb_shard_step asks by itself unless the host has decided
 * (nb_shard_set_pairs) or asked (this call).  Note: which form runs decides the rounding of FAST's sums -- a host that needs
 * run-to-run identical bits names the form. */
int nb_shard_choose_form(nb_shard *sh, uint32_t steps, int *chosen, double *ms3);
/* 1 where a step of this shard takes the pairs form in phases with both exchanges on the second stream, else 0. */
int nb_shard_pairs_overlapped(const nb_shard *sh);
/* This rank's index range. */
int nb_shard_range(const nb_shard *sh, uint32_t *first, uint32_t *count);
/* Host -> device: ALL n positions and ALL n velocities (identical on every rank; the rank keeps its own velocities). */
int nb_shard_upload(nb_shard *sh, const float *pos_xyz, const float *vel_xyz);
/* k steps of update_instance_nbody / update_instance_boids, asynchronous; collective over the ranks. */
int nb_shard_step(nb_shard *sh, uint32_t k);
int nb_shard_step_boids(nb_shard *sh, uint32_t k, const nb_boids_params *params);
/* Device -> host: all n positions (the replica), this rank's `count` velocities and model matrices.  Any may be NULL. */
int nb_shard_download(nb_shard *sh, float *pos_xyz, float *vel_xyz_local, float *inst_16n_local);
int nb_shard_sync(nb_shard *sh);
/* Message of the last failure on `sh` (never NULL); creation failures are reported through nb_last_error(NULL). */
const char *nb_shard_last_error(const nb_shard *sh);

#ifdef __cplusplus
}
#endif
#endif /* NENBODY_H */
