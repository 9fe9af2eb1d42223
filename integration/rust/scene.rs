//! src/scene.rs -- fills the reference's empty module (reference src/scene.rs:1, `mod scene;` at src/main.rs:2).
//!
//! A `Scene` owns the simulation state the reference keeps as locals of `main()` (src/main.rs:738-750) and
//! advances it with libnenbody_hip.so (include/nenbody.h).  `Scene::step()` is `update_instance_nbody`
//! (src/main.rs:404-441) on the GPU; afterwards `positions`, `velocities` and `instances` hold what the
//! per-frame consumers read (src/main.rs:932-945).
//!
//! NOT COMPILED in the build environment (no cargo/rustc there): a mechanical binding of the C ABI.
use cgmath::{Point3, Vector3};
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct NbParams {
    pub dt: f32,   // src/main.rs:411
    pub g: f32,    // src/main.rs:412
    pub bias: f32, // src/main.rs:413
    pub tile: u32, // 0 = library default
    pub mode: u32, // 0 = STRICT (bit-identical to the CPU path), 1 = FAST
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct NbBoidsParams {
    pub dt: f32,              // src/main.rs:450
    pub rule_1_distance: f32, // src/main.rs:451 (squared-distance radius)
    pub rule_2_distance: f32, // src/main.rs:452
    pub rule_3_distance: f32, // src/main.rs:453 (velocity space)
    pub rule_1_scale: f32,    // src/main.rs:454
    pub rule_2_scale: f32,    // src/main.rs:455
    pub rule_3_scale: f32,    // src/main.rs:456
    pub tile: u32,
}

#[repr(C)]
pub struct NbCtx {
    _private: [u8; 0],
}

/// The ABI this binding was written against (include/nenbody.h: NB_ABI_VERSION).  A symbol may keep its name and change its
/// arguments between versions (`nb_update_instance_random`: eight in ABI 1, six since ABI 2) and the linker cannot tell, so
/// every entry point of this module checks it once per process before anything else crosses the boundary.
pub const NB_ABI_VERSION: c_int = 2;

#[link(name = "nenbody_hip")]
extern "C" {
    fn nb_abi_version() -> c_int;
    fn nb_default_params(p: *mut NbParams);
    fn nb_last_error(ctx: *const NbCtx) -> *const c_char;
    fn nb_init_state(seed: u64, n: u32, pos_xyz: *mut f32, vel_xyz: *mut f32) -> c_int;
    fn nb_create(n: u32, n_devices: u32, params: *const NbParams, out: *mut *mut NbCtx) -> c_int;
    fn nb_destroy(ctx: *mut NbCtx);
    fn nb_upload(ctx: *mut NbCtx, pos_xyz: *const f32, vel_xyz: *const f32) -> c_int;
    fn nb_step(ctx: *mut NbCtx, k: u32) -> c_int;
    fn nb_step_boids(ctx: *mut NbCtx, k: u32, params: *const NbBoidsParams) -> c_int; // null = reference constants
    fn nb_download(ctx: *mut NbCtx, pos_xyz: *mut f32, vel_xyz: *mut f32, inst_16n: *mut f32) -> c_int;
    fn nb_sync(ctx: *mut NbCtx) -> c_int;
    // the reference's free functions themselves: five slices and their lengths, params null = reference constants
    fn nb_update_instance_nbody(
        instances: *mut f32, n_instances: usize, positions: *mut f32, n_positions: usize,
        old_positions: *mut f32, n_old_positions: usize, velocities: *mut f32, n_velocities: usize,
        old_velocities: *mut f32, n_old_velocities: usize, params: *const NbParams,
    ) -> c_int;
    fn nb_update_instance_boids(
        instances: *mut f32, n_instances: usize, positions: *mut f32, n_positions: usize,
        old_positions: *mut f32, n_old_positions: usize, velocities: *mut f32, n_velocities: usize,
        old_velocities: *mut f32, n_old_velocities: usize, params: *const NbBoidsParams,
    ) -> c_int;
    fn nb_update_instance_random(
        instances: *mut f32, n_instances: usize, positions: *mut f32, n_positions: usize,
        velocities: *mut f32, n_velocities: usize,
    ) -> c_int;
    fn nb_update_instance_random_seeded(
        instances: *mut f32, n_instances: usize, positions: *mut f32, n_positions: usize,
        velocities: *mut f32, n_velocities: usize, seed: u64, step: u64,
    ) -> c_int;
    fn nb_update_random_seed(seed: u64);
    // every entity's eye view (the reference's eye pass, src/main.rs:585-647, 962-998) and its colour row
    fn nb_camera_constant(vertical_fov_deg: f32, aspect_ratio: f32, near_plane: f32, far_plane: f32, cp16: *mut f32) -> c_int;
    fn nb_eyes(ctx: *mut NbCtx, first: u32, count: u32, up_xyz: *const f32, cp16: *const f32, width: u32, flags: u32, ids: *mut u32, depth: *mut f32) -> c_int;
    fn nb_eyes_skin(ctx: *mut NbCtx, rgba_linear: *const f32, tw: u32, th: u32) -> c_int; // null = the 1 x 1 white skin
    fn nb_eyes_colour(ctx: *mut NbCtx, first: u32, count: u32, up_xyz: *const f32, cp16: *const f32, width: u32, flags: u32, ids: *mut u32, depth: *mut f32, rgba: *mut f32, bgra8: *mut u32) -> c_int;
    fn nb_eyes_sample_offsets(out8: *mut f32) -> c_int;
    fn nb_eyes_msaa(ctx: *mut NbCtx, first: u32, count: u32, up_xyz: *const f32, cp16: *const f32, width: u32, flags: u32, ids8: *mut u32, depth8: *mut f32, rgba: *mut f32, bgra8: *mut u32) -> c_int;
    // what a controller makes of the eye rows: the seen set of every eye, and the boids step over it (null params = reference constants)
    fn nb_eyes_seen(ctx: *mut NbCtx, first: u32, count: u32, up_xyz: *const f32, cp16: *const f32, width: u32, flags: u32, seen_count: *mut u32, seen_ids: *mut u32, seen_depth: *mut f32, seen_cols: *mut u32) -> c_int;
    fn nb_step_boids_seen(ctx: *mut NbCtx, k: u32, params: *const NbBoidsParams, up_xyz: *const f32, cp16: *const f32, width: u32, batch: u32) -> c_int;
    // where each eye sees the members of its seen set, and the gravity step over those relative positions alone (the context's nb_params)
    fn nb_eyes_located(ctx: *mut NbCtx, first: u32, count: u32, up_xyz: *const f32, cp16: *const f32, width: u32, flags: u32, seen_count: *mut u32, seen_ids: *mut u32, seen_depth: *mut f32, seen_cols: *mut u32, seen_col: *mut u32, seen_rel: *mut f32) -> c_int;
    fn nb_step_nbody_located(ctx: *mut NbCtx, k: u32, up_xyz: *const f32, cp16: *const f32, width: u32, batch: u32) -> c_int;
    fn nb_srgb_decode_table(out256: *mut f32) -> c_int;
    fn nb_srgb_encode(linear: *const f32, n: usize, out: *mut u8) -> c_int;
    // the scene camera's frame (the reference's display pass, src/main.rs:948-960)
    fn nb_camera_at(ctx: *mut NbCtx, eye_xyz: *const f32, dir_xyz: *const f32, up_xyz: *const f32, cp16: *const f32, out16: *mut f32) -> c_int;
    fn nb_frame(ctx: *mut NbCtx, cam16: *const f32, width: u32, height: u32, flags: u32, ids: *mut u32, depth: *mut f32, rgba: *mut f32, bgra8: *mut u32) -> c_int;
    fn nb_frame_scratch_bytes(width: u32, height: u32) -> usize;
    // the same through 8 samples per pixel, resolved (msaa_samples = 8, src/main.rs:652, 685-690, 545-548)
    fn nb_frame_sample_offsets(out16: *mut f32) -> c_int;
    fn nb_frame_msaa(ctx: *mut NbCtx, cam16: *const f32, width: u32, height: u32, flags: u32, ids8: *mut u32, depth8: *mut f32, rgba: *mut f32, bgra8: *mut u32) -> c_int;
    fn nb_frame_msaa_scratch_bytes(width: u32, height: u32) -> usize;
    // scene batches (include/nenbody.h, "scene batches"): B scenes of n <= NB_SCENES_MAX_BODIES bodies, k steps per launch
    fn nb_scenes_create(scenes: u32, n: u32, params: *const NbParams, out: *mut *mut NbScenes) -> c_int;
    fn nb_scenes_destroy(ctx: *mut NbScenes);
    fn nb_scenes_upload(ctx: *mut NbScenes, pos_xyz: *const f32, vel_xyz: *const f32) -> c_int;
    fn nb_scenes_step(ctx: *mut NbScenes, k: u32) -> c_int;
    fn nb_scenes_step_boids(ctx: *mut NbScenes, k: u32, params: *const NbBoidsParams) -> c_int; // null = reference constants
    fn nb_scenes_download(ctx: *mut NbScenes, pos_xyz: *mut f32, vel_xyz: *mut f32, inst_16: *mut f32) -> c_int;
    fn nb_scenes_device_state(ctx: *mut NbScenes, pos_rec: *mut *const c_void, vel_rec: *mut *const c_void, inst_16: *mut *const c_void) -> c_int;
    fn nb_scenes_sync(ctx: *mut NbScenes) -> c_int;
    fn nb_scenes_steps(ctx: *const NbScenes) -> u64;
    fn nb_scenes_last_error(ctx: *const NbScenes) -> *const c_char;
    // the boids step over what each body sees of its own scene, one fused launch per step, and the seen sets it folds over
    fn nb_scenes_step_boids_seen(ctx: *mut NbScenes, k: u32, params: *const NbBoidsParams, up_xyz: *const f32, cp16: *const f32, width: u32) -> c_int;
    fn nb_scenes_eyes_seen(ctx: *mut NbScenes, first_scene: u32, scene_count: u32, up_xyz: *const f32, cp16: *const f32, width: u32, seen_count: *mut u32, seen_ids: *mut u32) -> c_int;
    fn nb_scenes_boids_seen_step_launch(params: *const NbBoidsParams, scenes: u32, n: u32, cams_16: *const c_void, inst_16: *const c_void, width: u32, pos_in: *const c_void, vel_in: *const c_void, pos_out: *mut c_void, vel_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn nb_scenes_seen_launch(scenes: u32, n: u32, first_eye: u32, count: u32, cams_16: *const c_void, inst_16: *const c_void, width: u32, seen_count: *mut c_void, seen_ids: *mut c_void, stream: *mut c_void) -> c_int;
    // gravity from located vision of every scene, one fused launch per step, and the located sets it folds over
    fn nb_scenes_step_nbody_located(ctx: *mut NbScenes, k: u32, up_xyz: *const f32, cp16: *const f32, width: u32) -> c_int;
    fn nb_scenes_eyes_located(ctx: *mut NbScenes, first_scene: u32, scene_count: u32, up_xyz: *const f32, cp16: *const f32, width: u32, seen_count: *mut u32, seen_ids: *mut u32, seen_depth: *mut f32, seen_col: *mut u32, seen_rel: *mut f32) -> c_int;
    fn nb_scenes_nbody_located_step_launch(params: *const NbParams, scenes: u32, n: u32, cams_16: *const c_void, inst_16: *const c_void, up_xyz: *const f32, cp16: *const f32, width: u32, pos_in: *const c_void, vel_in: *const c_void, pos_out: *mut c_void, vel_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn nb_scenes_located_launch(scenes: u32, n: u32, first_eye: u32, count: u32, cams_16: *const c_void, inst_16: *const c_void, vel_in: *const c_void, up_xyz: *const f32, cp16: *const f32, width: u32, seen_count: *mut c_void, seen_ids: *mut c_void, seen_depth: *mut c_void, seen_col: *mut c_void, seen_rel: *mut c_void, stream: *mut c_void) -> c_int;
    // a neural policy over each body's eye row (include/nenbody_scenes_policy.h), one fused launch per step, and what it computes per eye
    fn nb_policy_floats(features: u32, hidden: u32) -> usize;
    fn nb_scenes_set_policy(ctx: *mut NbScenes, features: u32, hidden: u32, policies: u32, weights_host: *const f32, accel_limit: f32) -> c_int;
    fn nb_scenes_step_policy(ctx: *mut NbScenes, k: u32, up_xyz: *const f32, cp16: *const f32, width: u32) -> c_int;
    fn nb_scenes_eyes_policy(ctx: *mut NbScenes, first_scene: u32, scene_count: u32, up_xyz: *const f32, cp16: *const f32, width: u32, feat: *mut f32, act: *mut f32) -> c_int;
    fn nb_scenes_policy_step_launch(params: *const NbParams, scenes: u32, n: u32, cams_16: *const c_void, inst_16: *const c_void, width: u32, up_xyz: *const f32, features: u32, hidden: u32, policies: u32, weights: *const c_void, accel_limit: f32, pos_in: *const c_void, vel_in: *const c_void, pos_out: *mut c_void, vel_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn nb_scenes_policy_observe_launch(scenes: u32, n: u32, first_eye: u32, count: u32, cams_16: *const c_void, inst_16: *const c_void, width: u32, features: u32, hidden: u32, policies: u32, weights: *const c_void, accel_limit: f32, feat_out: *mut c_void, act_out: *mut c_void, stream: *mut c_void) -> c_int;
    // the score of every scene, accumulated on the device (include/nenbody_scenes_score.h)
    fn nb_scenes_score_launch(sp: *const NbScoreParams, scenes: u32, n: u32, pos: *const c_void, vel: *const c_void, score: *mut c_void, stream: *mut c_void) -> c_int;
    fn nb_scenes_set_score(ctx: *mut NbScenes, sp: *const NbScoreParams) -> c_int;
    fn nb_scenes_score(ctx: *mut NbScenes) -> c_int;
    fn nb_scenes_score_reset(ctx: *mut NbScenes) -> c_int;
    fn nb_scenes_scores(ctx: *mut NbScenes, first_scene: u32, scene_count: u32, out_host: *mut NbSceneScore) -> c_int;
    fn nb_scenes_step_policy_scored(ctx: *mut NbScenes, k: u32, up_xyz: *const f32, cp16: *const f32, width: u32) -> c_int;
    // an evolution-strategies generation on the device (include/nenbody_scenes_es.h)
    fn nb_scenes_es_perturb_launch(ep: *const NbEsParams, features: u32, hidden: u32, generation: u32, first_scene: u32, count: u32, mean: *const c_void, theta_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn nb_scenes_es_update_launch(ep: *const NbEsParams, features: u32, hidden: u32, generation: u32, scenes: u32, score: *const c_void, mean: *const c_void, mean_out: *mut c_void, rank_out: *mut c_void, fitness_out: *mut c_void, report_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn nb_scenes_es_set(ctx: *mut NbScenes, features: u32, hidden: u32, mean_host: *const f32, accel_limit: f32, ep: *const NbEsParams) -> c_int;
    fn nb_scenes_es_perturb(ctx: *mut NbScenes) -> c_int;
    fn nb_scenes_es_update(ctx: *mut NbScenes) -> c_int;
    fn nb_scenes_es_mean(ctx: *mut NbScenes, out_host: *mut f32) -> c_int;
    fn nb_scenes_es_result(ctx: *mut NbScenes, report: *mut NbEsReport, fitness: *mut f32, rank: *mut u32) -> c_int;
    fn nb_scenes_es_generation(ctx: *const NbScenes) -> u32;
    fn nb_scenes_keep(ctx: *mut NbScenes) -> c_int;
    fn nb_scenes_rewind(ctx: *mut NbScenes) -> c_int;
    // a recurrent policy with per-body memory (include/nenbody_scenes_policy_recurrent.h)
    fn nb_policy_recurrent_floats(features: u32, hidden: u32) -> usize;
    fn nb_scenes_set_policy_recurrent(ctx: *mut NbScenes, features: u32, hidden: u32, policies: u32, weights_host: *const f32, accel_limit: f32, memory_limit: f32) -> c_int;
    fn nb_scenes_eyes_policy_memory(ctx: *mut NbScenes, first_scene: u32, scene_count: u32, up_xyz: *const f32, cp16: *const f32, width: u32, feat: *mut f32, act: *mut f32, mem_next: *mut f32) -> c_int;
    fn nb_scenes_memory_reset(ctx: *mut NbScenes) -> c_int;
    fn nb_scenes_memory(ctx: *mut NbScenes, first_scene: u32, scene_count: u32, out_host: *mut f32) -> c_int;
    fn nb_scenes_set_memory(ctx: *mut NbScenes, mem_host: *const f32) -> c_int;
    fn nb_scenes_es_set_recurrent(ctx: *mut NbScenes, features: u32, hidden: u32, mean_host: *const f32, accel_limit: f32, memory_limit: f32, ep: *const NbEsParams) -> c_int;
    fn nb_scenes_policy_recurrent_step_launch(params: *const NbParams, scenes: u32, n: u32, cams_16: *const c_void, inst_16: *const c_void, width: u32, up_xyz: *const f32, features: u32, hidden: u32, policies: u32, weights: *const c_void, accel_limit: f32, memory_limit: f32, pos_in: *const c_void, vel_in: *const c_void, mem_in: *const c_void, pos_out: *mut c_void, vel_out: *mut c_void, mem_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn nb_scenes_policy_recurrent_observe_launch(scenes: u32, n: u32, first_eye: u32, count: u32, cams_16: *const c_void, inst_16: *const c_void, width: u32, features: u32, hidden: u32, policies: u32, weights: *const c_void, accel_limit: f32, memory_limit: f32, mem: *const c_void, feat_out: *mut c_void, act_out: *mut c_void, mem_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn nb_scenes_es_perturb_floats_launch(ep: *const NbEsParams, floats: u32, generation: u32, first_scene: u32, count: u32, mean: *const c_void, theta_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn nb_scenes_es_update_floats_launch(ep: *const NbEsParams, floats: u32, generation: u32, scenes: u32, score: *const c_void, mean: *const c_void, mean_out: *mut c_void, rank_out: *mut c_void, fitness_out: *mut c_void, report_out: *mut c_void, stream: *mut c_void) -> c_int;
    // the same on caller-owned device memory, in place
    fn nb_scenes_nbody_step_launch(params: *const NbParams, scenes: u32, n: u32, k: u32, pos: *mut c_void, vel: *mut c_void, stream: *mut c_void) -> c_int;
    fn nb_scenes_boids_step_launch(params: *const NbBoidsParams, scenes: u32, n: u32, k: u32, pos: *mut c_void, vel: *mut c_void, stream: *mut c_void) -> c_int;
}

#[repr(C)]
pub struct NbScenes {
    _private: [u8; 0],
}

/// nb_score_params: the squared radius of `near` (Q2) and the goal (Q5)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct NbScoreParams {
    pub radius_sq: f32,
    pub goal: [f32; 3],
}

/// nb_scene_score, 32 bytes: what a scene's snapshots have added up to (Q7)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct NbSceneScore {
    pub near: u64,
    pub spread: f32,
    pub speed2: f32,
    pub momentum2: f32,
    pub goal2: f32,
    pub steps: u32,
    pub nonfinite: u32,
}

/// nb_es_params, 40 bytes: the draw's scale (E3), the update's step (E7), the fitness's coefficients over (near, spread, speed2,
/// momentum2, goal2, nonfinite) (E4) and the generator's seed (E1)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct NbEsParams {
    pub sigma: f32,
    pub step: f32,
    pub coef: [f32; 6],
    pub seed: u64,
}

/// nb_es_report, 16 bytes: what the ranking of a generation leaves
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct NbEsReport {
    pub best_scene: u32,
    pub best_fitness: f32,
    pub nan_count: u32,
    pub generation: u32,
}

pub const NB_ES_MAX_POPULATION: u32 = 4096;
pub const NB_SCENES_MAX_BODIES: u32 = 2048;
pub const NB_POLICY_MAX_FEATURES: u32 = 256;
pub const NB_POLICY_MAX_HIDDEN: u32 = 64;

/// The floats of one recurrent policy of shape (features, hidden): w1[f * H + j], wr[r * H + j], b1[j], w2[k * H + j], b2[k]; 0 for a
/// shape outside the limits.
pub fn policy_recurrent_floats(features: u32, hidden: u32) -> usize {
    unsafe { nb_policy_recurrent_floats(features, hidden) }
}

/// The floats of one policy of shape (features, hidden): w1[f * H + j], b1[j], w2[k * H + j] for k = 0, 1, b2[k]; 0 for a shape
/// outside the limits.
pub fn policy_floats(features: u32, hidden: u32) -> usize {
    unsafe { nb_policy_floats(features, hidden) }
}

pub const NB_FRAME_MAX_DIM: u32 = 4096;
pub const NB_FRAME_MSAA_MAX_DIM: u32 = 2048;

/// The scene camera's constant as the reference forms it for a `width` x `height` target (src/main.rs:753-762,
/// src/gfx.rs:379-383: the angle divided by the aspect ratio).
pub fn frame_constant(width: u32, height: u32) -> Result<[[f32; 4]; 4], SceneError> {
    check_abi();
    let a = width as f32 / height as f32;
    let mut cp = [[0.0f32; 4]; 4];
    check(unsafe { nb_camera_constant(90.0 / a, a, 1.0, 10000.0, cp.as_mut_ptr() as *mut f32) }, std::ptr::null())?;
    Ok(cp)
}

/// Bytes of the key plane `nb_launch_frame` needs for an extent (0 for an invalid one); `Scene::frame` keeps its own.
pub fn frame_scratch_bytes(width: u32, height: u32) -> usize {
    unsafe { nb_frame_scratch_bytes(width, height) }
}

/// What `Scene::frame` returns: `height` rows of `width` pixels, row 0 the top.
pub struct Frame {
    pub width: u32,
    pub height: u32,
    pub ids: Vec<u32>,       // the instance drawn at the pixel, NB_EYES_NONE where none
    pub depth: Vec<f32>,     // the depth attachment's value, 1.0 where none
    pub rgba: Vec<[f32; 4]>, // linear, what the fragment shader writes
    pub bgra8: Vec<u32>,     // the texel of the Bgra8UnormSrgb target, bytes B, G, R, A
}

/// Bytes of the key plane `nb_launch_frame_msaa` needs for an extent (0 for an invalid one); `Scene::frame_msaa` keeps its own.
pub fn frame_msaa_scratch_bytes(width: u32, height: u32) -> usize {
    unsafe { nb_frame_msaa_scratch_bytes(width, height) }
}

/// Where the eight samples of a pixel lie: sample k of pixel (c, r) is at (c + o[0][k], r + o[1][k]) -- Vulkan's standard
/// 8-sample pattern, the reference's `msaa_samples = 8`, src/main.rs:652; o[0] is `eye_sample_offsets`.
pub fn frame_sample_offsets() -> Result<[[f32; NB_EYES_SAMPLES]; 2], SceneError> {
    check_abi();
    let mut o = [[0.0f32; NB_EYES_SAMPLES]; 2];
    check(unsafe { nb_frame_sample_offsets(o.as_mut_ptr() as *mut f32) }, std::ptr::null())?;
    Ok(o)
}

/// What `Scene::frame_msaa` returns: per pixel its eight samples and the resolved colour; row 0 the top.
pub struct FrameMsaa {
    pub width: u32,
    pub height: u32,
    pub ids8: Vec<[u32; NB_EYES_SAMPLES]>,   // the instance drawn at each sample, NB_EYES_NONE where none
    pub depth8: Vec<[f32; NB_EYES_SAMPLES]>, // the depth per sample, 1.0 where none
    pub rgba: Vec<[f32; 4]>,                 // linear: the mean of the samples' fragments and the clear colour
    pub bgra8: Vec<u32>,                     // the texel of the resolved Bgra8UnormSrgb target, bytes B, G, R, A
}

pub const NB_EYES_NONE: u32 = 0xFFFF_FFFF;
pub const NB_EYES_SEE_SELF: u32 = 1;

/// The eye cameras' constant as the reference forms it for rows of `width` pixels (src/main.rs:693-697, src/gfx.rs:379-383).
pub fn eye_constant(width: u32) -> Result<[[f32; 4]; 4], SceneError> {
    check_abi();
    let mut cp = [[0.0f32; 4]; 4];
    check(unsafe { nb_camera_constant(90.0 / width as f32, width as f32 / 1.0, 1.0, 10000.0, cp.as_mut_ptr() as *mut f32) }, std::ptr::null())?;
    Ok(cp)
}

/// An 8-bit sRGB image (`Rgba8UnormSrgb`, src/main.rs:338) as the linear texels `Scene::set_skin` takes: colour through the
/// library's decode table, alpha / 255.
pub fn skin_from_srgb8(rgba8: &[[u8; 4]]) -> Result<Vec<[f32; 4]>, SceneError> {
    check_abi();
    let mut d = [0.0f32; 256];
    check(unsafe { nb_srgb_decode_table(d.as_mut_ptr()) }, std::ptr::null())?;
    Ok(rgba8.iter().map(|p| [d[p[0] as usize], d[p[1] as usize], d[p[2] as usize], p[3] as f32 / 255.0]).collect())
}

/// Linear values as the bytes an sRGB target stores (the exact nearest byte; a NaN gives 0).
pub fn srgb_encode(linear: &[f32]) -> Result<Vec<u8>, SceneError> {
    check_abi();
    let mut out = vec![0u8; linear.len()];
    check(unsafe { nb_srgb_encode(linear.as_ptr(), linear.len(), out.as_mut_ptr()) }, std::ptr::null())?;
    Ok(out)
}

/// What `Scene::eyes` returns: `count` rows of `width` columns each.
pub struct Eyes {
    pub width: u32,
    pub ids: Vec<u32>,   // the nearest instance per column, NB_EYES_NONE where none
    pub depth: Vec<f32>, // the depth attachment's value, 1.0 where none
}

/// What `Scene::seen` returns: per eye the entities that occur in its row, ascending; row e of `ids` / `depth` / `cols` has `width`
/// slots, `count[e]` of them used.
pub struct Seen {
    pub width: u32,
    pub count: Vec<u32>,
    pub ids: Vec<u32>,   // NB_EYES_NONE behind the used slots
    pub depth: Vec<f32>, // the nearest depth at which the eye sees the entity, 1.0 behind the used slots
    pub cols: Vec<u32>,  // the number of columns the entity holds, 0 behind the used slots
}

/// What `Scene::located` returns: `Seen`'s lists plus, per member, where the eye sees it.
pub struct Located {
    pub width: u32,
    pub count: Vec<u32>,
    pub ids: Vec<u32>,
    pub depth: Vec<f32>,
    pub cols: Vec<u32>,
    pub col: Vec<u32>,      // the column at which the entity is nearest, NB_EYES_NONE behind the used slots
    pub rel: Vec<[f32; 4]>, // the seen point relative to the eye in world axes and its range (x, y, z, r), +0 behind the used slots
}

/// What `Scene::eyes_colour` returns: the same plus the colour attachment.
pub struct EyesColour {
    pub width: u32,
    pub ids: Vec<u32>,
    pub depth: Vec<f32>,
    pub rgba: Vec<[f32; 4]>, // linear, what the fragment shader writes
    pub bgra8: Vec<u32>,     // the texel of the Bgra8UnormSrgb target, bytes B, G, R, A: what the imgui texture takes
}

pub const NB_EYES_SAMPLES: usize = 8;
pub const NB_EYES_MSAA_MAX_WIDTH: u32 = 2048;

/// Where the eight samples of a column lie: sample k of column c is at c + o[k] (the x coordinates of Vulkan's standard
/// 8-sample pattern, the reference's `msaa_samples = 8`, src/main.rs:652).
pub fn eye_sample_offsets() -> Result<[f32; NB_EYES_SAMPLES], SceneError> {
    check_abi();
    let mut o = [0.0f32; NB_EYES_SAMPLES];
    check(unsafe { nb_eyes_sample_offsets(o.as_mut_ptr()) }, std::ptr::null())?;
    Ok(o)
}

/// What `Scene::eyes_msaa` returns: per column its eight samples and the resolved colour.
pub struct EyesMsaa {
    pub width: u32,
    pub ids8: Vec<[u32; NB_EYES_SAMPLES]>,   // the nearest instance per sample, NB_EYES_NONE where none
    pub depth8: Vec<[f32; NB_EYES_SAMPLES]>, // the depth per sample, 1.0 where none
    pub rgba: Vec<[f32; 4]>,                 // linear: the mean of the samples' fragments and the clear colour
    pub bgra8: Vec<u32>,                     // the texel of the resolved Bgra8UnormSrgb target, bytes B, G, R, A
}

fn check_abi() {
    static ONCE: std::sync::Once = std::sync::Once::new();
    ONCE.call_once(|| {
        let got = unsafe { nb_abi_version() };
        assert_eq!(got, NB_ABI_VERSION, "libnenbody_hip.so speaks ABI {}, this binding was written against ABI {}", got, NB_ABI_VERSION);
    });
}

impl Default for NbParams {
    fn default() -> Self {
        check_abi();
        let mut p = NbParams { dt: 0.0, g: 0.0, bias: 0.0, tile: 0, mode: 0 };
        unsafe { nb_default_params(&mut p) };
        p
    }
}

#[derive(Debug)]
pub struct SceneError(pub i32, pub String);

fn check(rc: c_int, ctx: *const NbCtx) -> Result<(), SceneError> {
    if rc == 0 {
        return Ok(());
    }
    let msg = unsafe { CStr::from_ptr(nb_last_error(ctx)) }.to_string_lossy().into_owned();
    Err(SceneError(rc, msg))
}

/// Single owner of a device context: `Send`, not `Sync` (the reference calls the update on the winit main
/// thread, src/main.rs:925).
pub struct Scene {
    ctx: *mut NbCtx,
    pub positions: Vec<Point3<f32>>,   // src/main.rs:743
    pub velocities: Vec<Vector3<f32>>, // src/main.rs:738
    pub instances: Vec<[[f32; 4]; 4]>, // instance_data, uploaded at src/main.rs:932-936
}

unsafe impl Send for Scene {}

impl Scene {
    /// `entity_count` bodies with the reference's initial distributions (src/main.rs:738-747), seeded.
    pub fn new(n: usize, params: NbParams, seed: u64) -> Result<Scene, SceneError> {
        check_abi();
        let mut positions = vec![Point3::new(0.0f32, 0.0, 0.0); n];
        let mut velocities = vec![Vector3::new(0.0f32, 0.0, 0.0); n];
        // Point3<f32> / Vector3<f32> are #[repr(C)] {x, y, z}: the Vec's buffer is the stride-3 array the ABI takes
        check(
            unsafe { nb_init_state(seed, n as u32, positions.as_mut_ptr() as *mut f32, velocities.as_mut_ptr() as *mut f32) },
            std::ptr::null(),
        )?;
        Scene::from_state(positions, velocities, params)
    }

    pub fn from_state(positions: Vec<Point3<f32>>, velocities: Vec<Vector3<f32>>, params: NbParams) -> Result<Scene, SceneError> {
        check_abi();
        // same panic the reference has at src/main.rs:415-416 (copy_from_slice on unequal lengths)
        assert_eq!(positions.len(), velocities.len(), "positions and velocities must have the same length");
        let n = positions.len();
        let mut ctx: *mut NbCtx = std::ptr::null_mut();
        check(unsafe { nb_create(n as u32, 1, &params, &mut ctx) }, std::ptr::null())?;
        let scene = Scene { ctx, positions, velocities, instances: vec![[[0.0; 4]; 4]; n] };
        check(
            unsafe { nb_upload(scene.ctx, scene.positions.as_ptr() as *const f32, scene.velocities.as_ptr() as *const f32) },
            scene.ctx,
        )?;
        Ok(scene)
    }

    /// One `update_instance_nbody` (src/main.rs:404-441); host mirrors refreshed so the consumers at
    /// src/main.rs:932-945 work unchanged.
    pub fn step(&mut self) -> Result<(), SceneError> {
        check(unsafe { nb_step(self.ctx, 1) }, self.ctx)?;
        check(
            unsafe {
                nb_download(
                    self.ctx,
                    self.positions.as_mut_ptr() as *mut f32,
                    self.velocities.as_mut_ptr() as *mut f32,
                    self.instances.as_mut_ptr() as *mut f32,
                )
            },
            self.ctx,
        )
    }

    /// One `update_instance_boids` (src/main.rs:443-526) with the reference's constants; host mirrors refreshed.
    pub fn step_boids(&mut self) -> Result<(), SceneError> {
        check(unsafe { nb_step_boids(self.ctx, 1, std::ptr::null()) }, self.ctx)?;
        check(
            unsafe {
                nb_download(
                    self.ctx,
                    self.positions.as_mut_ptr() as *mut f32,
                    self.velocities.as_mut_ptr() as *mut f32,
                    self.instances.as_mut_ptr() as *mut f32,
                )
            },
            self.ctx,
        )
    }

    /// k steps, device-resident, no download: the benchmark path.
    pub fn step_n(&mut self, k: u32) -> Result<(), SceneError> {
        check(unsafe { nb_step(self.ctx, k) }, self.ctx)
    }

    pub fn sync(&mut self) -> Result<(), SceneError> {
        check(unsafe { nb_sync(self.ctx) }, self.ctx)
    }

    /// Every entity's eye view for bodies [first, first + count) of the current state (nb_eyes): replaces
    /// `eye_cams.update` (src/main.rs:939) and the depth side of `build_command_buffer_parallel` (:962-977).
    /// `cp` is the eyes' camera constant (`eye_constant(width)` is the reference's), `up` its `normal`.
    pub fn eyes(&mut self, cp: &[[f32; 4]; 4], up: Vector3<f32>, width: u32, first: u32, count: u32, see_self: bool) -> Result<Eyes, SceneError> {
        let cells = count as usize * width as usize;
        let mut e = Eyes { width, ids: vec![0; cells.max(1)], depth: vec![0.0; cells.max(1)] };
        let up = [up.x, up.y, up.z];
        let flags = if see_self { NB_EYES_SEE_SELF } else { 0 };
        check(
            unsafe { nb_eyes(self.ctx, first, count, up.as_ptr(), cp.as_ptr() as *const f32, width, flags, e.ids.as_mut_ptr(), e.depth.as_mut_ptr()) },
            self.ctx,
        )?;
        e.ids.truncate(cells);
        e.depth.truncate(cells);
        Ok(e)
    }

    /// The seen set of every eye (nb_eyes_seen) for bodies [first, first + count): which entities occur in the eye's row of `eyes`.
    pub fn seen(&mut self, cp: &[[f32; 4]; 4], up: Vector3<f32>, width: u32, first: u32, count: u32, see_self: bool) -> Result<Seen, SceneError> {
        let cells = count as usize * width as usize;
        let mut s = Seen { width, count: vec![0; (count as usize).max(1)], ids: vec![0; cells.max(1)], depth: vec![0.0; cells.max(1)], cols: vec![0; cells.max(1)] };
        let up = [up.x, up.y, up.z];
        let flags = if see_self { NB_EYES_SEE_SELF } else { 0 };
        check(
            unsafe {
                nb_eyes_seen(
                    self.ctx, first, count, up.as_ptr(), cp.as_ptr() as *const f32, width, flags,
                    s.count.as_mut_ptr(), s.ids.as_mut_ptr(), s.depth.as_mut_ptr(), s.cols.as_mut_ptr(),
                )
            },
            self.ctx,
        )?;
        s.count.truncate(count as usize);
        s.ids.truncate(cells);
        s.depth.truncate(cells);
        s.cols.truncate(cells);
        Ok(s)
    }

    /// One update_instance_boids restricted to what each entity sees (nb_step_boids_seen): entity n folds over the entities of its
    /// own eye row instead of over every entity; one that sees nobody stops.  Replaces the call at src/main.rs:925; mirrors refreshed.
    pub fn step_boids_seen(&mut self, cp: &[[f32; 4]; 4], up: Vector3<f32>, width: u32) -> Result<(), SceneError> {
        let up = [up.x, up.y, up.z];
        check(unsafe { nb_step_boids_seen(self.ctx, 1, std::ptr::null(), up.as_ptr(), cp.as_ptr() as *const f32, width, 0) }, self.ctx)?;
        check(
            unsafe {
                nb_download(
                    self.ctx,
                    self.positions.as_mut_ptr() as *mut f32,
                    self.velocities.as_mut_ptr() as *mut f32,
                    self.instances.as_mut_ptr() as *mut f32,
                )
            },
            self.ctx,
        )
    }

    /// Where every eye sees the members of its seen set (nb_eyes_located) for bodies [first, first + count): `seen`'s lists plus the
    /// column and the relative position of each member, formed from the eye's row, its heading, `up` and `cp` alone.  `cp` must be
    /// a perspective constant as `camera_constant` forms it.
    pub fn located(&mut self, cp: &[[f32; 4]; 4], up: Vector3<f32>, width: u32, first: u32, count: u32, see_self: bool) -> Result<Located, SceneError> {
        let cells = count as usize * width as usize;
        let mut s = Located {
            width,
            count: vec![0; (count as usize).max(1)],
            ids: vec![0; cells.max(1)],
            depth: vec![0.0; cells.max(1)],
            cols: vec![0; cells.max(1)],
            col: vec![0; cells.max(1)],
            rel: vec![[0.0; 4]; cells.max(1)],
        };
        let up = [up.x, up.y, up.z];
        let flags = if see_self { NB_EYES_SEE_SELF } else { 0 };
        check(
            unsafe {
                nb_eyes_located(
                    self.ctx, first, count, up.as_ptr(), cp.as_ptr() as *const f32, width, flags,
                    s.count.as_mut_ptr(), s.ids.as_mut_ptr(), s.depth.as_mut_ptr(), s.cols.as_mut_ptr(), s.col.as_mut_ptr(),
                    s.rel.as_mut_ptr() as *mut f32,
                )
            },
            self.ctx,
        )?;
        s.count.truncate(count as usize);
        s.ids.truncate(cells);
        s.depth.truncate(cells);
        s.cols.truncate(cells);
        s.col.truncate(cells);
        s.rel.truncate(cells);
        Ok(s)
    }

    /// One update_instance_nbody from vision alone (nb_step_nbody_located): entity n folds the reference's law over the relative
    /// positions of `located` instead of over p_i - p_n; one that sees nobody coasts.  Replaces the call at src/main.rs:925; mirrors
    /// refreshed.
    pub fn step_nbody_located(&mut self, cp: &[[f32; 4]; 4], up: Vector3<f32>, width: u32) -> Result<(), SceneError> {
        let up = [up.x, up.y, up.z];
        check(unsafe { nb_step_nbody_located(self.ctx, 1, up.as_ptr(), cp.as_ptr() as *const f32, width, 0) }, self.ctx)?;
        check(
            unsafe {
                nb_download(
                    self.ctx,
                    self.positions.as_mut_ptr() as *mut f32,
                    self.velocities.as_mut_ptr() as *mut f32,
                    self.instances.as_mut_ptr() as *mut f32,
                )
            },
            self.ctx,
        )
    }

    /// The skin the colour rows sample: `tw` x `th` linear RGBA texels, row 0 first (`skin_from_srgb8` for the decoded
    /// assets/skin.png); `None`: the 1 x 1 white skin.
    pub fn set_skin(&mut self, skin: Option<(&[[f32; 4]], u32, u32)>) -> Result<(), SceneError> {
        match skin {
            None => check(unsafe { nb_eyes_skin(self.ctx, std::ptr::null(), 0, 0) }, self.ctx),
            Some((texels, tw, th)) => {
                if texels.len() != tw as usize * th as usize {
                    return Err(SceneError(-1, "a skin needs tw * th texels".to_string())); // NB_ERR_INVALID
                }
                check(unsafe { nb_eyes_skin(self.ctx, texels.as_ptr() as *const f32, tw, th) }, self.ctx)
            }
        }
    }

    /// The same pass with its colour row (nb_eyes_colour): with it a host drops `build_command_buffer_parallel` and the
    /// viewport pass (src/main.rs:962-998) and writes row `viewport_camera` of `bgra8` into its imgui texture.
    pub fn eyes_colour(&mut self, cp: &[[f32; 4]; 4], up: Vector3<f32>, width: u32, first: u32, count: u32, see_self: bool) -> Result<EyesColour, SceneError> {
        let cells = count as usize * width as usize;
        let mut e = EyesColour {
            width,
            ids: vec![0; cells.max(1)],
            depth: vec![0.0; cells.max(1)],
            rgba: vec![[0.0; 4]; cells.max(1)],
            bgra8: vec![0; cells.max(1)],
        };
        let up = [up.x, up.y, up.z];
        let flags = if see_self { NB_EYES_SEE_SELF } else { 0 };
        check(
            unsafe {
                nb_eyes_colour(
                    self.ctx, first, count, up.as_ptr(), cp.as_ptr() as *const f32, width, flags,
                    e.ids.as_mut_ptr(), e.depth.as_mut_ptr(), e.rgba.as_mut_ptr() as *mut f32, e.bgra8.as_mut_ptr(),
                )
            },
            self.ctx,
        )?;
        e.ids.truncate(cells);
        e.depth.truncate(cells);
        e.rgba.truncate(cells);
        e.bgra8.truncate(cells);
        Ok(e)
    }

    /// The eye rows through 8 samples per column, resolved as the reference's targets are (nb_eyes_msaa; `resolve_target`,
    /// src/main.rs:547, 611): a span end covers a fraction of its column.  `width` is at most NB_EYES_MSAA_MAX_WIDTH.
    pub fn eyes_msaa(&mut self, cp: &[[f32; 4]; 4], up: Vector3<f32>, width: u32, first: u32, count: u32, see_self: bool) -> Result<EyesMsaa, SceneError> {
        let cells = count as usize * width as usize;
        let mut e = EyesMsaa {
            width,
            ids8: vec![[0; NB_EYES_SAMPLES]; cells.max(1)],
            depth8: vec![[0.0; NB_EYES_SAMPLES]; cells.max(1)],
            rgba: vec![[0.0; 4]; cells.max(1)],
            bgra8: vec![0; cells.max(1)],
        };
        let up = [up.x, up.y, up.z];
        let flags = if see_self { NB_EYES_SEE_SELF } else { 0 };
        check(
            unsafe {
                nb_eyes_msaa(
                    self.ctx, first, count, up.as_ptr(), cp.as_ptr() as *const f32, width, flags,
                    e.ids8.as_mut_ptr() as *mut u32, e.depth8.as_mut_ptr() as *mut f32, e.rgba.as_mut_ptr() as *mut f32, e.bgra8.as_mut_ptr(),
                )
            },
            self.ctx,
        )?;
        e.ids8.truncate(cells);
        e.depth8.truncate(cells);
        e.rgba.truncate(cells);
        e.bgra8.truncate(cells);
        Ok(e)
    }

    /// One camera from a host-supplied eye and direction (nb_camera_at).  The reference's scene camera (src/main.rs:753-762,
    /// 940-942): `camera_at(Point3::new(p.x, p.y, 990.0), -Vector3::unit_z(), Vector3::unit_x(), &frame_constant(w, h)?)`.
    pub fn camera_at(&mut self, eye: Point3<f32>, dir: Vector3<f32>, up: Vector3<f32>, cp: &[[f32; 4]; 4]) -> Result<[[f32; 4]; 4], SceneError> {
        let (eye, dir, up) = ([eye.x, eye.y, eye.z], [dir.x, dir.y, dir.z], [up.x, up.y, up.z]);
        let mut out = [[0.0f32; 4]; 4];
        check(
            unsafe { nb_camera_at(self.ctx, eye.as_ptr(), dir.as_ptr(), up.as_ptr(), cp.as_ptr() as *const f32, out.as_mut_ptr() as *mut f32) },
            self.ctx,
        )?;
        Ok(out)
    }

    /// The scene camera's frame of the current state (nb_frame): with it a headless host drops `render(&display, ...)`
    /// (src/main.rs:948-960) and presents, saves or streams `bgra8`.  The skin is `set_skin`'s.
    pub fn frame(&mut self, camera: &[[f32; 4]; 4], width: u32, height: u32) -> Result<Frame, SceneError> {
        let cells = width as usize * height as usize;
        let mut f = Frame {
            width,
            height,
            ids: vec![0; cells.max(1)],
            depth: vec![0.0; cells.max(1)],
            rgba: vec![[0.0; 4]; cells.max(1)],
            bgra8: vec![0; cells.max(1)],
        };
        check(
            unsafe {
                nb_frame(
                    self.ctx, camera.as_ptr() as *const f32, width, height, 0,
                    f.ids.as_mut_ptr(), f.depth.as_mut_ptr(), f.rgba.as_mut_ptr() as *mut f32, f.bgra8.as_mut_ptr(),
                )
            },
            self.ctx,
        )?;
        Ok(f)
    }

    /// The same frame through 8 samples per pixel, resolved as the reference's display target is (nb_frame_msaa): a line that
    /// crosses a pixel off-centre still shows there.  `width` and `height` are at most NB_FRAME_MSAA_MAX_DIM.
    pub fn frame_msaa(&mut self, camera: &[[f32; 4]; 4], width: u32, height: u32) -> Result<FrameMsaa, SceneError> {
        let valid = (1..=NB_FRAME_MSAA_MAX_DIM).contains(&width) && (1..=NB_FRAME_MSAA_MAX_DIM).contains(&height);
        let cells = if valid { width as usize * height as usize } else { 0 }; // (an extent the library refuses: nothing to allocate)
        let mut f = FrameMsaa {
            width,
            height,
            ids8: vec![[0; NB_EYES_SAMPLES]; cells.max(1)],
            depth8: vec![[0.0; NB_EYES_SAMPLES]; cells.max(1)],
            rgba: vec![[0.0; 4]; cells.max(1)],
            bgra8: vec![0; cells.max(1)],
        };
        check(
            unsafe {
                nb_frame_msaa(
                    self.ctx, camera.as_ptr() as *const f32, width, height, 0,
                    f.ids8.as_mut_ptr() as *mut u32, f.depth8.as_mut_ptr() as *mut f32, f.rgba.as_mut_ptr() as *mut f32, f.bgra8.as_mut_ptr(),
                )
            },
            self.ctx,
        )?;
        Ok(f)
    }
}

impl Drop for Scene {
    fn drop(&mut self) {
        unsafe { nb_destroy(self.ctx) };
    }
}

/// Drop-in for the reference's free function (same five arguments, src/main.rs:404-410): the body is one FFI call.
/// The snapshot copies (src/main.rs:415-416), the `zip` truncation (src/main.rs:420-423) and the fold over all of
/// `old_positions` happen inside `nb_update_instance_nbody`; a length mismatch panics here as `copy_from_slice`
/// does there.  One upload, one step, one download per call; the device context is kept by the library.
pub fn update_instance_nbody(
    instances: &mut Vec<[[f32; 4]; 4]>,
    positions: &mut Vec<Point3<f32>>,
    old_positions: &mut Vec<Point3<f32>>,
    velocities: &mut Vec<Vector3<f32>>,
    old_velocities: &mut Vec<Vector3<f32>>,
) {
    check_abi();
    let rc = unsafe {
        nb_update_instance_nbody(
            instances.as_mut_ptr() as *mut f32, instances.len(),
            positions.as_mut_ptr() as *mut f32, positions.len(),
            old_positions.as_mut_ptr() as *mut f32, old_positions.len(),
            velocities.as_mut_ptr() as *mut f32, velocities.len(),
            old_velocities.as_mut_ptr() as *mut f32, old_velocities.len(),
            std::ptr::null(),
        )
    };
    if let Err(SceneError(code, msg)) = check(rc, std::ptr::null()) {
        panic!("update_instance_nbody: {} ({})", msg, code);
    }
}

/// The controller the event loop calls today (src/main.rs:443-449, call site src/main.rs:925-931), same contract.
pub fn update_instance_boids(
    instances: &mut Vec<[[f32; 4]; 4]>,
    positions: &mut Vec<Point3<f32>>,
    old_positions: &mut Vec<Point3<f32>>,
    velocities: &mut Vec<Vector3<f32>>,
    old_velocities: &mut Vec<Vector3<f32>>,
) {
    check_abi();
    let rc = unsafe {
        nb_update_instance_boids(
            instances.as_mut_ptr() as *mut f32, instances.len(),
            positions.as_mut_ptr() as *mut f32, positions.len(),
            old_positions.as_mut_ptr() as *mut f32, old_positions.len(),
            velocities.as_mut_ptr() as *mut f32, velocities.len(),
            old_velocities.as_mut_ptr() as *mut f32, old_velocities.len(),
            std::ptr::null(),
        )
    };
    if let Err(SceneError(code, msg)) = check(rc, std::ptr::null()) {
        panic!("update_instance_boids: {} ({})", msg, code);
    }
}

/// The third controller with the reference's own signature (src/main.rs:381-385): a drop-in for the function body.
/// The reference draws from an unseeded `thread_rng`; the library draws from a counter-based stream whose seed and call
/// counter it keeps itself (`update_random_seed` restarts it).
pub fn update_instance_random(
    instances: &mut Vec<[[f32; 4]; 4]>,
    positions: &mut Vec<Point3<f32>>,
    velocities: &mut Vec<Vector3<f32>>,
) {
    check_abi();
    let rc = unsafe {
        nb_update_instance_random(
            instances.as_mut_ptr() as *mut f32, instances.len(),
            positions.as_mut_ptr() as *mut f32, positions.len(),
            velocities.as_mut_ptr() as *mut f32, velocities.len(),
        )
    };
    if let Err(SceneError(code, msg)) = check(rc, std::ptr::null()) {
        panic!("update_instance_random: {} ({})", msg, code);
    }
}

/// The same step at a stream position the caller names (`step` = the frame number): independent of how a run is split.
pub fn update_instance_random_seeded(
    instances: &mut Vec<[[f32; 4]; 4]>,
    positions: &mut Vec<Point3<f32>>,
    velocities: &mut Vec<Vector3<f32>>,
    seed: u64,
    step: u64,
) {
    check_abi();
    let rc = unsafe {
        nb_update_instance_random_seeded(
            instances.as_mut_ptr() as *mut f32, instances.len(),
            positions.as_mut_ptr() as *mut f32, positions.len(),
            velocities.as_mut_ptr() as *mut f32, velocities.len(),
            seed, step,
        )
    };
    if let Err(SceneError(code, msg)) = check(rc, std::ptr::null()) {
        panic!("update_instance_random_seeded: {} ({})", msg, code);
    }
}

/// Seed of `update_instance_random`'s stream; restarts its call counter.
pub fn update_random_seed(seed: u64) {
    unsafe { nb_update_random_seed(seed) }
}

fn check_scenes(rc: c_int, ctx: *const NbScenes) -> Result<(), SceneError> {
    if rc == 0 {
        return Ok(());
    }
    let msg = unsafe { CStr::from_ptr(nb_scenes_last_error(ctx)) }.to_string_lossy().into_owned();
    Err(SceneError(rc, msg))
}

/// What `SceneBatch::located` returns: per eye `s * n + i` its count and `width` slots of each list (no column counts).
pub struct BatchLocated {
    pub width: u32,
    pub count: Vec<u32>,
    pub ids: Vec<u32>,
    pub depth: Vec<f32>,
    pub col: Vec<u32>,
    pub rel: Vec<[f32; 4]>,
}

/// B independent scenes of n <= `NB_SCENES_MAX_BODIES` bodies, device-resident; one launch steps every scene k times, one
/// workgroup per scene, and every scene gets the bits a `Scene` of its n bodies gets.  Body i of scene s is element `s * n + i`.
pub struct SceneBatch {
    ctx: *mut NbScenes,
    pub scenes: usize,
    pub n: usize,
    policy_features: usize, // F of the policy set last; 0: none
    policy_hidden: usize,   // H of the recurrent policy set last; 0: none
    es_floats: usize,       // the floats of the search's mean; 0: none
}

unsafe impl Send for SceneBatch {}

impl SceneBatch {
    /// scene s starts from the reference's initial distributions drawn with `seed + s`
    pub fn new(scenes: usize, n: usize, seed: u64, params: NbParams) -> Result<SceneBatch, SceneError> {
        check_abi();
        let mut positions = vec![Point3::new(0.0f32, 0.0, 0.0); scenes * n];
        let mut velocities = vec![Vector3::new(0.0f32, 0.0, 0.0); scenes * n];
        for s in 0..scenes {
            check(
                unsafe {
                    nb_init_state(seed + s as u64, n as u32, positions[s * n..].as_mut_ptr() as *mut f32, velocities[s * n..].as_mut_ptr() as *mut f32)
                },
                std::ptr::null(),
            )?;
        }
        SceneBatch::from_state(scenes, n, &positions, &velocities, params)
    }

    pub fn from_state(scenes: usize, n: usize, positions: &[Point3<f32>], velocities: &[Vector3<f32>], params: NbParams) -> Result<SceneBatch, SceneError> {
        check_abi();
        assert!(positions.len() == scenes * n && velocities.len() == scenes * n, "positions and velocities must hold scenes * n bodies");
        let mut ctx: *mut NbScenes = std::ptr::null_mut();
        check_scenes(unsafe { nb_scenes_create(scenes as u32, n as u32, &params, &mut ctx) }, std::ptr::null())?;
        let batch = SceneBatch { ctx, scenes, n, policy_features: 0, policy_hidden: 0, es_floats: 0 };
        check_scenes(unsafe { nb_scenes_upload(batch.ctx, positions.as_ptr() as *const f32, velocities.as_ptr() as *const f32) }, batch.ctx)?;
        Ok(batch)
    }

    /// k `update_instance_nbody` of every scene (STRICT), asynchronous
    pub fn step(&mut self, k: u32) -> Result<(), SceneError> {
        check_scenes(unsafe { nb_scenes_step(self.ctx, k) }, self.ctx)
    }

    /// k `update_instance_boids` of every scene with the reference's constants, asynchronous
    pub fn step_boids(&mut self, k: u32) -> Result<(), SceneError> {
        check_scenes(unsafe { nb_scenes_step_boids(self.ctx, k, std::ptr::null()) }, self.ctx)
    }

    /// k `update_instance_boids` of every scene restricted to what each entity sees of its own scene,
    /// with the reference's constants, asynchronous; `cp`: the eyes' camera constant, column-major
    pub fn step_boids_seen(&mut self, k: u32, cp: &[[f32; 4]; 4], width: u32) -> Result<(), SceneError> {
        let up = [0.0f32, 0.0, 1.0];
        check_scenes(
            unsafe { nb_scenes_step_boids_seen(self.ctx, k, std::ptr::null(), up.as_ptr(), cp.as_ptr() as *const f32, width) },
            self.ctx,
        )
    }

    /// the seen sets that step folds over, for scenes [first_scene, first_scene + scene_count): (count, ids) with `width` slots an
    /// eye, scene-local ids ascending, NB_EYES_NONE behind the count
    pub fn seen(&mut self, first_scene: u32, scene_count: u32, cp: &[[f32; 4]; 4], width: u32) -> Result<(Vec<u32>, Vec<u32>), SceneError> {
        let up = [0.0f32, 0.0, 1.0];
        let eyes = scene_count as usize * self.n;
        let mut count = vec![0u32; eyes.max(1)];
        let mut ids = vec![0u32; (eyes * width as usize).max(1)];
        check_scenes(
            unsafe {
                nb_scenes_eyes_seen(self.ctx, first_scene, scene_count, up.as_ptr(), cp.as_ptr() as *const f32, width, count.as_mut_ptr(), ids.as_mut_ptr())
            },
            self.ctx,
        )?;
        count.truncate(eyes);
        ids.truncate(eyes * width as usize);
        Ok((count, ids))
    }

    /// k `update_instance_nbody` of every scene from vision alone: every body folds the law over where its
    /// own eye sees the bodies of its own scene; asynchronous; `cp`: the eyes' perspective constant, column-major
    pub fn step_nbody_located(&mut self, k: u32, cp: &[[f32; 4]; 4], width: u32) -> Result<(), SceneError> {
        let up = [0.0f32, 0.0, 1.0];
        check_scenes(
            unsafe { nb_scenes_step_nbody_located(self.ctx, k, up.as_ptr(), cp.as_ptr() as *const f32, width) },
            self.ctx,
        )
    }

    /// the located sets that step folds over, for scenes [first_scene, first_scene + scene_count): `width` slots an eye of ids,
    /// depth, col and rel (x, y, z, range), padded with NB_EYES_NONE, 1.0, NB_EYES_NONE and +0 behind the count
    pub fn located(&mut self, first_scene: u32, scene_count: u32, cp: &[[f32; 4]; 4], width: u32) -> Result<BatchLocated, SceneError> {
        let up = [0.0f32, 0.0, 1.0];
        let eyes = scene_count as usize * self.n;
        let cells = eyes * width as usize;
        let mut l = BatchLocated {
            width,
            count: vec![0u32; eyes.max(1)],
            ids: vec![0u32; cells.max(1)],
            depth: vec![0f32; cells.max(1)],
            col: vec![0u32; cells.max(1)],
            rel: vec![[0f32; 4]; cells.max(1)],
        };
        check_scenes(
            unsafe {
                nb_scenes_eyes_located(self.ctx, first_scene, scene_count, up.as_ptr(), cp.as_ptr() as *const f32, width, l.count.as_mut_ptr(), l.ids.as_mut_ptr(), l.depth.as_mut_ptr(), l.col.as_mut_ptr(), l.rel.as_mut_ptr() as *mut f32)
            },
            self.ctx,
        )?;
        l.count.truncate(eyes);
        l.ids.truncate(cells);
        l.depth.truncate(cells);
        l.col.truncate(cells);
        l.rel.truncate(cells);
        Ok(l)
    }

    /// the batch's policies (nb_scenes_set_policy): `weights` holds 1 or `scenes` policies of policy_floats(features, hidden) floats
    /// each, scene s using policy s (or all policy 0); `accel_limit` >= 0 clamps the two outputs, f32::INFINITY: no limit
    pub fn set_policy(&mut self, weights: &[f32], features: u32, hidden: u32, accel_limit: f32) -> Result<(), SceneError> {
        let one = policy_floats(features, hidden);
        if one == 0 || weights.is_empty() || weights.len() % one != 0 {
            return Err(SceneError(-1, "weights must hold whole policies of policy_floats(features, hidden) floats".to_string())); // NB_ERR_INVALID
        }
        check_scenes(
            unsafe { nb_scenes_set_policy(self.ctx, features, hidden, (weights.len() / one) as u32, weights.as_ptr(), accel_limit) },
            self.ctx,
        )?;
        self.policy_features = features as usize;
        Ok(())
    }

    /// k steps of every scene under its policy (nb_scenes_step_policy): the pooled eye row through the two-layer network, thrust and
    /// turn along the eye's own axes; one fused launch per step.  `width` must be a multiple of the policy's features.
    pub fn step_policy(&mut self, k: u32, cp: &[[f32; 4]; 4], width: u32) -> Result<(), SceneError> {
        let up = [0.0f32, 0.0, 1.0];
        check_scenes(
            unsafe { nb_scenes_step_policy(self.ctx, k, up.as_ptr(), cp.as_ptr() as *const f32, width) },
            self.ctx,
        )
    }

    /// what that step computes in front of the actuation, for scenes [first_scene, first_scene + scene_count): per eye the policy's
    /// features and the two outputs behind the limit
    pub fn policy_observe(&mut self, first_scene: u32, scene_count: u32, cp: &[[f32; 4]; 4], width: u32) -> Result<(Vec<f32>, Vec<[f32; 2]>), SceneError> {
        let up = [0.0f32, 0.0, 1.0];
        let eyes = scene_count as usize * self.n;
        let mut feat = vec![0f32; (eyes * self.policy_features).max(1)];
        let mut act = vec![[0f32; 2]; eyes.max(1)];
        check_scenes(
            unsafe {
                nb_scenes_eyes_policy(self.ctx, first_scene, scene_count, up.as_ptr(), cp.as_ptr() as *const f32, width, feat.as_mut_ptr(), act.as_mut_ptr() as *mut f32)
            },
            self.ctx,
        )?;
        feat.truncate(eyes * self.policy_features);
        act.truncate(eyes);
        Ok((feat, act))
    }

    /// the batch's score (nb_scenes_set_score): `radius_sq` >= 0 is the squared radius below which a pair
    /// counts as near (f32::INFINITY: every pair), `goal` the point whose squared distance is summed; clears the records
    pub fn set_score(&mut self, radius_sq: f32, goal: [f32; 3]) -> Result<(), SceneError> {
        let sp = NbScoreParams { radius_sq, goal };
        check_scenes(unsafe { nb_scenes_set_score(self.ctx, &sp) }, self.ctx)
    }

    /// the current snapshot of every scene added to its record (nb_scenes_score): one kernel, asynchronous
    pub fn score(&mut self) -> Result<(), SceneError> {
        check_scenes(unsafe { nb_scenes_score(self.ctx) }, self.ctx)
    }

    /// the records cleared (nb_scenes_score_reset), asynchronous; an upload does not clear them
    pub fn score_reset(&mut self) -> Result<(), SceneError> {
        check_scenes(unsafe { nb_scenes_score_reset(self.ctx) }, self.ctx)
    }

    /// the records of scenes [first_scene, first_scene + scene_count) (nb_scenes_scores); waits for the stream
    pub fn scores(&mut self, first_scene: u32, scene_count: u32) -> Result<Vec<NbSceneScore>, SceneError> {
        let mut out = vec![NbSceneScore::default(); (scene_count as usize).max(1)];
        check_scenes(unsafe { nb_scenes_scores(self.ctx, first_scene, scene_count, out.as_mut_ptr()) }, self.ctx)?;
        out.truncate(scene_count as usize);
        Ok(out)
    }

    /// k times step_policy(1) then score() (nb_scenes_step_policy_scored): a rollout scored where it runs
    pub fn step_policy_scored(&mut self, k: u32, cp: &[[f32; 4]; 4], width: u32) -> Result<(), SceneError> {
        let up = [0.0f32, 0.0, 1.0];
        check_scenes(
            unsafe { nb_scenes_step_policy_scored(self.ctx, k, up.as_ptr(), cp.as_ptr() as *const f32, width) },
            self.ctx,
        )
    }

    /// the batch's search (nb_scenes_es_set): `mean` of policy_floats(features, hidden) floats is the policy
    /// the population -- one policy a scene, at most NB_ES_MAX_POPULATION scenes -- is drawn around; the generation starts at 0
    pub fn es_set(&mut self, features: u32, hidden: u32, mean: &[f32], accel_limit: f32, ep: &NbEsParams) -> Result<(), SceneError> {
        assert_eq!(mean.len(), policy_floats(features, hidden), "mean must hold policy_floats(features, hidden) floats");
        check_scenes(unsafe { nb_scenes_es_set(self.ctx, features, hidden, mean.as_ptr(), accel_limit, ep) }, self.ctx)?;
        self.es_floats = mean.len();
        self.policy_features = features as usize;
        Ok(())
    }

    /// the batch's policies, recurrent (nb_scenes_set_policy_recurrent): `weights` holds 1 or `scenes` policies
    /// of policy_recurrent_floats(features, hidden) floats each; every body gets `hidden` words of memory, cleared to +0 here;
    /// `memory_limit` >= 0 clamps what a step writes to it, f32::INFINITY: no limit.  step_policy, step_policy_scored and
    /// policy_observe then run the recurrent kernel until set_policy sets a feedforward policy
    pub fn set_policy_recurrent(&mut self, weights: &[f32], features: u32, hidden: u32, accel_limit: f32, memory_limit: f32) -> Result<(), SceneError> {
        let one = policy_recurrent_floats(features, hidden);
        if one == 0 || weights.is_empty() || weights.len() % one != 0 {
            return Err(SceneError(-1, "weights must hold whole policies of policy_recurrent_floats(features, hidden) floats".to_string())); // NB_ERR_INVALID
        }
        check_scenes(
            unsafe { nb_scenes_set_policy_recurrent(self.ctx, features, hidden, (weights.len() / one) as u32, weights.as_ptr(), accel_limit, memory_limit) },
            self.ctx,
        )?;
        self.policy_features = features as usize;
        self.policy_hidden = hidden as usize;
        Ok(())
    }

    /// the memory of scenes [first_scene, first_scene + scene_count) (nb_scenes_memory): n * hidden floats a scene; waits for the stream
    pub fn memory(&mut self, first_scene: u32, scene_count: u32) -> Result<Vec<f32>, SceneError> {
        let words = scene_count as usize * self.n * self.policy_hidden;
        let mut out = vec![0f32; words.max(1)];
        check_scenes(unsafe { nb_scenes_memory(self.ctx, first_scene, scene_count, out.as_mut_ptr()) }, self.ctx)?;
        out.truncate(words);
        Ok(out)
    }

    /// the memory of the whole batch from the host (nb_scenes_set_memory): scenes * n * hidden floats, any bit patterns
    pub fn set_memory(&mut self, memory: &[f32]) -> Result<(), SceneError> {
        if memory.is_empty() || memory.len() != self.scenes * self.n * self.policy_hidden {
            return Err(SceneError(-1, "memory must hold scenes * n * hidden floats".to_string())); // NB_ERR_INVALID
        }
        check_scenes(unsafe { nb_scenes_set_memory(self.ctx, memory.as_ptr()) }, self.ctx)
    }

    /// the memory of every body set to +0 (nb_scenes_memory_reset), asynchronous; an upload, keep and rewind do not touch the memory
    pub fn memory_reset(&mut self) -> Result<(), SceneError> {
        check_scenes(unsafe { nb_scenes_memory_reset(self.ctx) }, self.ctx)
    }

    /// policy_observe for a recurrent policy with the memory the step would write (nb_scenes_eyes_policy_memory), the memory left as
    /// it is: (features, outputs, next memory)
    pub fn policy_observe_memory(&mut self, first_scene: u32, scene_count: u32, cp: &[[f32; 4]; 4], width: u32) -> Result<(Vec<f32>, Vec<[f32; 2]>, Vec<f32>), SceneError> {
        let up = [0f32, 0.0, 1.0];
        let eyes = scene_count as usize * self.n;
        let mut feat = vec![0f32; (eyes * self.policy_features).max(1)];
        let mut act = vec![[0f32; 2]; eyes.max(1)];
        let mut mem = vec![0f32; (eyes * self.policy_hidden).max(1)];
        check_scenes(
            unsafe {
                nb_scenes_eyes_policy_memory(self.ctx, first_scene, scene_count, up.as_ptr(), cp.as_ptr() as *const f32, width, feat.as_mut_ptr(), act.as_mut_ptr() as *mut f32, mem.as_mut_ptr())
            },
            self.ctx,
        )?;
        feat.truncate(eyes * self.policy_features);
        act.truncate(eyes);
        mem.truncate(eyes * self.policy_hidden);
        Ok((feat, act, mem))
    }

    /// es_set over a recurrent policy (nb_scenes_es_set_recurrent): `mean` holds policy_recurrent_floats(features, hidden) floats.  A
    /// generation is rewind, memory_reset, score_reset, es_perturb, step_policy_scored, es_update: rewind does not touch the memory
    pub fn es_set_recurrent(&mut self, features: u32, hidden: u32, mean: &[f32], accel_limit: f32, memory_limit: f32, ep: &NbEsParams) -> Result<(), SceneError> {
        assert_eq!(mean.len(), policy_recurrent_floats(features, hidden), "mean must hold policy_recurrent_floats(features, hidden) floats");
        check_scenes(unsafe { nb_scenes_es_set_recurrent(self.ctx, features, hidden, mean.as_ptr(), accel_limit, memory_limit, ep) }, self.ctx)?;
        self.es_floats = mean.len();
        self.policy_features = features as usize;
        self.policy_hidden = hidden as usize;
        Ok(())
    }

    /// the batch's policies become the population of the current generation (nb_scenes_es_perturb), asynchronous
    pub fn es_perturb(&mut self) -> Result<(), SceneError> {
        check_scenes(unsafe { nb_scenes_es_perturb(self.ctx) }, self.ctx)
    }

    /// the score records ranked, the mean updated in place and the generation incremented (nb_scenes_es_update), asynchronous
    pub fn es_update(&mut self) -> Result<(), SceneError> {
        check_scenes(unsafe { nb_scenes_es_update(self.ctx) }, self.ctx)
    }

    /// the mean (nb_scenes_es_mean); waits for the stream
    pub fn es_mean(&mut self) -> Result<Vec<f32>, SceneError> {
        let mut out = vec![0.0f32; self.es_floats.max(1)];
        check_scenes(unsafe { nb_scenes_es_mean(self.ctx, out.as_mut_ptr()) }, self.ctx)?;
        out.truncate(self.es_floats);
        Ok(out)
    }

    /// what the last es_update left (nb_scenes_es_result): the report, the fitnesses and the ranks (0 the worst); waits for the stream
    pub fn es_result(&mut self) -> Result<(NbEsReport, Vec<f32>, Vec<u32>), SceneError> {
        let mut report = NbEsReport::default();
        let mut fitness = vec![0.0f32; self.scenes];
        let mut rank = vec![0u32; self.scenes];
        check_scenes(unsafe { nb_scenes_es_result(self.ctx, &mut report, fitness.as_mut_ptr(), rank.as_mut_ptr()) }, self.ctx)?;
        Ok((report, fitness, rank))
    }

    /// the generation the next es_perturb draws
    pub fn es_generation(&self) -> u32 {
        unsafe { nb_scenes_es_generation(self.ctx) }
    }

    /// positions, velocities and the step counter copied to buffers the batch keeps (nb_scenes_keep), on the device
    pub fn keep(&mut self) -> Result<(), SceneError> {
        check_scenes(unsafe { nb_scenes_keep(self.ctx) }, self.ctx)
    }

    /// the kept state copied back (nb_scenes_rewind), asynchronous
    pub fn rewind(&mut self) -> Result<(), SceneError> {
        check_scenes(unsafe { nb_scenes_rewind(self.ctx) }, self.ctx)
    }

    /// positions, velocities and model matrices of every body, scene after scene
    pub fn download(&mut self) -> Result<(Vec<Point3<f32>>, Vec<Vector3<f32>>, Vec<[[f32; 4]; 4]>), SceneError> {
        let total = self.scenes * self.n;
        let mut p = vec![Point3::new(0.0f32, 0.0, 0.0); total];
        let mut v = vec![Vector3::new(0.0f32, 0.0, 0.0); total];
        let mut m = vec![[[0.0f32; 4]; 4]; total];
        check_scenes(
            unsafe { nb_scenes_download(self.ctx, p.as_mut_ptr() as *mut f32, v.as_mut_ptr() as *mut f32, m.as_mut_ptr() as *mut f32) },
            self.ctx,
        )?;
        Ok((p, v, m))
    }

    /// device addresses of the position records, velocity records and model matrices (scene s: `s * n` records behind each)
    pub fn device_state(&mut self) -> Result<(*const c_void, *const c_void, *const c_void), SceneError> {
        let (mut p, mut v, mut m) = (std::ptr::null(), std::ptr::null(), std::ptr::null());
        check_scenes(unsafe { nb_scenes_device_state(self.ctx, &mut p, &mut v, &mut m) }, self.ctx)?;
        Ok((p, v, m))
    }

    pub fn sync(&mut self) -> Result<(), SceneError> {
        check_scenes(unsafe { nb_scenes_sync(self.ctx) }, self.ctx)
    }

    pub fn steps_done(&self) -> u64 {
        unsafe { nb_scenes_steps(self.ctx) }
    }
}

impl Drop for SceneBatch {
    fn drop(&mut self) {
        unsafe { nb_scenes_destroy(self.ctx) };
    }
}
