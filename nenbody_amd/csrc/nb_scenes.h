// nb_scenes.h -- launchers of the scene-batch kernels (nb_scenes.inc, compiled in the SLP-off unit of nb_kernels.hip), for the C ABI
// (nb_scenes_api.inc).  A scene batch is `scenes` independent scenes of n <= kScenesMaxBodies bodies; body i of scene s is record
// s * n + i.  One launch steps every scene k times, one workgroup per scene, the scene's state on chip between the steps
// (DESIGN.md section 14).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nb_kernels.h"

namespace nbk {

constexpr uint32_t kScenesMaxBodies = 2048;   // NB_SCENES_MAX_BODIES: two bodies per lane of a 1024-lane workgroup
constexpr uint32_t kScenesMaxGrid = 2048;     // workgroups per launch; more scenes than that are walked by a grid-stride loop

// k >= 1 gravity steps (update_instance_nbody, STRICT) of every scene, in place.  The caller has checked the arguments.
struct ScenesNbodyArgs {
    float4 *pos, *vel;           // scenes * n records each, read at the start and written after step k
    uint32_t scenes, n, k;
    float dt, G, bias;           // main.rs:411-413
    uint32_t lo_bits, hi_bits;   // the divide guard's range, as StepArgs carries it
    uint32_t force_ieee;         // 1 = always the IEEE '/'
    uint32_t force_3d;           // 2 = never the planar shortcut
};
hipError_t launch_scenes_nbody(const ScenesNbodyArgs &a, hipStream_t s);

// k >= 1 boids steps (update_instance_boids) of every scene, in place.  `c`: the constants of a set of n bodies (n_total = count = n,
// first = 0) as make_boids_args forms them; its four buffer pointers are not read.
hipError_t launch_scenes_boids(const BoidsArgs &c, float4 *pos, float4 *vel, uint32_t scenes, uint32_t k, hipStream_t s);

// The seen boids step of a batch (nb_scenes_seen.inc): one workgroup per eye, the eye's row and its seen set
// in LDS only.  A scene of at most kScenesSeenWaveBodies bodies takes one wave per eye, a larger one four; the bits are the same.
constexpr uint32_t kScenesSeenWaveBodies = 128;
// The eyes a one-workgroup-per-eye scenes kernel walks, the head of its arguments (scenes_eye_begin, nb_scenes_seen.inc).
struct ScenesEyes {
    uint32_t n, first_eye, count, width;     // eyes [first_eye, first_eye + count) of the batch; eye b is body b % n of scene b / n
    const float4 *__restrict__ cams;         // 4 / 4 float4 per body of the WHOLE batch, as launch_cameras / launch_instances leave them
    const float4 *__restrict__ inst;
};
struct ScenesSeenArgs {                       // the launchers'; the kernel keeps a loose parameter list
    ScenesEyes eye;
    BoidsArgs c;                             // the step's: the constants of a set of n bodies as make_boids_args forms them (n_total = n,
                                             // first = 0), the four record pointers set to the batch's scenes * n records
    uint32_t *__restrict__ seen_count;       // the sets' (S1-S3): count words, and count x width words; either may be NULL
    uint32_t *__restrict__ seen_ids;
};
// ONE step, out of place, for every eye the arguments name (the entries pass the whole batch).
hipError_t launch_scenes_boids_seen(const ScenesSeenArgs &a, hipStream_t s);
// The seen sets that step folds over, indexed from first_eye; `c` is not read.
hipError_t launch_scenes_seen(const ScenesSeenArgs &a, hipStream_t s);

// Gravity from located vision for a batch (nb_scenes_located.inc): one workgroup per eye, the eye's row, its
// members' nearest depths and columns and the quotients in LDS only -- 8 width + 12 n + 256 bytes, at most 57 600.  The launch shape
// follows kScenesSeenWaveBodies as above; the bits are the same.  The caller has checked the arguments (1 <= n <= kScenesMaxBodies,
// 1 <= width <= NB_EYES_MAX_WIDTH, count >= 1, a constant that L2 inverts: L6).
struct ScenesLocatedArgs {
    ScenesEyes eye;
    const float4 *__restrict__ pos_in;       // the batch's records; the step reads both, the sets vel_in alone (the eye's direction)
    const float4 *__restrict__ vel_in;
    float ux, uy, uz;
    float cp0, cp10, cp14;
    float dt, G, bias;                       // main.rs:411-413; the step's
    float4 *__restrict__ pos_out;            // the step's: record b written
    float4 *__restrict__ vel_out;
    uint32_t *__restrict__ seen_count;       // the sets' (SL3): count words, and count x width words or records; any may be NULL
    uint32_t *__restrict__ seen_ids;
    uint32_t *__restrict__ seen_depth;       // bit patterns
    uint32_t *__restrict__ seen_col;
    float4 *__restrict__ seen_rel;
};
// ONE step, out of place, for every eye the arguments name (the entries pass the whole batch).
hipError_t launch_scenes_nbody_located(const ScenesLocatedArgs &a, hipStream_t s);
// The located sets that step folds over: the words nb_eyes_located gives a context holding the eye's scene, indexed from first_eye.
hipError_t launch_scenes_located(const ScenesLocatedArgs &a, hipStream_t s);

// A neural policy over each body's eye row (nb_scenes_policy.inc): one workgroup per eye, the eye's row, its
// pooled features and the hidden layer in LDS only -- 8 width + 4 features + 4 hidden bytes, at most 34 048.  The launch shape follows
// kScenesSeenWaveBodies as above; the bits are the same.  The caller has checked the arguments (1 <= n <= kScenesMaxBodies,
// 1 <= width <= NB_EYES_MAX_WIDTH, count >= 1, 1 <= features <= kPolicyMaxFeatures dividing width, 1 <= hidden <= kPolicyMaxHidden,
// limit >= 0).
constexpr uint32_t kPolicyMaxFeatures = 256;  // NB_POLICY_MAX_FEATURES
constexpr uint32_t kPolicyMaxHidden = 64;     // NB_POLICY_MAX_HIDDEN: one lane per hidden unit of a 64-lane workgroup
// the floats of one policy: w1[f H + j], b1[j], w2[k H + j] (k = 0, 1), b2[k]
constexpr size_t policy_floats(uint32_t features, uint32_t hidden) { return (size_t)features * hidden + hidden + 2u * (size_t)hidden + 2u; }
struct ScenesPolicyArgs {
    ScenesEyes eye;
    uint32_t features, hidden;               // the policy shape (F, H)
    uint32_t stride;                         // floats from scene s's policy to scene s + 1's: policy_floats, or 0 where all share policy 0
    const float *__restrict__ weights;
    float limit;                             // L >= 0; +inf: none
    const float4 *__restrict__ pos_in;       // the step's: the batch's records
    const float4 *__restrict__ vel_in;
    float ux, uy, uz;
    float dt;                                // main.rs:411
    float4 *__restrict__ pos_out;            // the step's: record b written
    float4 *__restrict__ vel_out;
    uint32_t *__restrict__ feat_out;         // the observable's (P8): count x features words of x, count x 2 words of o; either may be NULL
    uint32_t *__restrict__ act_out;
};
// ONE step, out of place, for every eye the arguments name (the entries pass the whole batch).
hipError_t launch_scenes_policy(const ScenesPolicyArgs &a, hipStream_t s);
// What that step computes per eye in front of the actuation: the features and the limited outputs, indexed from first_eye.
hipError_t launch_scenes_policy_observe(const ScenesPolicyArgs &a, hipStream_t s);

// The recurrent policy (nb_scenes_policy_recurrent.inc): the policy above with H words of memory per body in
// device memory -- 8 width + 4 features + 8 hidden bytes of LDS, at most 34 304.  The caller has checked what the policy above asks
// and mem_limit >= 0.
// the floats of one recurrent policy: w1[f H + j], wr[r H + j], b1[j], w2[k H + j] (k = 0, 1), b2[k]
constexpr size_t policy_recurrent_floats(uint32_t features, uint32_t hidden) { return policy_floats(features, hidden) + (size_t)hidden * hidden; }
struct ScenesPolicyRecurrentArgs {
    ScenesPolicyArgs p;                      // as above; stride is policy_recurrent_floats, or 0
    float mem_limit;                         // S >= 0; +inf: none
    const float *mem_in;                     // the WHOLE batch's memory, body b at b * hidden: read for the eyes the arguments name
    float *mem_out;                          // the step's: written at b * hidden; may be mem_in itself
    uint32_t *mem_obs;                       // the observable's (R8): count x hidden words of m', indexed from first_eye; may be NULL
};
// ONE step for every eye the arguments name (the entries pass the whole batch): records out of place, the memory in place or not.
hipError_t launch_scenes_policy_recurrent(const ScenesPolicyRecurrentArgs &a, hipStream_t s);
// What that step computes per eye in front of the actuation, the memory left as it is.
hipError_t launch_scenes_policy_recurrent_observe(const ScenesPolicyRecurrentArgs &a, hipStream_t s);

// The score of a batch (nb_scenes_score.inc): one workgroup per scene in launch_scenes_nbody's shape, the
// scene's positions and the partial sums in LDS -- 16 n + 32 LANES + 32 bytes, 65 568 at n = 2 048.  Every scene's record takes the
// metrics of its current snapshot (Q1-Q7).  The caller has checked the arguments (scenes >= 1, 1 <= n <= kScenesMaxBodies,
// radius_sq >= 0, a finite goal, score clear of pos and vel).
struct SceneScore {                          // nb_scene_score
    uint64_t near;
    float spread, speed2, momentum2, goal2;
    uint32_t steps, nonfinite;
};
struct ScenesScoreArgs {
    const float4 *__restrict__ pos;          // scenes * n records each, read only
    const float4 *__restrict__ vel;
    SceneScore *__restrict__ score;          // scenes records, read, updated and written
    uint32_t scenes, n;
    float radius_sq;                         // Q2
    float gx, gy, gz;                        // Q5
};
hipError_t launch_scenes_score(const ScenesScoreArgs &a, hipStream_t s);

// One evolution-strategies generation over a batch (nb_scenes_es.inc): the population of a generation
// drawn from a mean, the score records ranked, the mean updated.  The caller has checked the arguments (1 <= scenes <=
// kEsMaxPopulation, m = policy_floats of a valid shape, sigma >= 0 and finite, step and the coefficients finite).
constexpr uint32_t kEsMaxPopulation = 4096;   // NB_ES_MAX_POPULATION: the keys and counts of one ranking workgroup fit the default LDS
struct EsArgs {
    uint64_t seed;
    uint32_t g;                              // the generation
    uint32_t scenes, m;                      // B (the perturb kernel does not read it: E8) and M
    float sigma, step;
    float c0, c1, c2, c3, c4, c5;            // E4's coefficients, in the order of the fields
};
// theta of scenes [first, first + count), count >= 1, first + count <= kEsMaxPopulation: count * m floats
hipError_t launch_es_perturb(const EsArgs &a, uint32_t first, uint32_t count, const float *mean, float *theta, hipStream_t s);
// E4-E5 in ONE workgroup: rank, a.scenes words; fitness, as many floats, or NULL; report, the four words of nb_es_report, or NULL
hipError_t launch_es_rank(const EsArgs &a, const SceneScore *score, uint32_t *rank, float *fitness, uint32_t *report, hipStream_t s);
// E6-E7 from the ranks: mean_out may be mean_in itself
hipError_t launch_es_update(const EsArgs &a, const uint32_t *rank, const float *mean_in, float *mean_out, hipStream_t s);

}  // namespace nbk
