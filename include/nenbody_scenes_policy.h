/* nenbody_scenes_policy.h -- a neural policy over each body's eye row, for scene batches.  Included by
 * nenbody.h, which states the rule (P1-P8) in front of the include; a host includes nenbody.h.  These are additions to ABI version 2:
 * a library that exports them exports everything nenbody.h declares. */
#ifndef NENBODY_SCENES_POLICY_H
#define NENBODY_SCENES_POLICY_H

#include "nenbody.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The floats of one policy of shape (features, hidden): features*hidden + hidden + 2*hidden + 2.  Host arithmetic; 0 for a shape
 * outside 1 <= features <= NB_POLICY_MAX_FEATURES, 1 <= hidden <= NB_POLICY_MAX_HIDDEN. */
size_t nb_policy_floats(uint32_t features, uint32_t hidden);
/* ONE step of a batch on caller-owned device memory, out of place, one kernel on `stream`.  cams_16, inst_16: 16 floats per body for
 * the scenes*n bodies, as nb_launch_cameras and nb_launch_instances leave them with count = scenes*n.  up_xyz (3 floats) is host
 * memory: the `up` the cameras were formed with.  weights: device memory, 4-byte aligned, policies * nb_policy_floats(features,
 * hidden) floats; policies is 1 or scenes.  accel_limit >= 0 (+inf: none).  pos_in, vel_in, pos_out, vel_out: scenes*n records each;
 * every record and matrix pointer 16-byte aligned; no output may overlap an input or the other output.  params == NULL -> defaults;
 * dt is used, the rest is validated. */
int nb_scenes_policy_step_launch(const nb_params *params, uint32_t scenes, uint32_t n, const void *cams_16, const void *inst_16,
                                 uint32_t width, const float *up_xyz, uint32_t features, uint32_t hidden, uint32_t policies,
                                 const void *weights, float accel_limit, const void *pos_in, const void *vel_in, void *pos_out,
                                 void *vel_out, void *stream);
/* P8 for eyes [first_eye, first_eye + count) of the batch (eye s*n + i is body i of scene s), one kernel on `stream`: feat_out,
 * count*features words of x; act_out, count*2 words of o behind the limit; device memory, 4-byte aligned; either may be NULL, not
 * both.  Every word of every output that is passed is written.  cams_16, inst_16 and weights as above, for the WHOLE batch.
 * count = 0 is a checked no-op. */
int nb_scenes_policy_observe_launch(uint32_t scenes, uint32_t n, uint32_t first_eye, uint32_t count, const void *cams_16,
                                    const void *inst_16, uint32_t width, uint32_t features, uint32_t hidden, uint32_t policies,
                                    const void *weights, float accel_limit, void *feat_out, void *act_out, void *stream);
/* The context's policies: policies * nb_policy_floats(features, hidden) host floats, copied to a buffer the context owns (the host
 * array is not retained).  policies is 1 or the context's scenes.  May be called again, before or after an upload. */
int nb_scenes_set_policy(nb_scenes *ctx, uint32_t features, uint32_t hidden, uint32_t policies, const float *weights_host,
                         float accel_limit);
/* k such steps of every scene with the context's dt, asynchronous on the context's stream; mixes freely with the other steps.  Per
 * step: the model matrices and the eye cameras of all bodies, the fused kernel into a second pair of record buffers, the swap.
 * NB_ERR_STATE before an upload or before a policy is set.  width must be a multiple of the policy's features.  k = 0 is a checked
 * no-op. */
int nb_scenes_step_policy(nb_scenes *ctx, uint32_t k, const float *up_xyz, const float *cp16, uint32_t width);
/* P8 for scenes [first_scene, first_scene + scene_count) of the current state, to the host: feat, scene_count*n*features floats;
 * act, scene_count*n*2 floats; either may be NULL, not both.  Waits for the result. */
int nb_scenes_eyes_policy(nb_scenes *ctx, uint32_t first_scene, uint32_t scene_count, const float *up_xyz, const float *cp16,
                          uint32_t width, float *feat, float *act);

#ifdef __cplusplus
}
#endif
#endif /* NENBODY_SCENES_POLICY_H */
