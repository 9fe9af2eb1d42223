/* nenbody_scenes_policy_recurrent.h -- a recurrent policy with per-body memory, for scene batches.  Included
 * by nenbody.h, which states the rule (R1-R8) in front of the include; a host includes nenbody.h.  These are additions to ABI
 * version 2: a library that exports them exports everything nenbody.h declares. */
#ifndef NENBODY_SCENES_POLICY_RECURRENT_H
#define NENBODY_SCENES_POLICY_RECURRENT_H

#include "nenbody.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The floats of one recurrent policy of shape (features, hidden): features*hidden + hidden*hidden + hidden + 2*hidden + 2 (R1).  Host
 * arithmetic; 0 for a shape outside 1 <= features <= NB_POLICY_MAX_FEATURES, 1 <= hidden <= NB_POLICY_MAX_HIDDEN. */
size_t nb_policy_recurrent_floats(uint32_t features, uint32_t hidden);
/* ONE step of a batch on caller-owned device memory, one kernel on `stream`: nb_scenes_policy_step_launch with a memory.  weights:
 * policies * nb_policy_recurrent_floats(features, hidden) floats.  memory_limit >= 0 (+inf: none) is R4's S.  mem_in, mem_out: device
 * memory, 4-byte aligned, scenes*n*hidden floats each, body s*n + i at (s*n + i)*hidden.  mem_out may be mem_in itself (in place) or
 * clear of it; a partial overlap is refused.  Neither may overlap the weights, the records or the matrices.  Everything else as
 * nb_scenes_policy_step_launch takes it: the records are stepped out of place. */
int nb_scenes_policy_recurrent_step_launch(const nb_params *params, uint32_t scenes, uint32_t n, const void *cams_16, const void *inst_16,
                                           uint32_t width, const float *up_xyz, uint32_t features, uint32_t hidden, uint32_t policies,
                                           const void *weights, float accel_limit, float memory_limit, const void *pos_in,
                                           const void *vel_in, const void *mem_in, void *pos_out, void *vel_out, void *mem_out,
                                           void *stream);
/* R8 for eyes [first_eye, first_eye + count) of the batch, which may begin and end inside a scene; one kernel on `stream`.  mem: the
 * memory of the WHOLE batch, scenes*n*hidden floats, read only and left as it is.  feat_out, count*features words of x; act_out,
 * count*2 words of o behind the limit; mem_out, count*hidden words of m', eye first_eye + e at e*hidden, clear of mem.  Device
 * memory, 4-byte aligned; any output may be NULL, not all three.  Every word of every output that is passed is written.
 * count = 0 is a checked no-op. */
int nb_scenes_policy_recurrent_observe_launch(uint32_t scenes, uint32_t n, uint32_t first_eye, uint32_t count, const void *cams_16,
                                              const void *inst_16, uint32_t width, uint32_t features, uint32_t hidden, uint32_t policies,
                                              const void *weights, float accel_limit, float memory_limit, const void *mem, void *feat_out,
                                              void *act_out, void *mem_out, void *stream);
/* nb_scenes_es_perturb_launch and nb_scenes_es_update_launch (nenbody_scenes_es.h) for a mean of any length M = floats,
 * 1 <= floats <= NB_ES_MAX_FLOATS: E1-E8 depend on the weight index alone, so the kernels are the same.  With
 * floats = nb_policy_floats(features, hidden) the words are those of the shape launches. */
int nb_scenes_es_perturb_floats_launch(const nb_es_params *ep, uint32_t floats, uint32_t generation, uint32_t first_scene, uint32_t count,
                                       const void *mean, void *theta_out, void *stream);
int nb_scenes_es_update_floats_launch(const nb_es_params *ep, uint32_t floats, uint32_t generation, uint32_t scenes, const void *score,
                                      const void *mean, void *mean_out, void *rank_out, void *fitness_out, void *report_out, void *stream);
/* The context's policies, recurrent: as nb_scenes_set_policy, with policies * nb_policy_recurrent_floats(features, hidden) host
 * floats and R4's memory_limit.  It also reserves the context's memory (scenes*n*hidden floats) and clears it to +0.  From here on
 * nb_scenes_step_policy, nb_scenes_step_policy_scored and nb_scenes_eyes_policy run the recurrent kernel, the steps updating the
 * memory in place; a later nb_scenes_set_policy returns the context to the feedforward kernel. */
int nb_scenes_set_policy_recurrent(nb_scenes *ctx, uint32_t features, uint32_t hidden, uint32_t policies, const float *weights_host,
                                   float accel_limit, float memory_limit);
/* R8 for scenes [first_scene, first_scene + scene_count) of the current state and memory, to the host: feat and act as
 * nb_scenes_eyes_policy gives them; mem_next, scene_count*n*hidden floats of m'.  Any may be NULL, not all three.  The memory is
 * not changed.  Waits for the result.  NB_ERR_STATE unless the policy that is set is recurrent. */
int nb_scenes_eyes_policy_memory(nb_scenes *ctx, uint32_t first_scene, uint32_t scene_count, const float *up_xyz, const float *cp16,
                                 uint32_t width, float *feat, float *act, float *mem_next);
/* The memory of every body set to +0: a memset, asynchronous on the context's stream.  NB_ERR_STATE unless the policy that is set is
 * recurrent, as for the two entries below. */
int nb_scenes_memory_reset(nb_scenes *ctx);
/* The memory of scenes [first_scene, first_scene + scene_count) to the host, scene_count*n*hidden floats; waits for the stream. */
int nb_scenes_memory(nb_scenes *ctx, uint32_t first_scene, uint32_t scene_count, float *out_host);
/* The memory of the whole batch from the host, scenes*n*hidden floats of any bit patterns; waits for the stream first and for the
 * copy behind (the host array is not retained). */
int nb_scenes_set_memory(nb_scenes *ctx, const float *mem_host);
/* The context's search over a recurrent policy: as nb_scenes_es_set with M = nb_policy_recurrent_floats(features, hidden) and R4's
 * memory_limit.  nb_scenes_es_perturb, nb_scenes_es_update and nb_scenes_es_mean use that M; nb_scenes_es_perturb makes the
 * context's policy recurrent and reserves (and then clears) the memory if the context has none of that size yet. */
int nb_scenes_es_set_recurrent(nb_scenes *ctx, uint32_t features, uint32_t hidden, const float *mean_host, float accel_limit,
                               float memory_limit, const nb_es_params *ep);

#ifdef __cplusplus
}
#endif
#endif /* NENBODY_SCENES_POLICY_RECURRENT_H */
