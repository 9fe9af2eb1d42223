/* nenbody_scenes_es.h -- an evolution-strategies generation over a scene batch.  Included by nenbody.h,
 * which states the rule (E1-E8) and declares nb_es_params and nb_es_report in front of the include; a host includes nenbody.h.
 * These are additions to ABI version 2: a library that exports them exports everything nenbody.h declares. */
#ifndef NENBODY_SCENES_ES_H
#define NENBODY_SCENES_ES_H

#include "nenbody.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The population of generation `generation` for scenes [first_scene, first_scene + count) (E1-E3), one kernel on `stream`.  mean:
 * M = nb_policy_floats(features, hidden) floats in device memory, read only.  theta_out: count * M floats in device memory, scene
 * first_scene + i at i * M, clear of mean; both 4-byte aligned.  first_scene + count <= NB_ES_MAX_POPULATION; count = 0 is a checked
 * no-op.  ep: host memory; NULL is NB_ERR_INVALID.  Stateless; theta of a scene does not depend on the range it is asked in (E8). */
int nb_scenes_es_perturb_launch(const nb_es_params *ep, uint32_t features, uint32_t hidden, uint32_t generation, uint32_t first_scene,
                                uint32_t count, const void *mean, void *theta_out, void *stream);
/* The records of a rollout ranked and the mean updated (E4-E7), two kernels on `stream`.  score: scenes records of nb_scene_score in
 * device memory, 8-byte aligned, read only.  mean: M floats, read.  mean_out: M floats, written: mean itself (in place) or memory
 * clear of it.  rank_out: scenes words, required: the second kernel reads it.  fitness_out: scenes floats, or NULL.  report_out: one
 * nb_es_report, or NULL.  All of these 4-byte aligned device memory; no output may overlap another or an input.
 * 1 <= scenes <= NB_ES_MAX_POPULATION.  Stateless. */
int nb_scenes_es_update_launch(const nb_es_params *ep, uint32_t features, uint32_t hidden, uint32_t generation, uint32_t scenes,
                               const void *score, const void *mean, void *mean_out, void *rank_out, void *fitness_out, void *report_out,
                               void *stream);
/* The context's search: the policy shape, the limit of the policies' outputs and the parameters are stored, mean_host (M floats) is
 * uploaded to a buffer the context owns, and the generation is set to 0.  Waits for the stream first.  A context of more than
 * NB_ES_MAX_POPULATION scenes is NB_ERR_INVALID.  May be called again. */
int nb_scenes_es_set(nb_scenes *ctx, uint32_t features, uint32_t hidden, const float *mean_host, float accel_limit, const nb_es_params *ep);
/* The context's policies become the population of the current generation, one policy a scene, with the shape and the limit of
 * nb_scenes_es_set: what nb_scenes_set_policy had set is overwritten.  Asynchronous on the context's stream.  NB_ERR_STATE before
 * nb_scenes_es_set. */
int nb_scenes_es_perturb(nb_scenes *ctx);
/* The context's score records ranked, the mean updated in place and the generation incremented.  Asynchronous on the context's
 * stream.  NB_ERR_STATE before nb_scenes_es_set and before nb_scenes_set_score. */
int nb_scenes_es_update(nb_scenes *ctx);
/* The mean (M floats) to the host; waits for the stream.  NB_ERR_STATE before nb_scenes_es_set. */
int nb_scenes_es_mean(nb_scenes *ctx, float *out_host);
/* What the last nb_scenes_es_update left: the report, the fitnesses (scenes floats) and the ranks (scenes words) to the host; waits
 * for the stream.  Any pointer may be NULL.  NB_ERR_STATE before the first nb_scenes_es_update behind an nb_scenes_es_set. */
int nb_scenes_es_result(nb_scenes *ctx, nb_es_report *report, float *fitness, uint32_t *rank);
/* The generation the next nb_scenes_es_perturb draws: the updates since nb_scenes_es_set, modulo 2^32.  0 for a NULL context. */
uint32_t nb_scenes_es_generation(const nb_scenes *ctx);
/* The current state -- positions, velocities and the step counter -- copied to buffers the context keeps, device to device,
 * asynchronous on the context's stream.  An upload does not drop the kept state.  NB_ERR_STATE before an upload. */
int nb_scenes_keep(nb_scenes *ctx);
/* The kept state copied back, asynchronous on the context's stream.  NB_ERR_STATE before nb_scenes_keep. */
int nb_scenes_rewind(nb_scenes *ctx);

#ifdef __cplusplus
}
#endif
#endif /* NENBODY_SCENES_ES_H */
