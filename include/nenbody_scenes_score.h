/* nenbody_scenes_score.h -- the score of scene batches.  Included by nenbody.h, which states the rule
 * (Q1-Q7) and declares nb_score_params and nb_scene_score in front of the include; a host includes nenbody.h.  These are additions to
 * ABI version 2: a library that exports them exports everything nenbody.h declares. */
#ifndef NENBODY_SCENES_SCORE_H
#define NENBODY_SCENES_SCORE_H

#include "nenbody.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The snapshot of every scene of a batch on caller-owned device memory scored into `score`, one kernel on `stream`.  pos, vel:
 * scenes*n records each, 16-byte aligned, read only.  score: scenes records of nb_scene_score in device memory, 8-byte aligned, clear
 * of pos and vel; every record is read, takes the snapshot's terms (Q7) and is written.  Clearing is the caller's memset: all-zero
 * bytes are the cleared state.  sp: host memory; NULL is NB_ERR_INVALID.  Stateless. */
int nb_scenes_score_launch(const nb_score_params *sp, uint32_t scenes, uint32_t n, const void *pos, const void *vel, void *score,
                           void *stream);
/* The context's score: the parameters are stored, the context's `scenes` records are allocated on first use and cleared.  Waits for
 * the stream first.  May be called again, before or after an upload. */
int nb_scenes_set_score(nb_scenes *ctx, const nb_score_params *sp);
/* The current snapshot of every scene scored into the context's records, asynchronous on the context's stream; mixes freely with
 * every step.  NB_ERR_STATE before an upload or before nb_scenes_set_score. */
int nb_scenes_score(nb_scenes *ctx);
/* The context's records cleared, asynchronous on the context's stream.  (An upload does not clear them.)  NB_ERR_STATE before
 * nb_scenes_set_score. */
int nb_scenes_score_reset(nb_scenes *ctx);
/* The records of scenes [first_scene, first_scene + scene_count) to the host; waits for the stream.  scene_count = 0 is a checked
 * no-op.  NB_ERR_STATE before nb_scenes_set_score. */
int nb_scenes_scores(nb_scenes *ctx, uint32_t first_scene, uint32_t scene_count, nb_scene_score *out_host);
/* k times: the policy step exactly as nb_scenes_step_policy issues it, then the score of the new snapshot; asynchronous on the
 * context's stream.  The checks of nb_scenes_step_policy, then NB_ERR_STATE before nb_scenes_set_score.  k = 0 is a checked no-op. */
int nb_scenes_step_policy_scored(nb_scenes *ctx, uint32_t k, const float *up_xyz, const float *cp16, uint32_t width);

#ifdef __cplusplus
}
#endif
#endif /* NENBODY_SCENES_SCORE_H */
