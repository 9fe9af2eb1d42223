/* nenbody_scenes_located.h -- gravity from located vision, for scene batches.  Included by nenbody.h, which
 * states the rule (SL1-SL5) in front of the include; a host includes nenbody.h.  These are additions to ABI version 2: a library
 * that exports them exports everything nenbody.h declares. */
#ifndef NENBODY_SCENES_LOCATED_H
#define NENBODY_SCENES_LOCATED_H

#include "nenbody.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ONE step of a batch on caller-owned device memory, out of place, one kernel on `stream`.  cams_16, inst_16: 16 floats per body for
 * the scenes*n bodies, as nb_launch_cameras and nb_launch_instances leave them with count = scenes*n.  up_xyz (3 floats) and cp16
 * (16 floats) are host memory: the eye set-up the cameras were formed with, cp16 invertible (SL5).  pos_in, vel_in, pos_out,
 * vel_out: scenes*n records each; every device pointer 16-byte aligned; no output may overlap an input or the other output.
 * params == NULL -> defaults; dt, G and bias are used. */
int nb_scenes_nbody_located_step_launch(const nb_params *params, uint32_t scenes, uint32_t n, const void *cams_16, const void *inst_16,
                                        const float *up_xyz, const float *cp16, uint32_t width, const void *pos_in, const void *vel_in,
                                        void *pos_out, void *vel_out, void *stream);
/* SL3 for eyes [first_eye, first_eye + count) of the batch (eye s*n + i is body i of scene s), one kernel on `stream`: seen_count,
 * count words; seen_ids, seen_depth and seen_col, count*width words each; seen_rel, count*width records of 16 bytes; device memory,
 * 4-byte aligned (seen_rel: 16); any may be NULL, not all.  Every word of every output that is passed is written.  cams_16 and
 * inst_16 as above and vel_in, the batch's velocity records, for the WHOLE batch (eye b reads camera b and record b).  count = 0 is
 * a checked no-op. */
int nb_scenes_located_launch(uint32_t scenes, uint32_t n, uint32_t first_eye, uint32_t count, const void *cams_16, const void *inst_16,
                             const void *vel_in, const float *up_xyz, const float *cp16, uint32_t width, void *seen_count, void *seen_ids,
                             void *seen_depth, void *seen_col, void *seen_rel, void *stream);
/* k such steps of every scene with the context's dt, G and bias, asynchronous on the context's stream; mixes freely with
 * nb_scenes_step, nb_scenes_step_boids and nb_scenes_step_boids_seen.  Per step: the model matrices and the eye cameras of all
 * bodies, the fused kernel into a second pair of record buffers, the swap.  NB_ERR_STATE before an upload.  k = 0 is a checked
 * no-op. */
int nb_scenes_step_nbody_located(nb_scenes *ctx, uint32_t k, const float *up_xyz, const float *cp16, uint32_t width);
/* SL3 for scenes [first_scene, first_scene + scene_count) of the current state, to the host: seen_count, scene_count*n words;
 * seen_ids, seen_depth, seen_col, scene_count*n*width words each; seen_rel, scene_count*n*width*4 floats; any may be NULL, not
 * all.  Waits for the result. */
int nb_scenes_eyes_located(nb_scenes *ctx, uint32_t first_scene, uint32_t scene_count, const float *up_xyz, const float *cp16,
                           uint32_t width, uint32_t *seen_count, uint32_t *seen_ids, float *seen_depth, uint32_t *seen_col, float *seen_rel);

#ifdef __cplusplus
}
#endif
#endif /* NENBODY_SCENES_LOCATED_H */
