/* nenbody_scenes_seen.h -- the boids step over what each body sees, for scene batches.  Included by
 * nenbody.h, which states the rule (SV1-SV4) in front of the include; a host includes nenbody.h.  These are additions to ABI
 * version 2: a library that exports them exports everything nenbody.h declares. */
#ifndef NENBODY_SCENES_SEEN_H
#define NENBODY_SCENES_SEEN_H

#include "nenbody.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ONE step of a batch on caller-owned device memory, out of place, one kernel on `stream`.  cams_16, inst_16: 16 floats per body for
 * the scenes*n bodies, as nb_launch_cameras and nb_launch_instances leave them with count = scenes*n (both are per body, so they
 * serve a batch as they are).  pos_in, vel_in, pos_out, vel_out: scenes*n records each; everything 16-byte aligned; no output may
 * overlap an input or the other output.  params == NULL -> defaults. */
int nb_scenes_boids_seen_step_launch(const nb_boids_params *params, uint32_t scenes, uint32_t n, const void *cams_16, const void *inst_16,
                                     uint32_t width, const void *pos_in, const void *vel_in, void *pos_out, void *vel_out, void *stream);
/* SV3 for eyes [first_eye, first_eye + count) of the batch (eye s*n + i is body i of scene s), one kernel on `stream`: seen_count,
 * count words; seen_ids, count*width words; device memory, 4-byte aligned; either may be NULL, not both.  cams_16 and inst_16 as
 * above, for the WHOLE batch (eye b reads camera b).  count = 0 is a checked no-op. */
int nb_scenes_seen_launch(uint32_t scenes, uint32_t n, uint32_t first_eye, uint32_t count, const void *cams_16, const void *inst_16,
                          uint32_t width, void *seen_count, void *seen_ids, void *stream);
/* k such steps of every scene, asynchronous on the context's stream; mixes freely with nb_scenes_step / nb_scenes_step_boids.  Per
 * step: the model matrices and the eye cameras of all bodies, the fused kernel into a second pair of record buffers, the swap
 * (nb_scenes_device_state and nb_scenes_download see the current pair).  NB_ERR_STATE before an upload.  k = 0 is a checked no-op. */
int nb_scenes_step_boids_seen(nb_scenes *ctx, uint32_t k, const nb_boids_params *params, const float *up_xyz, const float *cp16,
                              uint32_t width);
/* SV3 for scenes [first_scene, first_scene + scene_count) of the current state, to the host: seen_count, scene_count*n words;
 * seen_ids, scene_count*n*width words; either may be NULL, not both.  Waits for the result. */
int nb_scenes_eyes_seen(nb_scenes *ctx, uint32_t first_scene, uint32_t scene_count, const float *up_xyz, const float *cp16, uint32_t width,
                        uint32_t *seen_count, uint32_t *seen_ids);

#ifdef __cplusplus
}
#endif
#endif /* NENBODY_SCENES_SEEN_H */
