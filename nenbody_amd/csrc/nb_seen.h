// nb_seen.h -- launchers of the seen-set kernel and of the boids fold over seen lists (nb_seen.inc, compiled in the SLP-off unit of
// nb_kernels.hip), for the C ABI (nb_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nb_kernels.h"

namespace nbk {

// The seen set of every eye from its resolved row: ids_rows / depth_rows hold count x width words as
// launch_eyes leaves them (depth_rows may be NULL: seen_depth must then be NULL too); seen_count: count words; seen_ids, seen_depth,
// seen_cols: count x width words each, the last two may be NULL.  The caller has checked the arguments (1 <= width <=
// NB_EYES_MAX_WIDTH, count >= 1).
hipError_t launch_seen(uint32_t count, uint32_t width, const uint32_t *ids_rows, const float *depth_rows, uint32_t *seen_count,
                       uint32_t *seen_ids, float *seen_depth, uint32_t *seen_cols, hipStream_t s);

// One boids step (V2-V3) for bodies [a.first, a.first + a.count): body a.first + e folds over the first seen_count[e] entries (at most
// `stride`) of seen_ids[e * stride ..], in list order.  a as make_boids_args leaves it, with the four record pointers set.
hipError_t launch_boids_seen(const BoidsArgs &a, const uint32_t *seen_count, const uint32_t *seen_ids, uint32_t stride, hipStream_t s);

}  // namespace nbk
