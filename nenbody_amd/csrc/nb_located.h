// nb_located.h -- launchers of the located-set kernel and of the gravity fold over located lists (nb_located.inc, compiled in the
// SLP-off unit of nb_kernels.hip), for the C ABI (nb_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nb_kernels.h"

namespace nbk {

// The located seen set of every eye.  ids_rows / depth_rows: count x width words as launch_eyes leaves
// them; seen_count: count words, seen_ids / seen_depth: count x width words as launch_seen leaves them for those rows; dirs: count
// direction records; seen_col (may be NULL): count x width words, seen_rel: count x width records.  The caller has checked the
// arguments (1 <= width <= NB_EYES_MAX_WIDTH, count >= 1, a constant that L2 inverts: L6).
struct LocatedArgs {
    uint32_t count, width;
    const uint32_t *__restrict__ ids_rows;
    const uint32_t *__restrict__ depth_rows;   // bit patterns
    const uint32_t *__restrict__ seen_count;
    const uint32_t *__restrict__ seen_ids;
    const uint32_t *__restrict__ seen_depth;   // bit patterns
    const float4 *__restrict__ dirs;
    float ux, uy, uz;
    float cp0, cp10, cp14;
    uint32_t *__restrict__ seen_col;
    float4 *__restrict__ seen_rel;
};
hipError_t launch_located(const LocatedArgs &a, hipStream_t s);

// One gravity step (G2-G3) for bodies [first, first + count): body first + e folds over the first seen_count[e] records (at most
// `stride`) of seen_rel[e * stride ..], in slot order.
struct LocatedStepArgs {
    const float4 *__restrict__ pos_in;   // n_total records, read at [first, first + count)
    const float4 *__restrict__ vel_in;
    float4 *__restrict__ pos_out;        // n_total records; [first, first + count) written
    float4 *__restrict__ vel_out;
    uint32_t first, count;
    float dt, G, bias;                   // main.rs:411-413
};
hipError_t launch_nbody_located(const LocatedStepArgs &a, const uint32_t *seen_count, const float4 *seen_rel, uint32_t stride, hipStream_t s);

}  // namespace nbk
