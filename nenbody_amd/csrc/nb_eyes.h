// nb_eyes.h -- launcher of the eye kernel (nb_eyes.inc, compiled in the SLP-off unit of nb_kernels.hip), for the C ABI (nb_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nbk {

// Every entity's eye view for eyes [first, first+count) of n_total bodies: cams = count cameras (eye e is
// body first + e), inst = n_total model matrices, 16 floats each, column-major, both 16-byte aligned; ids / depth: count x width
// each, either may be NULL.  The caller has checked the arguments (1 <= width <= NB_EYES_MAX_WIDTH, count >= 1).
hipError_t launch_eyes(uint32_t n_total, uint32_t first, uint32_t count, const float *cams, const float *inst, uint32_t width,
                       uint32_t flags, uint32_t *ids, float *depth, hipStream_t s);

}  // namespace nbk
