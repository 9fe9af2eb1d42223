// nb_frame.h -- launcher of the frame kernels (nb_frame.inc, compiled in the SLP-off unit of nb_kernels.hip), for the C ABI (nb_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nb_eyes.h"

namespace nbk {

// The y half of the 8 samples of a pixel (rule step FM1; the x half is kEyeSampleX16): sample k at r + kFrameSampleY16[k] / 16.
static constexpr uint32_t kFrameSampleY16[8] = {5, 11, 9, 3, 13, 7, 15, 1};

// The scene camera's frame of n_total bodies: cam = one camera, inst = n_total model matrices, 16 floats each,
// column-major, both 16-byte aligned (inst may be NULL where n_total = 0); skin = tw x th linear RGBA texels, row 0 first, 16-byte
// aligned, or NULL for the 1 x 1 white skin; keys = width * height 64-bit words of scratch, rewritten by every call; ids / depth /
// bgra8: height x width words each, rgba: height x width x 4 floats, 16-byte aligned, row 0 the top; any of the four may be NULL.
// Three kernels on stream s: clear, edges, resolve.  The caller has checked the arguments (1 <= width, height <= NB_FRAME_MAX_DIM).
hipError_t launch_frame(uint32_t n_total, const float *cam, const float *inst, uint32_t width, uint32_t height, const float *skin,
                        uint32_t tw, uint32_t th, uint64_t *keys, uint32_t *ids, float *depth, float *rgba, uint32_t *bgra8, hipStream_t s);

// The same frame through 8 samples per pixel, resolved: inputs as launch_frame's; keys = width * height * 8
// 64-bit words of scratch, rewritten by every call; ids8 / depth8: height x width x 8 words each, sample k of pixel (c, r) at
// (r * width + c) * 8 + k; rgba / bgra8 as launch_frame's; any of the four may be NULL.  Three kernels on stream s: clear, edges,
// resolve.  The caller has checked the arguments (1 <= width, height <= NB_FRAME_MSAA_MAX_DIM).
hipError_t launch_frame_msaa(uint32_t n_total, const float *cam, const float *inst, uint32_t width, uint32_t height, const float *skin,
                             uint32_t tw, uint32_t th, uint64_t *keys, uint32_t *ids8, float *depth8, float *rgba, uint32_t *bgra8,
                             hipStream_t s);

}  // namespace nbk
