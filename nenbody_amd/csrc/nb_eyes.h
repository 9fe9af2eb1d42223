// nb_eyes.h -- launcher of the eye kernel (nb_eyes.inc, compiled in the SLP-off unit of nb_kernels.hip), for the C ABI (nb_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nbk {

// The 8 samples of a column (rule step M1): sample k at c + kEyeSampleX16[k] / 16, the x half of Vulkan's standard 8-sample pattern.
// nb_eyes_sample_offsets hands these out; the kernels carry them as one nibble each (nb_raster.inc), tied to this list in
// nb_kernels.hip.
static constexpr uint32_t kEyeSampleX16[8] = {9, 7, 13, 5, 3, 1, 11, 15};
constexpr uint32_t sample_nibbles(const uint32_t (&v)[8])
{
    uint32_t p = 0;
    for (int k = 0; k < 8; ++k) p |= v[k] << (4 * k);
    return p;
}

// Every entity's eye view for eyes [first, first+count) of n_total bodies: cams = count cameras (eye e is
// body first + e), inst = n_total model matrices, 16 floats each, column-major, both 16-byte aligned; ids / depth: count x width
// each, either may be NULL.  The caller has checked the arguments (1 <= width <= NB_EYES_MAX_WIDTH, count >= 1).
hipError_t launch_eyes(uint32_t n_total, uint32_t first, uint32_t count, const float *cams, const float *inst, uint32_t width,
                       uint32_t flags, uint32_t *ids, float *depth, hipStream_t s);

// The same with the colour row (rule steps 6-11): skin = tw x th linear RGBA texels, row 0 first, 16-byte aligned, or NULL for the
// 1 x 1 white skin; rgba: count x width x 4 floats, 16-byte aligned; bgra8: count x width words whose bytes are B, G, R, A.  Any of
// the four outputs may be NULL.  The caller has checked the arguments (as above; 1 <= tw, th <= NB_EYES_MAX_SKIN where skin is given).
hipError_t launch_eyes_colour(uint32_t n_total, uint32_t first, uint32_t count, const float *cams, const float *inst, uint32_t width,
                              uint32_t flags, const float *skin, uint32_t tw, uint32_t th, uint32_t *ids, float *depth, float *rgba,
                              uint32_t *bgra8, hipStream_t s);

// The same through 8 samples per column (rule steps M1-M5, nb_eyes_msaa.inc): ids8 / depth8 hold count x width x 8 words, sample k
// of column c of eye e at (e * width + c) * 8 + k; rgba / bgra8 are the resolved rows, shaped as above.  Any of the four outputs may
// be NULL.  The caller has checked the arguments (1 <= width <= NB_EYES_MSAA_MAX_WIDTH: the eye's keys take 64 bytes of LDS a column).
hipError_t launch_eyes_msaa(uint32_t n_total, uint32_t first, uint32_t count, const float *cams, const float *inst, uint32_t width,
                            uint32_t flags, const float *skin, uint32_t tw, uint32_t th, uint32_t *ids8, float *depth8, float *rgba,
                            uint32_t *bgra8, hipStream_t s);

}  // namespace nbk
