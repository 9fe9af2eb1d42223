// nb_scenes.h -- launchers of the scene-batch kernels (nb_scenes.inc, compiled in the SLP-off unit of nb_kernels.hip), for the C ABI
// (nb_scenes_api.inc).  A scene batch is `scenes` independent scenes of n <= kScenesMaxBodies bodies; body i of scene s is record
// s * n + i.  One launch steps every scene k times, one workgroup per scene, the scene's state on chip between the steps
// (DESIGN.md section 14).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nb_kernels.h"

namespace nbk {

constexpr uint32_t kScenesMaxBodies = 2048;   // NB_SCENES_MAX_BODIES: two bodies per lane of a 1024-lane workgroup
constexpr uint32_t kScenesMaxGrid = 2048;     // workgroups per launch; more scenes than that are walked by a grid-stride loop

// k >= 1 gravity steps (update_instance_nbody, STRICT) of every scene, in place.  The caller has checked the arguments.
struct ScenesNbodyArgs {
    float4 *pos, *vel;           // scenes * n records each, read at the start and written after step k
    uint32_t scenes, n, k;
    float dt, G, bias;           // main.rs:411-413
    uint32_t lo_bits, hi_bits;   // the divide guard's range, as StepArgs carries it
    uint32_t force_ieee;         // 1 = always the IEEE '/'
    uint32_t force_3d;           // 2 = never the planar shortcut
};
hipError_t launch_scenes_nbody(const ScenesNbodyArgs &a, hipStream_t s);

// k >= 1 boids steps (update_instance_boids) of every scene, in place.  `c`: the constants of a set of n bodies (n_total = count = n,
// first = 0) as make_boids_args forms them; its four buffer pointers are not read.
hipError_t launch_scenes_boids(const BoidsArgs &c, float4 *pos, float4 *vel, uint32_t scenes, uint32_t k, hipStream_t s);

}  // namespace nbk
