// nb_kernels.hip -- gfx950 (MI355X / CDNA4) kernels for nenbody's all-pairs gravity + Euler step.
//
// Path: update_instance_nbody, reference src/main.rs:404-441.  Per body n, against the
// start-of-step snapshot of all positions (old_positions, main.rs:415):
//     a_n = sum_{i=0..N-1} ((p_i - p_n) * G) / (|p_i - p_n|^2 + bias)      main.rs:425-432 (i == n included)
//     v_n = v_n + a_n * dt                                                  main.rs:434
//     p_n = v_n + p_n                      (new v, no dt)                   main.rs:436
//     M_n = T(p_n) * Rz(atan2(v_n.y, v_n.x))                                main.rs:437-439, 141-143
//
// Mapping to the hardware (one thread per body, 64-lane waves, 256-thread workgroups):
//   - the j loop is tiled through LDS: a workgroup stages TJ 16-byte position records per tile
//     (coalesced global_load_dwordx4 -> ds_write_b128, double buffered, one barrier per tile);
//     every lane then walks the tile IN INDEX ORDER reading the same LDS address (a broadcast:
//     no bank conflict), so each wave-instruction evaluates 64 pairs.
//   - the work is fp32 VALU (no MFMA: pairwise math, not a contraction); HBM traffic is 48 B per
//     body per step against 18*N flop per body, so the kernel is VALU-issue bound.
//   - STRICT: the reference's exact binary32 operation order.  The divides by the same denominator share one
//     v_rcp_f32 + Newton step and take ONE FMA correction step each (div_ladder): the compiler's IEEE divide takes two,
//     and an enumeration of all 2^23 x 2^23 significand pairs shows the second never changes the result here; a range
//     guard falls back to the plain IEEE '/' where the unscaled ladder is not covered by that proof.  The fold is packed
//     across consecutive j's (pair2_strict), not across components.  Result: bit-identical.  Shards too small to fill
//     the chip with one lane per body run the block-chain kernel (nb_nbody_bc.inc).
//   - FAST: FMA chain for r^2, v_rcp_f32 for the divide, G hoisted, IB bodies per thread to amortise
//     the LDS reads, j range optionally split over blockIdx.y with a fixed-order combine.
//
// Everything is compiled with -ffp-contract=off: every fused multiply-add is an explicit __builtin_fmaf, every
// unfused a*b+c stays two roundings.
//
// Source layout.  This file is compiled THREE times (Makefile): as is; with -DNBK_NOSLP_TU -fno-slp-vectorize for the kernels
// that lose from SLP packing; and with -DNBK_SL_TU and the machine scheduler switched off for the scalar-load STRICT kernel,
// whose source order is its issue order (nb_nbody_sl.inc).  The kernels live in per-topic includes:
//   nb_nbody_strict.inc  STRICT arithmetic + step_strict_kernel<TJ,U,S>  (S = 1 here; S > 1 "j-parallel" in the SLP-off unit)
//   nb_nbody_pc.inc      STRICT producer/consumer kernel                  (this unit)
//   nb_nbody_bc.inc      STRICT block-chain kernel for small shards        (this unit)
//   nb_nbody_sl.inc      STRICT scalar-load kernel: whole sets and large shards, no LDS, no barrier  (its own unit)
//   nb_nbody_sym.inc     FAST pairs form: every unordered pair evaluated once, whole sets       (the scalar-load unit)
//   nb_nbody_ring.inc    FAST pairs form on a shard ("half shell"): a second exchange carries the other GPUs' halves  (the scalar-load unit)
//   nb_nbody_fast.inc    FAST kernels + fixed-order combine               (this unit)
//   nb_aux.inc           model matrices, cameras, random walk, self-test  (this unit)
//   nb_boids.inc         boids controller: one-lane, chain-split and producer/consumer kernels over one tile stage, form ladder and epilogue (SLP-off unit)
//   nb_raster.inc        what the four files below share: vertices, clip, depth, fragment, sRGB bytes (SLP-off unit; device functions only)
//   nb_eyes.inc          every entity's eye view: depth + entity id per column (SLP-off unit; its own launcher, nb_eyes.h)
//   nb_frame.inc         the scene camera's frame: ids, depth and colour per pixel (SLP-off unit; its own launcher, nb_frame.h)
//   nb_eyes_msaa.inc     the eye view through 8 samples per column, resolved (SLP-off unit; launcher in nb_eyes.h)
//   nb_frame_msaa.inc    the scene camera's frame through 8 samples per pixel, resolved (SLP-off unit; launcher in nb_frame.h)
//   nb_seen.inc          the seen set of every eye row; the boids step over what each body sees (SLP-off unit; launchers in nb_seen.h)
//   nb_located.inc       where each eye sees the members of its seen set; the gravity step over those relative positions (SLP-off unit; launchers in nb_located.h)
//   nb_scenes.inc        scene batches: B scenes of up to 2 048 bodies, k steps, one workgroup per scene (SLP-off unit; launchers in nb_scenes.h)
//   nb_scenes_seen.inc   scene batches: the seen boids step, eye row and seen set in LDS, one workgroup per eye (SLP-off unit; launchers in nb_scenes.h)
//   nb_scenes_located.inc scene batches: gravity from located vision, row, depths, columns and quotients in LDS, one workgroup per eye (SLP-off unit; launchers in nb_scenes.h)
//   nb_scenes_policy.inc scene batches: a neural policy over each eye row, row, pooled features and hidden layer in LDS, one workgroup per eye (SLP-off unit; launchers in nb_scenes.h)
//   nb_scenes_policy_recurrent.inc scene batches: that policy with H words of memory per body kept in device memory between steps, one workgroup per eye (SLP-off unit; launchers in nb_scenes.h)
//   nb_scenes_score.inc  scene batches: every scene's snapshot reduced to a 32-byte record of metrics, positions and partial sums in LDS, one workgroup per scene (SLP-off unit; launcher in nb_scenes.h)
//   nb_scenes_es.inc     scene batches: an evolution-strategies generation -- the population drawn by Philox, the records ranked in one workgroup, the mean updated from exact integer sums (SLP-off unit; launchers in nb_scenes.h)
//   nb_launch.inc        host-side launchers
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "nb_kernels.h"
#ifdef NBK_NOSLP_TU
#include "nb_eyes.h"
#include "nb_frame.h"
#include "nb_seen.h"
#include "nb_located.h"
#include "nb_scenes.h"
#endif

namespace nbk {

static constexpr int kBlock = 256;   // threads per workgroup = 4 waves, one per SIMD of a CU
static constexpr int kWaves = kBlock / 64;
[[maybe_unused]] static inline uint32_t ceil_div_u(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }

#include "nb_nbody_strict.inc"  // both translation units: the one-lane form here, the j-parallel shapes in the SLP-off unit

#if defined(NBK_SL_TU)
#include "nb_nbody_sl.inc"    // alone in its unit: compiled without the machine scheduler (its source order is its issue order)
#include "nb_nbody_sym.inc"   // FAST, every unordered pair once: hand-ordered like the scalar-load folds
#include "nb_nbody_ring.inc"  // the same on a shard of a multi-GPU job: the blocks on a ring, each against the half that follows it
#elif defined(NBK_NOSLP_TU)
#include "nb_boids.inc"
#include "nb_raster.inc"      // the rule the four files below share, once: outside the two units kernel_code_sha() stamps the evidence with
static_assert(kMsaaOffsets16 == sample_nibbles(kEyeSampleX16) && kFrameMsaaOffsetsY16 == sample_nibbles(kFrameSampleY16),
              "the kernels' sample offsets are the ones nb_eyes_sample_offsets / nb_frame_sample_offsets hand out");
#include "nb_eyes.inc"        // every entity's eye view: likewise
#include "nb_frame.inc"       // the scene camera's frame: likewise
#include "nb_eyes_msaa.inc"   // the eye view through 8 samples per column: likewise; uses nb_eyes.inc's edge
#include "nb_frame_msaa.inc"  // the frame through 8 samples per pixel: likewise; uses nb_frame.inc's edge and clear
#include "nb_seen.inc"        // the seen set of every eye row and the boids step over it: likewise; uses nb_boids.inc's accumulators and epilogue
#include "nb_located.inc"     // the located seen sets and the gravity step over them: likewise; uses nb_seen.inc's constants and nb_nbody_strict.inc's integrate
#include "nb_scenes.inc"      // scene batches, one workgroup per scene: likewise; uses nb_nbody_strict.inc's folds and nb_boids.inc's pair and epilogue
#include "nb_scenes_seen.inc" // the seen boids step of a batch, one workgroup per eye: likewise; uses nb_eyes.inc's eye_row_fill, nb_seen.inc's pair and nb_boids.inc's epilogue
#include "nb_scenes_located.inc" // gravity from located vision for a batch, one workgroup per eye: likewise; uses nb_eyes.inc's eye_row_fill, nb_located.inc's L2-L4 and G2 helpers, nb_scenes_seen.inc's bitmap helpers and nb_nbody_strict.inc's integrate
#include "nb_scenes_policy.inc" // a neural policy over each eye row of a batch, one workgroup per eye: likewise; uses nb_eyes.inc's eye_row_fill, nb_located.inc's located_basis, nb_scenes_seen.inc's launch shape and nb_nbody_strict.inc's integrate
#include "nb_scenes_policy_recurrent.inc" // the recurrent policy of a batch, one workgroup per eye: likewise; uses nb_scenes_policy.inc's pooling, outputs and actuation as they are
#include "nb_scenes_score.inc" // the score of a batch, one workgroup per scene: likewise; uses nb_scenes.inc's launch ladder and nb_scenes_policy.inc's policy_finite
#include "nb_scenes_es.inc"   // one evolution-strategies generation over a batch: likewise; uses nb_scenes_score.inc's score_wave_sum
#else
#include "nb_nbody_pc.inc"
#include "nb_nbody_bc.inc"
#include "nb_nbody_fast.inc"
#include "nb_aux.inc"
#endif

#ifndef NBK_SL_TU
#include "nb_launch.inc"
#endif

}  // namespace nbk
