"""ctypes binding of libnenbody_hip.so (the C ABI declared in include/nenbody.h).

The library is the product; this module only loads it and declares prototypes.  There is no
Python or CPU implementation of the step to fall back to: if the shared object is missing the import
of the binding fails loudly, and on a machine without a HIP device every compute entry point returns
NB_ERR_NO_DEVICE, surfaced here as :class:`NbError`.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_size_t, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# NENBODY_LIB overrides the path (kernel experiments: a second build of the same sources with other flags)
LIB_PATH = os.environ.get("NENBODY_LIB") or os.path.join(_HERE, "lib", "libnenbody_hip.so")

NB_ABI_VERSION = 2
NB_OK = 0
NB_ERR_INVALID = -1
NB_ERR_NO_DEVICE = -2
NB_ERR_HIP = -3
NB_ERR_ALLOC = -4
NB_ERR_STATE = -5
NB_ERR_UNSUPPORTED = -6

NB_MODE_STRICT = 0
NB_MODE_FAST = 1
NB_PHASE_RANGE = 0
NB_PHASE_REST = 1
# phases of the pairs form on shards (nb_launch_ring_fold_phase)
NB_RING_OWN, NB_RING_REST, NB_RING_SUMS, NB_RING_OWN_READY = 1, 2, 3, 4
# every entity's eye view (nb_eyes / nb_launch_eyes)
NB_SCENES_MAX_BODIES = 2048
NB_POLICY_MAX_FEATURES = 256
NB_POLICY_MAX_HIDDEN = 64
NB_ES_MAX_POPULATION = 4096
NB_ES_MAX_FLOATS = 20674
NB_EYES_NONE = 0xFFFFFFFF
NB_EYES_SEE_SELF = 1
NB_EYES_MAX_WIDTH = 4096
NB_EYES_MAX_SKIN = 2048
# the eye rows through 8 samples per column (nb_eyes_msaa / nb_launch_eyes_msaa)
NB_EYES_SAMPLES = 8
NB_EYES_MSAA_MAX_WIDTH = 2048
# the scene camera's frame (nb_frame / nb_launch_frame)
NB_FRAME_MAX_DIM = 4096
# the frame through 8 samples per pixel (nb_frame_msaa / nb_launch_frame_msaa)
NB_FRAME_MSAA_MAX_DIM = 2048

_STATUS_NAMES = {
    NB_ERR_INVALID: "NB_ERR_INVALID",
    NB_ERR_NO_DEVICE: "NB_ERR_NO_DEVICE",
    NB_ERR_HIP: "NB_ERR_HIP",
    NB_ERR_ALLOC: "NB_ERR_ALLOC",
    NB_ERR_STATE: "NB_ERR_STATE",
    NB_ERR_UNSUPPORTED: "NB_ERR_UNSUPPORTED",
}


class NbParams(ctypes.Structure):
    """struct nb_params (include/nenbody.h); defaults are the reference's src/main.rs:411-413."""

    _fields_ = [("dt", c_float), ("G", c_float), ("bias", c_float), ("tile", c_uint32), ("mode", c_uint32)]

    def __repr__(self) -> str:  # pragma: no cover - debugging aid
        return f"NbParams(dt={self.dt}, G={self.G}, bias={self.bias}, tile={self.tile}, mode={self.mode})"


class NbBoidsParams(ctypes.Structure):
    """struct nb_boids_params (include/nenbody.h); defaults are the reference's src/main.rs:450-456."""

    _fields_ = [("dt", c_float), ("rule_1_distance", c_float), ("rule_2_distance", c_float), ("rule_3_distance", c_float),
                ("rule_1_scale", c_float), ("rule_2_scale", c_float), ("rule_3_scale", c_float), ("tile", c_uint32)]


class NbScoreParams(ctypes.Structure):
    """struct nb_score_params (include/nenbody.h, Q2 and Q5): the radius of `near`, squared, and the goal."""

    _fields_ = [("radius_sq", c_float), ("goal", c_float * 3)]


class NbEsParams(ctypes.Structure):
    """struct nb_es_params (include/nenbody.h, E1-E7): the draw's scale, the update's step, the fitness's six coefficients over
    (near, spread, speed2, momentum2, goal2, nonfinite) and the generator's seed."""

    _fields_ = [("sigma", c_float), ("step", c_float), ("coef", c_float * 6), ("seed", c_uint64)]


class NbEsReport(ctypes.Structure):
    """struct nb_es_report (include/nenbody.h): what the ranking of a generation leaves."""

    _fields_ = [("best_scene", c_uint32), ("best_fitness", c_float), ("nan_count", c_uint32), ("generation", c_uint32)]


class NbError(RuntimeError):
    """A non-zero nb_status from the library."""

    def __init__(self, status: int, message: str):
        self.status = status
        super().__init__(f"{_STATUS_NAMES.get(status, status)}: {message}")


# every symbol include/nenbody.h declares: name -> (restype, argtypes)
NB_COMM_ID_BYTES = 128
# nb_gather_fn: int (*)(void *user, void *buf, size_t slot_bytes, int rank, int world, void *stream)
GATHER_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p)

# nb_ring_fn: int (*)(void *user, const void *send, void *recv, size_t chunk_bytes, int partners, int rank, int world, void *stream)
RING_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p)

PROTOTYPES = {
    "nb_abi_version": (c_int, []),
    "nb_default_params": (None, [POINTER(NbParams)]),
    "nb_device_count": (c_int, []),
    "nb_last_error": (c_char_p, [c_void_p]),
    "nb_init_state": (c_int, [c_uint64, c_uint32, c_void_p, c_void_p]),
    "nb_create": (c_int, [c_uint32, c_uint32, POINTER(NbParams), POINTER(c_void_p)]),
    "nb_destroy": (None, [c_void_p]),
    "nb_upload": (c_int, [c_void_p, c_void_p, c_void_p]),
    "nb_step": (c_int, [c_void_p, c_uint32]),
    "nb_download": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_boids_default_params": (None, [POINTER(NbBoidsParams)]),
    "nb_step_boids": (c_int, [c_void_p, c_uint32, POINTER(NbBoidsParams)]),
    "nb_launch_boids_step": (
        c_int, [POINTER(NbBoidsParams), c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_boids_split_scratch_bytes": (c_size_t, [POINTER(NbBoidsParams), c_uint32, c_uint32]),
    "nb_launch_boids_step_split": (
        c_int, [POINTER(NbBoidsParams), c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "nb_step_random": (c_int, [c_void_p, c_uint32, c_uint64]),
    "nb_device_state": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p)]),
    "nb_cameras": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_camera_constant": (c_int, [ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, c_void_p]),
    "nb_launch_cameras": (c_int, [c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_eyes": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p]),
    "nb_launch_eyes": (c_int, [c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p]),
    "nb_eyes_skin": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32]),
    "nb_eyes_colour": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_launch_eyes_colour": (c_int, [c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_eyes_sample_offsets": (c_int, [c_void_p]),
    "nb_eyes_msaa": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_launch_eyes_msaa": (c_int, [c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_eyes_seen": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_launch_seen": (c_int, [c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_step_boids_seen": (c_int, [c_void_p, c_uint32, POINTER(NbBoidsParams), c_void_p, c_void_p, c_uint32, c_uint32]),
    "nb_launch_boids_seen_step": (
        c_int, [POINTER(NbBoidsParams), c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p,
                c_void_p]),
    "nb_eyes_located": (
        c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                c_void_p]),
    "nb_seen_located_launch": (
        c_int, [c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                c_void_p, c_void_p]),
    "nb_step_nbody_located": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_uint32, c_uint32]),
    "nb_nbody_located_step_launch": (
        c_int, [POINTER(NbParams), c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p,
                c_void_p]),
    "nb_scenes_nbody_step_launch": (c_int, [POINTER(NbParams), c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p]),
    "nb_scenes_boids_step_launch": (c_int, [POINTER(NbBoidsParams), c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p]),
    "nb_scenes_create": (c_int, [c_uint32, c_uint32, POINTER(NbParams), POINTER(c_void_p)]),
    "nb_scenes_destroy": (None, [c_void_p]),
    "nb_scenes_upload": (c_int, [c_void_p, c_void_p, c_void_p]),
    "nb_scenes_step": (c_int, [c_void_p, c_uint32]),
    "nb_scenes_step_boids": (c_int, [c_void_p, c_uint32, POINTER(NbBoidsParams)]),
    "nb_scenes_download": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_scenes_device_state": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p)]),
    "nb_scenes_sync": (c_int, [c_void_p]),
    "nb_scenes_steps": (c_uint64, [c_void_p]),
    "nb_scenes_last_error": (c_char_p, [c_void_p]),
    "nb_srgb_decode_table": (c_int, [c_void_p]),
    "nb_srgb_encode": (c_int, [c_void_p, c_size_t, c_void_p]),
    "nb_camera_at": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_frame": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_frame_scratch_bytes": (c_size_t, [c_uint32, c_uint32]),
    "nb_launch_frame": (c_int, [c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_frame_sample_offsets": (c_int, [c_void_p]),
    "nb_frame_msaa": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_frame_msaa_scratch_bytes": (c_size_t, [c_uint32, c_uint32]),
    "nb_launch_frame_msaa": (c_int, [c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_launch_random_step": (c_int, [c_uint32, c_uint32, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p]),
    "nb_update_instance_nbody": (c_int, [c_void_p, c_size_t] * 5 + [POINTER(NbParams)]),
    "nb_update_instance_boids": (c_int, [c_void_p, c_size_t] * 5 + [POINTER(NbBoidsParams)]),
    "nb_update_instance_random": (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t]),
    "nb_update_instance_random_seeded": (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t, c_uint64, c_uint64]),
    "nb_update_random_seed": (None, [c_uint64]),
    "nb_update_release": (None, []),
    "nb_sync": (c_int, [c_void_p]),
    "nb_steps_done": (c_uint64, [c_void_p]),
    "nb_scratch_bytes": (c_size_t, [POINTER(NbParams), c_uint32, c_uint32]),
    "nb_launch_step": (
        c_int,
        [POINTER(NbParams), c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    "nb_scratch_bytes_phased": (c_size_t, [POINTER(NbParams), c_uint32, c_uint32, c_uint32, c_uint32]),
    "nb_launch_step_phase": (
        c_int,
        [POINTER(NbParams), c_uint32, c_uint32, c_uint32, c_uint32, c_uint32, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
         c_void_p],
    ),
    "nb_ring_partners": (c_int, [POINTER(NbParams), c_uint32, c_uint32, c_uint32]),
    "nb_ring_scratch_bytes": (c_size_t, [POINTER(NbParams), c_uint32, c_uint32, c_uint32]),
    "nb_launch_ring_fold": (c_int, [POINTER(NbParams), c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "nb_ring_phased": (c_int, [POINTER(NbParams), c_uint32, c_uint32, c_uint32]),
    "nb_launch_ring_fold_phase": (c_int, [POINTER(NbParams), c_uint32, c_uint32, c_uint32, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "nb_launch_ring_finish": (
        c_int, [POINTER(NbParams), c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_launch_ring_finish_phase": (
        c_int, [POINTER(NbParams), c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "nb_launch_status": (c_int, [c_void_p]),
    "nb_launch_instances": (c_int, [c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_launch_pack": (c_int, [c_uint32, c_void_p, c_void_p, c_void_p]),
    "nb_launch_unpack": (c_int, [c_uint32, c_void_p, c_void_p, c_void_p]),
    "nb_comm_id": (c_int, [c_void_p]),
    "nb_shard_create": (c_int, [c_uint32, c_int, c_int, POINTER(NbParams), POINTER(c_void_p)]),
    "nb_shard_destroy": (None, [c_void_p]),
    "nb_shard_use_rccl": (c_int, [c_void_p, c_void_p]),
    "nb_shard_use_gather": (c_int, [c_void_p, GATHER_FN, c_void_p]),
    "nb_shard_set_overlap": (c_int, [c_void_p, c_int]),
    "nb_shard_use_ring": (c_int, [c_void_p, RING_FN, c_void_p]),
    "nb_shard_set_pairs": (c_int, [c_void_p, c_int]),
    "nb_shard_pairs_partners": (c_int, [c_void_p]),
    "nb_shard_pairs_overlapped": (c_int, [c_void_p]),
    "nb_shard_verify_exchanges": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "nb_shard_peer_export": (c_int, [c_void_p, c_void_p]),
    "nb_shard_peer_import": (c_int, [c_void_p, c_void_p]),
    "nb_shard_use_peers": (c_int, [c_void_p, c_int]),
    "nb_peers_blob_bytes": (c_size_t, []),
    "nb_peers_create": (c_int, [c_int, c_int, POINTER(c_void_p)]),
    "nb_peers_destroy": (None, [c_void_p]),
    "nb_peers_last_error": (c_char_p, [c_void_p]),
    "nb_peers_export": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_size_t), c_int, c_void_p]),
    "nb_peers_import": (c_int, [c_void_p, c_void_p]),
    "nb_peers_probe": (c_int, [c_void_p, c_uint32]),
    "nb_peers_signal": (c_int, [c_void_p, c_int, c_void_p]),
    "nb_peers_gather": (c_int, [c_void_p, c_int, c_int, c_size_t, c_void_p]),
    "nb_peers_ring": (c_int, [c_void_p, c_int, c_int, c_void_p, c_size_t, c_int, c_void_p]),
    "nb_shard_choose_form": (c_int, [c_void_p, c_uint32, POINTER(c_int), POINTER(ctypes.c_double)]),
    "nb_shard_set_boids_split": (c_int, [c_void_p, c_int]),
    "nb_shard_range": (c_int, [c_void_p, POINTER(c_uint32), POINTER(c_uint32)]),
    "nb_shard_upload": (c_int, [c_void_p, c_void_p, c_void_p]),
    "nb_shard_step": (c_int, [c_void_p, c_uint32]),
    "nb_shard_step_boids": (c_int, [c_void_p, c_uint32, POINTER(NbBoidsParams)]),
    "nb_shard_download": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_shard_sync": (c_int, [c_void_p]),
    "nb_shard_last_error": (c_char_p, [c_void_p]),
}

# include/nenbody_scenes_seen.h: the seen boids step of scene batches, bound with the table above
SCENES_SEEN_PROTOTYPES = {
    "nb_scenes_boids_seen_step_launch": (c_int, [POINTER(NbBoidsParams), c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p,
                                                 c_void_p, c_void_p, c_void_p]),
    "nb_scenes_seen_launch": (c_int, [c_uint32, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p]),
    "nb_scenes_step_boids_seen": (c_int, [c_void_p, c_uint32, POINTER(NbBoidsParams), c_void_p, c_void_p, c_uint32]),
    "nb_scenes_eyes_seen": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p]),
}

# include/nenbody_scenes_located.h: gravity from located vision for scene batches, bound likewise
SCENES_LOCATED_PROTOTYPES = {
    "nb_scenes_nbody_located_step_launch": (c_int, [POINTER(NbParams), c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32,
                                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_scenes_located_launch": (c_int, [c_uint32, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_scenes_step_nbody_located": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_uint32]),
    "nb_scenes_eyes_located": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
}

# include/nenbody_scenes_policy.h: a neural policy over each eye row of scene batches, bound likewise
SCENES_POLICY_PROTOTYPES = {
    "nb_policy_floats": (c_size_t, [c_uint32, c_uint32]),
    "nb_scenes_policy_step_launch": (c_int, [POINTER(NbParams), c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_uint32,
                                             c_uint32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_scenes_policy_observe_launch": (c_int, [c_uint32, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_uint32,
                                                c_uint32, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "nb_scenes_set_policy": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_float]),
    "nb_scenes_step_policy": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_uint32]),
    "nb_scenes_eyes_policy": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p]),
}

# include/nenbody_scenes_score.h: the score of every scene, accumulated on the device, bound likewise
SCENES_SCORE_PROTOTYPES = {
    "nb_scenes_score_launch": (c_int, [POINTER(NbScoreParams), c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_scenes_set_score": (c_int, [c_void_p, POINTER(NbScoreParams)]),
    "nb_scenes_score": (c_int, [c_void_p]),
    "nb_scenes_score_reset": (c_int, [c_void_p]),
    "nb_scenes_scores": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p]),
    "nb_scenes_step_policy_scored": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_uint32]),
}

# include/nenbody_scenes_es.h: an evolution-strategies generation on the device, bound likewise
ES_PROTOTYPES = {
    "nb_scenes_es_perturb_launch": (c_int, [POINTER(NbEsParams), c_uint32, c_uint32, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p]),
    "nb_scenes_es_update_launch": (c_int, [POINTER(NbEsParams), c_uint32, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p]),
    "nb_scenes_es_set": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_float, POINTER(NbEsParams)]),
    "nb_scenes_es_perturb": (c_int, [c_void_p]),
    "nb_scenes_es_update": (c_int, [c_void_p]),
    "nb_scenes_es_mean": (c_int, [c_void_p, c_void_p]),
    "nb_scenes_es_result": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "nb_scenes_es_generation": (c_uint32, [c_void_p]),
    "nb_scenes_keep": (c_int, [c_void_p]),
    "nb_scenes_rewind": (c_int, [c_void_p]),
}

# include/nenbody_scenes_policy_recurrent.h: a recurrent policy with per-body memory, bound likewise
SCENES_POLICY_RECURRENT_PROTOTYPES = {
    "nb_policy_recurrent_floats": (c_size_t, [c_uint32, c_uint32]),
    "nb_scenes_policy_recurrent_step_launch": (c_int, [POINTER(NbParams), c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32,
                                                       c_uint32, c_uint32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                                       c_void_p, c_void_p, c_void_p]),
    "nb_scenes_policy_recurrent_observe_launch": (c_int, [c_uint32, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_uint32,
                                                          c_uint32, c_uint32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                                          c_void_p]),
    "nb_scenes_es_perturb_floats_launch": (c_int, [POINTER(NbEsParams), c_uint32, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p]),
    "nb_scenes_es_update_floats_launch": (c_int, [POINTER(NbEsParams), c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                                  c_void_p, c_void_p, c_void_p]),
    "nb_scenes_set_policy_recurrent": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_float, c_float]),
    "nb_scenes_eyes_policy_memory": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p]),
    "nb_scenes_memory_reset": (c_int, [c_void_p]),
    "nb_scenes_memory": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p]),
    "nb_scenes_set_memory": (c_int, [c_void_p, c_void_p]),
    "nb_scenes_es_set_recurrent": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_float, c_float, POINTER(NbEsParams)]),
}

# every symbol include/nenbody_diag.h declares (self-tests, the test suite's switches): not part of the drop-in boundary
DIAG_PROTOTYPES = {
    "nb_selftest_ladder": (c_int, [c_uint32, c_uint32, POINTER(c_uint64), c_void_p]),
    "nb_selftest_rcp_scaling": (c_int, [c_int, c_int, POINTER(c_uint64)]),
    "nb_selftest_matrices": (c_int, [c_uint32, c_uint64, POINTER(c_uint64), c_void_p]),
    "nb_selftest_libm": (c_int, [c_int, c_uint32, c_uint64, c_uint32, POINTER(c_uint64), POINTER(c_uint32)]),
    "nb_selftest_divide": (c_int, [POINTER(NbParams), c_uint64, c_uint64, POINTER(c_uint64), c_void_p]),
    "nb_selftest_valu_rate": (c_int, [c_int, ctypes.c_double, POINTER(ctypes.c_double), POINTER(ctypes.c_double)]),
    "nb_diag_step_clock": (c_int, [POINTER(NbParams), c_uint32, ctypes.c_double, POINTER(ctypes.c_double), POINTER(ctypes.c_double),
                                   POINTER(ctypes.c_double)]),
    "nb_debug_reload_env": (c_int, []),
    "nb_diag_enable_env": (c_int, [c_int]),
    "nb_diag_rccl_solo": (c_int, [c_int]),
    "nb_diag_legacy_forms": (c_int, []),
    "nb_diag_peers_lossy": (c_int, [c_int]),
    "nb_diag_plan": (c_int, [POINTER(NbParams), c_uint32, c_uint32, ctypes.c_char_p, c_size_t]),
}

_lib = None


def _preload_torch_hip_runtime() -> None:
    """Make a torch process hold ONE HIP runtime.

    libnenbody_hip.so needs `libamdhip64.so.7` (by SONAME); torch's wheels bundle their own copy with the same SONAME
    but load it by FILE name (`libamdhip64.so`, RPATH $ORIGIN), so without help the process ends up with two runtimes:
    streams and events of one mean nothing to the other, and whichever initialises second may find no device.
    Loading torch's copy first (no `import torch` needed) makes both the library and torch resolve to it.  A process
    without torch (the C++/Rust hosts) simply uses the system runtime.  NENBODY_SYSTEM_HIP=1 skips this.
    """
    if os.environ.get("NENBODY_SYSTEM_HIP"):
        return
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
            rccl = os.path.join(os.path.dirname(path), "librccl.so")
            if os.path.exists(rccl):  # nb_shard_use_rccl: the RCCL built against that runtime
                os.environ.setdefault("NENBODY_RCCL", rccl)
    except Exception:  # pragma: no cover - best effort; the loader falls back to the system runtime
        pass


_loaded = {}   # path -> bound CDLL


def _bind(path: str) -> ctypes.CDLL:
    if path in _loaded:
        return _loaded[path]
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `make -C nenbody_amd/csrc` (hipcc, gfx950). "
            "nenbody_amd has no CPU fallback."
        )
    _preload_torch_hip_runtime()
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in list(PROTOTYPES.items()) + list(SCENES_SEEN_PROTOTYPES.items()) + list(SCENES_LOCATED_PROTOTYPES.items()) \
            + list(SCENES_POLICY_PROTOTYPES.items()) + list(SCENES_SCORE_PROTOTYPES.items()) + list(ES_PROTOTYPES.items()) \
            + list(SCENES_POLICY_RECURRENT_PROTOTYPES.items()) + list(DIAG_PROTOTYPES.items()):
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    got = lib.nb_abi_version()
    if got != NB_ABI_VERSION:
        raise ImportError(f"{os.path.basename(path)} ABI {got} != binding ABI {NB_ABI_VERSION}")
    _loaded[path] = lib
    return lib


def load() -> ctypes.CDLL:
    """Load libnenbody_hip.so (built by nenbody_amd/csrc/Makefile or __graft_entry__.build())."""
    global _lib
    if _lib is None:
        _lib = _bind(LIB_PATH)
    return _lib


# Test infrastructure: the product library holds the launch shapes its own plan reaches; the shapes only the diagnostic knobs can
# name (NB_STRICT_PC, NB_FAST_WAVES, ...: rounds 1-3's measurement history) live in libnenbody_hip_legacy.so, the same sources built
# with -DNB_LEGACY_FORMS (`make -C nenbody_amd/csrc legacy`).  The test suite binds it for the tests that name such a shape.
LEGACY_LIB_PATH = os.path.join(_HERE, "lib", "libnenbody_hip_legacy.so")


def use_library(path=None) -> str:
    """Bind another build of the library for the calls that follow (None: back to LIB_PATH); returns the path that was bound.
    Objects created before the switch keep the library they were created with."""
    global _lib
    before = next((p for p, lib in _loaded.items() if lib is _lib), LIB_PATH)
    _lib = _bind(path or LIB_PATH)
    return before


# the sources that define the kernels bench.py times and profiles/hbm_traffic.json meters (the two whole-set folds, the block
# chain the shards of a multi-GPU run take, their launchers): NOT the boids controller, the aux kernels, the producer/consumer
# form, the host-side ABI or anything outside csrc/ -- edits there leave the PMC evidence valid
BENCHED_KERNEL_SOURCES = ("nb_kernels.hip", "nb_kernels.h", "nb_launch.inc", "nb_nbody_strict.inc", "nb_nbody_sl.inc", "nb_nbody_sym.inc", "nb_nbody_ring.inc", "nb_nbody_fast.inc",
                          "nb_nbody_bc.inc")


def kernel_source_sha() -> str:
    """sha256 (first 16 hex digits) over BENCHED_KERNEL_SOURCES, in name order: stamps measurements
    (profiles/hbm_traffic.json) with the code they were taken from, so a stale profile is recognised."""
    import hashlib

    h = hashlib.sha256()
    src = os.path.join(_HERE, "csrc")
    for name in sorted(BENCHED_KERNEL_SOURCES):
        h.update(name.encode())
        h.update(open(os.path.join(src, name), "rb").read())
    return h.hexdigest()[:16]


def kernel_code_sha(path: str = None) -> str:
    """sha256 (first 16 hex digits) of the DEVICE CODE of the benchmarked kernels as built into the library: the offload bundles of
    its `.hip_fatbin` section that hold the whole-set folds (the scalar-load unit: step_strict_sl_kernel, the pairs forms) and
    planes_kernel / the combines (the main unit) -- not the boids unit.  This is what stamps profiles/hbm_traffic.json since
    round 4: a comment, a test, a host-side or a boids edit leaves the measured kernels' code -- and so the evidence -- as it was,
    where the source-text hash above made every comment-only commit cost a rocprofv3 + PMC re-collection.
    The bundles carry no line numbers or paths: the same sources and compiler give the same bytes."""
    import hashlib
    import struct

    b = open(path or LIB_PATH, "rb").read()
    if b[:4] != b"\x7fELF":
        raise ValueError("not an ELF file")
    shoff = struct.unpack_from("<Q", b, 0x28)[0]
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize) for i in range(shnum)]
    stroff = secs[shstrndx][4]
    fat = None
    for sec in secs:
        name = b[stroff + sec[0]:b.index(b"\0", stroff + sec[0])]
        if name == b".hip_fatbin":
            fat = b[sec[4]:sec[4] + sec[5]]
    if fat is None:
        raise ValueError("no .hip_fatbin section")
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts, i = [], fat.find(magic)
    while i >= 0:
        starts.append(i)
        i = fat.find(magic, i + 1)
    h, used = hashlib.sha256(), 0
    for a, e in zip(starts, starts[1:] + [len(fat)]):
        bundle = fat[a:e]
        if b"step_strict_sl_kernel" in bundle or b"planes_kernel" in bundle:
            h.update(bundle)
            used += 1
    if used != 2:
        raise ValueError(f"expected the main and the scalar-load bundle in .hip_fatbin, found {used} of {len(starts)}")
    return h.hexdigest()[:16]


def planned_kernels(params: "NbParams", n_total: int, count: int) -> list:
    """The kernels one step of this shape launches, dominant one first, as the library plans it (nb_diag_plan)."""
    buf = ctypes.create_string_buffer(256)
    check(load().nb_diag_plan(ctypes.byref(params), n_total, count, buf, len(buf)))
    return buf.value.decode().split(",")


def default_params(mode: int = NB_MODE_STRICT, tile: int = 0) -> NbParams:
    p = NbParams()
    load().nb_default_params(ctypes.byref(p))
    p.mode = mode
    p.tile = tile
    return p


def default_boids_params(tile: int = 0) -> NbBoidsParams:
    p = NbBoidsParams()
    load().nb_boids_default_params(ctypes.byref(p))
    p.tile = tile
    return p


def last_error(ctx=None) -> str:
    msg = load().nb_last_error(ctx)
    return msg.decode("utf-8", "replace") if msg else ""


def check(status: int, ctx=None) -> None:
    if status != NB_OK:
        raise NbError(status, last_error(ctx))
