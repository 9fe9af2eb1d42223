"""What every stateless entry of the launch API answers to arguments it must refuse: the status and the full nb_last_error() text.

A table.  Each row is an entry, arguments that fail validation before anything touches the device (the addresses are fake and never
dereferenced, as in test_abi.py::test_launch_step_validates_pointers_and_ranges), the status and the message.  A message of None
means the call writes none: the size queries, and the calls that succeed without work (count == 0).  Rows marked "two faults" have
two arguments wrong at once and pin which check comes first.  The answers were recorded from the library as it was before the
host side of the launch API was folded into shared helpers; the table holds that refactor, and later ones, to them byte for byte.

No row may reach the device: on a machine with a GPU the fake addresses would be used.  nb_launch_status has no row for that
reason (it has no argument to refuse and waits for the device at once).  The context's entries have rows for the one refusal that
needs no context -- there is none --; what they answer with one is tests/test_gpu_ctx_entries.py's and tests/test_gpu_vision_entries.py's.
"""
import ctypes

import pytest

from nenbody_amd import _lib

A, B, C, D, E, F, G, H = (0x100000 * k for k in range(1, 9))   # fake device addresses, 1 MiB apart, 16-byte aligned

# the parameter blocks a row names: the defaults, FAST, a mode and a tile that do not exist; None is the NULL pointer
PARAMS = {
    "strict": lambda: _lib.default_params(),
    "fast": lambda: _lib.default_params(mode=_lib.NB_MODE_FAST),
    "badmode": lambda: _lib.default_params(mode=7),
    "badtile": lambda: _lib.default_params(tile=100),
    "boids": lambda: _lib.default_boids_params(),
    "boids_badtile": lambda: _lib.default_boids_params(tile=100),
}
SIZE_QUERIES = ("nb_scratch_bytes", "nb_scratch_bytes_phased", "nb_ring_scratch_bytes", "nb_boids_split_scratch_bytes",
                "nb_frame_scratch_bytes", "nb_frame_msaa_scratch_bytes")

# (entry, arguments, status or size, message)
ROWS = [
    # nb_scratch_bytes
    ('nb_scratch_bytes', ('strict', 131072, 131072), 1573184, None),
    ('nb_scratch_bytes', ('strict', 1000, 1000), 0, None),
    ('nb_scratch_bytes', (None, 4096, 4096), 49472, None),
    ('nb_scratch_bytes', ('fast', 4096, 1024), 82240, None),
    ('nb_scratch_bytes', ('fast', 10, 20), 0, None),
    ('nb_scratch_bytes', ('badmode', 4096, 4096), 0, None),
    # nb_launch_step
    ('nb_launch_step', ('strict', 16, 0, 16, None, B, C, None, 0, None), -1, 'nb_launch_step: pos_in, pos_out, vel must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_step', ('strict', 16, 0, 16, A, None, C, None, 0, None), -1, 'nb_launch_step: pos_in, pos_out, vel must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_step', ('strict', 16, 0, 16, A, B, None, None, 0, None), -1, 'nb_launch_step: pos_in, pos_out, vel must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_step', ('strict', 16, 0, 16, A, A, C, None, 0, None), -1, 'nb_launch_step: pos_in, pos_out, vel must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_step', ('strict', 16, 8, 9, A, B, C, None, 0, None), -1, 'nb_launch_step: [first, first+count) exceeds n_total'),
    ('nb_launch_step', ('strict', 16, 0xffffffff, 2, A, B, C, None, 0, None), -1, 'nb_launch_step: [first, first+count) exceeds n_total'),
    ('nb_launch_step', ('strict', 16, 0, 0, A, B, C, None, 0, None), -1, 'nb: need 0 < count <= n_total'),
    ('nb_launch_step', (None, 16, 0, 0, A, B, C, None, 0, None), -1, 'nb: need 0 < count <= n_total'),
    ('nb_launch_step', ('strict', 16, 0, 17, A, B, C, None, 0, None), -1, 'nb_launch_step: [first, first+count) exceeds n_total'),
    ('nb_launch_step', ('badmode', 16, 0, 16, A, B, C, None, 0, None), -1, 'nb: params.mode must be NB_MODE_STRICT or NB_MODE_FAST'),
    ('nb_launch_step', ('badtile', 16, 0, 16, A, B, C, None, 0, None), -1, 'nb: params.tile must be 0, 256, 512 or 1024'),
    ('nb_launch_step', ('strict', 0x80000001, 0, 1, A, B, C, None, 0, None), -6, 'nb: sets of more than 2^31 bodies are not supported'),
    ('nb_launch_step', ('fast', 131072, 0, 16384, A, B, C, None, 0, None), -1, 'nb_launch_step: scratch smaller than nb_scratch_bytes()'),
    ('nb_launch_step', ('fast', 131072, 0, 16384, A, B, C, D, 16, None), -1, 'nb_launch_step: scratch smaller than nb_scratch_bytes()'),
    ('nb_launch_step', ('strict', 4096, 0, 4096, A, B, C, D, 0xc13f, None), -1, 'nb_launch_step: scratch smaller than nb_scratch_bytes()'),
    ('nb_launch_step', ('strict', 16, 8, 9, None, B, C, None, 0, None), -1, 'nb_launch_step: pos_in, pos_out, vel must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_step', ('badmode', 16, 8, 9, A, B, C, None, 0, None), -1, 'nb_launch_step: [first, first+count) exceeds n_total'),
    ('nb_launch_step', ('badmode', 16, 0, 0, A, B, C, None, 0, None), -1, 'nb: need 0 < count <= n_total'),
    ('nb_launch_step', ('badtile', 0x80000001, 0, 1, A, B, C, None, 0, None), -6, 'nb: sets of more than 2^31 bodies are not supported'),
    # nb_scratch_bytes_phased
    ('nb_scratch_bytes_phased', ('fast', 4096, 1024, 1024, 2048), 98624, None),
    ('nb_scratch_bytes_phased', ('fast', 1024, 256, 0, 256), 8192, None),
    ('nb_scratch_bytes_phased', (None, 4096, 1024, 1024, 2048), 0, None),
    ('nb_scratch_bytes_phased', ('fast', 4096, 1024, 2048, 1024), 0, None),
    ('nb_scratch_bytes_phased', ('fast', 4096, 1024, 0, 4097), 0, None),
    ('nb_scratch_bytes_phased', ('fast', 4096, 0, 0, 16), 0, None),
    # nb_launch_step_phase
    ('nb_launch_step_phase', ('fast', 4096, 0, 1024, 1024, 2048, 0, None, B, C, D, 1073741824, None), -1, 'nb_launch_step_phase: pos_in, pos_out, vel, scratch must be non-null, pos_out must not alias pos_in, phase is NB_PHASE_RANGE or NB_PHASE_REST'),
    ('nb_launch_step_phase', ('fast', 4096, 0, 1024, 1024, 2048, 0, A, A, C, D, 1073741824, None), -1, 'nb_launch_step_phase: pos_in, pos_out, vel, scratch must be non-null, pos_out must not alias pos_in, phase is NB_PHASE_RANGE or NB_PHASE_REST'),
    ('nb_launch_step_phase', ('fast', 4096, 0, 1024, 1024, 2048, 0, A, B, C, None, 1073741824, None), -1, 'nb_launch_step_phase: pos_in, pos_out, vel, scratch must be non-null, pos_out must not alias pos_in, phase is NB_PHASE_RANGE or NB_PHASE_REST'),
    ('nb_launch_step_phase', ('fast', 4096, 0, 1024, 1024, 2048, 2, A, B, C, D, 1073741824, None), -1, 'nb_launch_step_phase: pos_in, pos_out, vel, scratch must be non-null, pos_out must not alias pos_in, phase is NB_PHASE_RANGE or NB_PHASE_REST'),
    ('nb_launch_step_phase', ('fast', 4096, 0, 1024, 1024, 2048, -1, A, B, C, D, 1073741824, None), -1, 'nb_launch_step_phase: pos_in, pos_out, vel, scratch must be non-null, pos_out must not alias pos_in, phase is NB_PHASE_RANGE or NB_PHASE_REST'),
    ('nb_launch_step_phase', ('fast', 4096, 3584, 1024, 1024, 2048, 0, A, B, C, D, 1073741824, None), -1, 'nb_launch_step_phase: [first, first+count) exceeds n_total'),
    ('nb_launch_step_phase', ('strict', 4096, 0, 1024, 1024, 2048, 0, A, B, C, D, 1073741824, None), -6, "nb: a step in phases is FAST only: the reference's sum runs j = 0..N-1 in order, and STRICT keeps that order"),
    ('nb_launch_step_phase', (None, 4096, 0, 1024, 1024, 2048, 1, A, B, C, D, 1073741824, None), -6, "nb: a step in phases is FAST only: the reference's sum runs j = 0..N-1 in order, and STRICT keeps that order"),
    ('nb_launch_step_phase', ('fast', 4096, 0, 1024, 2048, 1024, 0, A, B, C, D, 1073741824, None), -1, 'nb: need j_lo <= j_hi <= n_total'),
    ('nb_launch_step_phase', ('fast', 4096, 0, 1024, 0, 4097, 0, A, B, C, D, 1073741824, None), -1, 'nb: need j_lo <= j_hi <= n_total'),
    ('nb_launch_step_phase', ('fast', 4096, 0, 0, 1024, 2048, 0, A, B, C, D, 1073741824, None), -1, 'nb: need 0 < count <= n_total'),
    ('nb_launch_step_phase', ('badmode', 4096, 0, 1024, 1024, 2048, 0, A, B, C, D, 1073741824, None), -6, "nb: a step in phases is FAST only: the reference's sum runs j = 0..N-1 in order, and STRICT keeps that order"),
    ('nb_launch_step_phase', ('fast', 4096, 0, 1024, 1024, 2048, 0, A, B, C, D, 0, None), -1, 'nb_launch_step_phase: scratch smaller than nb_scratch_bytes_phased()'),
    ('nb_launch_step_phase', ('fast', 4096, 0, 1024, 1024, 2048, 1, A, B, C, D, 1000, None), -1, 'nb_launch_step_phase: scratch smaller than nb_scratch_bytes_phased()'),
    ('nb_launch_step_phase', ('fast', 4096, 3584, 1024, 1024, 2048, 7, A, B, C, D, 0, None), -1, 'nb_launch_step_phase: pos_in, pos_out, vel, scratch must be non-null, pos_out must not alias pos_in, phase is NB_PHASE_RANGE or NB_PHASE_REST'),
    ('nb_launch_step_phase', ('strict', 4096, 3584, 1024, 2048, 1024, 0, A, B, C, D, 0, None), -1, 'nb_launch_step_phase: [first, first+count) exceeds n_total'),
    ('nb_launch_step_phase', ('strict', 4096, 0, 1024, 2048, 1024, 0, A, B, C, D, 0, None), -6, "nb: a step in phases is FAST only: the reference's sum runs j = 0..N-1 in order, and STRICT keeps that order"),
    ('nb_launch_step_phase', ('fast', 4096, 0, 0, 2048, 1024, 0, A, B, C, D, 0, None), -1, 'nb: need j_lo <= j_hi <= n_total'),
    # nb_ring_partners
    ('nb_ring_partners', ('fast', 65536, 0, 16384), 2, None),
    ('nb_ring_partners', ('fast', 65536, 16384, 16384), 2, None),
    ('nb_ring_partners', (None, 65536, 0, 16384), 0, None),
    ('nb_ring_partners', ('strict', 65536, 0, 16384), 0, None),
    ('nb_ring_partners', ('fast', 4096, 0, 1024), 0, None),
    ('nb_ring_partners', ('fast', 65536, 0, 0), -1, 'nb: need 0 < count <= n_total'),
    ('nb_ring_partners', ('fast', 65536, 0, 65537), -1, 'nb: need 0 < count <= n_total'),
    ('nb_ring_partners', ('badmode', 65536, 0, 16384), -1, 'nb: params.mode must be NB_MODE_STRICT or NB_MODE_FAST'),
    ('nb_ring_partners', ('badtile', 65536, 0, 16384), -1, 'nb: params.tile must be 0, 256, 512 or 1024'),
    ('nb_ring_partners', ('fast', 65536, 57344, 16384), 0, None),
    ('nb_ring_partners', ('fast', 65536, 100, 16384), 0, None),
    # nb_ring_phased
    ('nb_ring_phased', ('fast', 65536, 0, 16384), 1, None),
    ('nb_ring_phased', ('fast', 65536, 16384, 16384), 1, None),
    ('nb_ring_phased', (None, 65536, 0, 16384), 0, None),
    ('nb_ring_phased', ('strict', 65536, 0, 16384), 0, None),
    ('nb_ring_phased', ('fast', 4096, 0, 1024), 0, None),
    ('nb_ring_phased', ('fast', 65536, 0, 0), -1, 'nb: need 0 < count <= n_total'),
    ('nb_ring_phased', ('fast', 65536, 0, 65537), -1, 'nb: need 0 < count <= n_total'),
    ('nb_ring_phased', ('badmode', 65536, 0, 16384), -1, 'nb: params.mode must be NB_MODE_STRICT or NB_MODE_FAST'),
    ('nb_ring_phased', ('badtile', 65536, 0, 16384), -1, 'nb: params.tile must be 0, 256, 512 or 1024'),
    ('nb_ring_phased', ('fast', 65536, 57344, 16384), 0, None),
    ('nb_ring_phased', ('fast', 65536, 100, 16384), 0, None),
    # nb_ring_scratch_bytes
    ('nb_ring_scratch_bytes', ('fast', 65536, 0, 16384), 30867776, None),
    ('nb_ring_scratch_bytes', ('fast', 65536, 16384, 16384), 30867776, None),
    ('nb_ring_scratch_bytes', (None, 65536, 0, 16384), 0, None),
    ('nb_ring_scratch_bytes', ('strict', 65536, 0, 16384), 0, None),
    ('nb_ring_scratch_bytes', ('fast', 4096, 0, 1024), 0, None),
    ('nb_ring_scratch_bytes', ('fast', 65536, 0, 0), 0, None),
    ('nb_ring_scratch_bytes', ('fast', 65536, 0, 65537), 0, None),
    ('nb_ring_scratch_bytes', ('badmode', 65536, 0, 16384), 0, None),
    ('nb_ring_scratch_bytes', ('badtile', 65536, 0, 16384), 0, None),
    ('nb_ring_scratch_bytes', ('fast', 65536, 57344, 16384), 0, None),
    ('nb_ring_scratch_bytes', ('fast', 65536, 100, 16384), 0, None),
    # nb_launch_ring_fold
    ('nb_launch_ring_fold', ('fast', 65536, 0, 16384, None, B, C, 1099511627776, None), -1, 'nb_launch_ring_fold: pos_in, sums and scratch must be non-null'),
    ('nb_launch_ring_fold', ('fast', 65536, 0, 16384, A, None, C, 1099511627776, None), -1, 'nb_launch_ring_fold: pos_in, sums and scratch must be non-null'),
    ('nb_launch_ring_fold', ('fast', 65536, 0, 16384, A, B, None, 1099511627776, None), -1, 'nb_launch_ring_fold: pos_in, sums and scratch must be non-null'),
    ('nb_launch_ring_fold', ('fast', 65536, 0, 0, A, B, C, 1099511627776, None), -1, 'nb: need 0 < count <= n_total'),
    ('nb_launch_ring_fold', ('badmode', 65536, 0, 16384, A, B, C, 1099511627776, None), -1, 'nb: params.mode must be NB_MODE_STRICT or NB_MODE_FAST'),
    ('nb_launch_ring_fold', ('strict', 65536, 0, 16384, A, B, C, 1099511627776, None), -6, 'nb_launch_ring_fold: this shape does not take the pairs form on shards (nb_ring_partners() == 0): use nb_launch_step'),
    ('nb_launch_ring_fold', (None, 65536, 0, 16384, A, B, C, 1099511627776, None), -6, 'nb_launch_ring_fold: this shape does not take the pairs form on shards (nb_ring_partners() == 0): use nb_launch_step'),
    ('nb_launch_ring_fold', ('fast', 4096, 0, 1024, A, B, C, 1099511627776, None), -6, 'nb_launch_ring_fold: this shape does not take the pairs form on shards (nb_ring_partners() == 0): use nb_launch_step'),
    ('nb_launch_ring_fold', ('fast', 65536, 0, 16384, A, B, C, 0, None), -1, 'nb_launch_ring_fold: scratch smaller than nb_ring_scratch_bytes()'),
    ('nb_launch_ring_fold', ('fast', 65536, 0, 0, None, B, C, 0, None), -1, 'nb_launch_ring_fold: pos_in, sums and scratch must be non-null'),
    ('nb_launch_ring_fold', ('strict', 65536, 0, 16384, A, B, C, 0, None), -6, 'nb_launch_ring_fold: this shape does not take the pairs form on shards (nb_ring_partners() == 0): use nb_launch_step'),
    # nb_launch_ring_fold_phase
    ('nb_launch_ring_fold_phase', ('fast', 65536, 0, 16384, 0, A, B, C, 1099511627776, None), -1, 'nb_launch_ring_fold_phase: phase must be NB_RING_OWN, NB_RING_REST, NB_RING_SUMS or NB_RING_OWN_READY'),
    ('nb_launch_ring_fold_phase', ('fast', 65536, 0, 16384, 5, A, B, C, 1099511627776, None), -1, 'nb_launch_ring_fold_phase: phase must be NB_RING_OWN, NB_RING_REST, NB_RING_SUMS or NB_RING_OWN_READY'),
    ('nb_launch_ring_fold_phase', ('fast', 65536, 0, 16384, -1, A, B, C, 1099511627776, None), -1, 'nb_launch_ring_fold_phase: phase must be NB_RING_OWN, NB_RING_REST, NB_RING_SUMS or NB_RING_OWN_READY'),
    ('nb_launch_ring_fold_phase', ('fast', 65536, 0, 16384, 1, None, B, C, 1099511627776, None), -1, 'nb_launch_ring_fold_phase: pos_in, sums and scratch must be non-null'),
    ('nb_launch_ring_fold_phase', ('fast', 65536, 0, 16384, 1, A, None, C, 1099511627776, None), -1, 'nb_launch_ring_fold_phase: pos_in, sums and scratch must be non-null'),
    ('nb_launch_ring_fold_phase', ('fast', 65536, 0, 16384, 1, A, B, None, 1099511627776, None), -1, 'nb_launch_ring_fold_phase: pos_in, sums and scratch must be non-null'),
    ('nb_launch_ring_fold_phase', ('fast', 65536, 0, 0, 1, A, B, C, 1099511627776, None), -1, 'nb: need 0 < count <= n_total'),
    ('nb_launch_ring_fold_phase', ('strict', 65536, 0, 16384, 2, A, B, C, 1099511627776, None), -6, 'nb_launch_ring_fold_phase: this shape does not run its step in phases (nb_ring_phased() == 0): use nb_launch_ring_fold'),
    ('nb_launch_ring_fold_phase', ('fast', 4096, 0, 1024, 3, A, B, C, 1099511627776, None), -6, 'nb_launch_ring_fold_phase: this shape does not run its step in phases (nb_ring_phased() == 0): use nb_launch_ring_fold'),
    ('nb_launch_ring_fold_phase', ('fast', 65536, 0, 16384, 4, A, B, C, 0, None), -1, 'nb_launch_ring_fold_phase: scratch smaller than nb_ring_scratch_bytes()'),
    ('nb_launch_ring_fold_phase', ('fast', 65536, 0, 16384, 9, None, B, C, 0, None), -1, 'nb_launch_ring_fold_phase: pos_in, sums and scratch must be non-null'),
    ('nb_launch_ring_fold_phase', ('fast', 65536, 0, 0, 9, A, B, C, 0, None), -1, 'nb_launch_ring_fold_phase: phase must be NB_RING_OWN, NB_RING_REST, NB_RING_SUMS or NB_RING_OWN_READY'),
    ('nb_launch_ring_fold_phase', ('strict', 65536, 0, 16384, 1, A, B, C, 0, None), -6, 'nb_launch_ring_fold_phase: this shape does not run its step in phases (nb_ring_phased() == 0): use nb_launch_ring_fold'),
    # nb_launch_ring_finish
    ('nb_launch_ring_finish', ('fast', 65536, 0, 16384, None, B, C, D, E, None), -1, 'nb_launch_ring_finish: pos_in, pos_out, vel, sums, recv must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_ring_finish', ('fast', 65536, 0, 16384, A, None, C, D, E, None), -1, 'nb_launch_ring_finish: pos_in, pos_out, vel, sums, recv must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_ring_finish', ('fast', 65536, 0, 16384, A, B, None, D, E, None), -1, 'nb_launch_ring_finish: pos_in, pos_out, vel, sums, recv must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_ring_finish', ('fast', 65536, 0, 16384, A, B, C, None, E, None), -1, 'nb_launch_ring_finish: pos_in, pos_out, vel, sums, recv must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_ring_finish', ('fast', 65536, 0, 16384, A, B, C, D, None, None), -1, 'nb_launch_ring_finish: pos_in, pos_out, vel, sums, recv must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_ring_finish', ('fast', 65536, 0, 16384, A, A, C, D, E, None), -1, 'nb_launch_ring_finish: pos_in, pos_out, vel, sums, recv must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_ring_finish', ('fast', 65536, 0, 0, A, B, C, D, E, None), -1, 'nb: need 0 < count <= n_total'),
    ('nb_launch_ring_finish', ('strict', 65536, 0, 16384, A, B, C, D, E, None), -6, 'nb_launch_ring_finish: this shape does not take the pairs form on shards (nb_ring_partners() == 0)'),
    ('nb_launch_ring_finish', (None, 65536, 0, 16384, A, B, C, D, E, None), -6, 'nb_launch_ring_finish: this shape does not take the pairs form on shards (nb_ring_partners() == 0)'),
    ('nb_launch_ring_finish', ('strict', 65536, 0, 0, A, A, C, D, E, None), -1, 'nb_launch_ring_finish: pos_in, pos_out, vel, sums, recv must be non-null and pos_out must not alias pos_in'),
    # nb_launch_ring_finish_phase
    ('nb_launch_ring_finish_phase', ('fast', 65536, 0, 16384, None, B, C, D, E, F, 1099511627776, None), -1, 'nb_launch_ring_finish_phase: pos_in, pos_out, vel, recv, scratch must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_ring_finish_phase', ('fast', 65536, 0, 16384, A, B, C, D, None, F, 1099511627776, None), -1, 'nb_launch_ring_finish_phase: pos_in, pos_out, vel, recv, scratch must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_ring_finish_phase', ('fast', 65536, 0, 16384, A, B, C, D, E, None, 1099511627776, None), -1, 'nb_launch_ring_finish_phase: pos_in, pos_out, vel, recv, scratch must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_ring_finish_phase', ('fast', 65536, 0, 16384, A, A, C, D, E, F, 1099511627776, None), -1, 'nb_launch_ring_finish_phase: pos_in, pos_out, vel, recv, scratch must be non-null and pos_out must not alias pos_in'),
    ('nb_launch_ring_finish_phase', ('fast', 65536, 0, 0, A, B, C, None, E, F, 1099511627776, None), -1, 'nb: need 0 < count <= n_total'),
    ('nb_launch_ring_finish_phase', ('strict', 65536, 0, 16384, A, B, C, None, E, F, 1099511627776, None), -6, 'nb_launch_ring_finish_phase: this shape does not run its step in phases (nb_ring_phased() == 0): use nb_launch_ring_finish'),
    ('nb_launch_ring_finish_phase', ('fast', 65536, 0, 16384, A, B, C, None, E, F, 0, None), -1, 'nb_launch_ring_finish_phase: scratch smaller than nb_ring_scratch_bytes()'),
    ('nb_launch_ring_finish_phase', ('fast', 4096, 0, 1024, A, B, C, D, E, F, 0, None), -6, 'nb_launch_ring_finish_phase: this shape does not run its step in phases (nb_ring_phased() == 0): use nb_launch_ring_finish'),
    # nb_launch_boids_step
    ('nb_launch_boids_step', ('boids', 1024, 0, 1024, None, B, C, D, None), -1, 'nb_launch_boids_step: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_step', ('boids', 1024, 0, 1024, A, None, C, D, None), -1, 'nb_launch_boids_step: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_step', ('boids', 1024, 0, 1024, A, B, None, D, None), -1, 'nb_launch_boids_step: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_step', ('boids', 1024, 0, 1024, A, B, C, None, None), -1, 'nb_launch_boids_step: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_step', ('boids', 1024, 0, 1024, A, B, A, D, None), -1, 'nb_launch_boids_step: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_step', ('boids', 1024, 0, 1024, A, B, C, B, None), -1, 'nb_launch_boids_step: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_step', ('boids', 1024, 0, 0, A, B, C, D, None), -1, 'nb: boids: need count > 0 and [first, first+count) inside n_total'),
    ('nb_launch_boids_step', (None, 1024, 0, 0, A, B, C, D, None), -1, 'nb: boids: need count > 0 and [first, first+count) inside n_total'),
    ('nb_launch_boids_step', ('boids', 0, 0, 0, A, B, C, D, None), -1, 'nb: boids: need count > 0 and [first, first+count) inside n_total'),
    ('nb_launch_boids_step', ('boids', 1024, 512, 513, A, B, C, D, None), -1, 'nb: boids: need count > 0 and [first, first+count) inside n_total'),
    ('nb_launch_boids_step', ('boids_badtile', 1024, 0, 1024, A, B, C, D, None), -1, 'nb: boids params.tile must be 0, 256, 512 or 1024'),
    ('nb_launch_boids_step', ('boids', 16777216, 0, 1024, A, B, C, D, None), -6, 'nb: boids: neighbour counts are kept in binary32 and need n_total < 2^24'),
    ('nb_launch_boids_step', ('boids', 1024, 512, 513, A, B, A, D, None), -1, 'nb_launch_boids_step: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_step', ('boids_badtile', 16777216, 0, 1024, A, B, C, D, None), -1, 'nb: boids params.tile must be 0, 256, 512 or 1024'),
    ('nb_launch_boids_step', ('boids_badtile', 1024, 0, 0, A, B, C, D, None), -1, 'nb: boids: need count > 0 and [first, first+count) inside n_total'),
    # nb_boids_split_scratch_bytes
    ('nb_boids_split_scratch_bytes', ('boids', 16384, 2048), 1573184, None),
    ('nb_boids_split_scratch_bytes', (None, 16384, 2048), 1573184, None),
    ('nb_boids_split_scratch_bytes', ('boids', 1000, 1000), 48080, None),
    ('nb_boids_split_scratch_bytes', ('boids', 16384, 0), 0, None),
    ('nb_boids_split_scratch_bytes', ('boids', 1024, 1025), 0, None),
    ('nb_boids_split_scratch_bytes', ('boids_badtile', 16384, 2048), 0, None),
    ('nb_boids_split_scratch_bytes', ('boids', 16777216, 2048), 0, None),
    # nb_launch_boids_step_split
    ('nb_launch_boids_step_split', ('boids', 16384, 0, 2048, None, B, C, D, E, 1099511627776, None), -1, 'nb_launch_boids_step_split: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_step_split', ('boids', 16384, 0, 2048, A, B, C, D, None, 1099511627776, None), -1, 'nb_launch_boids_step_split: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_step_split', ('boids', 16384, 0, 2048, A, B, A, D, E, 1099511627776, None), -1, 'nb_launch_boids_step_split: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_step_split', ('boids', 16384, 0, 2048, A, B, C, B, E, 1099511627776, None), -1, 'nb_launch_boids_step_split: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_step_split', ('boids', 16384, 0, 0, A, B, C, D, E, 1099511627776, None), -1, 'nb: boids: need count > 0 and [first, first+count) inside n_total'),
    ('nb_launch_boids_step_split', ('boids', 16384, 16000, 2048, A, B, C, D, E, 1099511627776, None), -1, 'nb: boids: need count > 0 and [first, first+count) inside n_total'),
    ('nb_launch_boids_step_split', ('boids_badtile', 16384, 0, 2048, A, B, C, D, E, 1099511627776, None), -1, 'nb: boids params.tile must be 0, 256, 512 or 1024'),
    ('nb_launch_boids_step_split', ('boids', 16777216, 0, 2048, A, B, C, D, E, 1099511627776, None), -6, 'nb: boids: neighbour counts are kept in binary32 and need n_total < 2^24'),
    ('nb_launch_boids_step_split', ('boids', 16384, 0, 2048, A, B, C, D, E, 0, None), -1, 'nb_launch_boids_step_split: scratch smaller than nb_boids_split_scratch_bytes()'),
    ('nb_launch_boids_step_split', (None, 16384, 0, 2048, A, B, C, D, E, 100, None), -1, 'nb_launch_boids_step_split: scratch smaller than nb_boids_split_scratch_bytes()'),
    ('nb_launch_boids_step_split', ('boids', 16384, 0, 0, A, B, C, D, None, 0, None), -1, 'nb_launch_boids_step_split: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_step_split', ('boids_badtile', 16384, 0, 2048, A, B, C, D, E, 0, None), -1, 'nb: boids params.tile must be 0, 256, 512 or 1024'),
    # nb_launch_boids_seen_step
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 1024, None, B, E, F, 8, C, D, None), -1, 'nb_launch_boids_seen_step: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 1024, A, B, None, F, 8, C, D, None), -1, 'nb_launch_boids_seen_step: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 1024, A, B, E, None, 8, C, D, None), -1, 'nb_launch_boids_seen_step: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 1024, A, B, E, F, 8, A, D, None), -1, 'nb_launch_boids_seen_step: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 1024, A, B, E, F, 8, C, B, None), -1, 'nb_launch_boids_seen_step: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 1024, A, B, E, F, 0, C, D, None), -1, 'nb_launch_boids_seen_step: stride must be at least 1'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 1024, A, B, E + 2, F, 8, C, D, None), -1, 'nb_launch_boids_seen_step: seen_count and seen_ids must be 4-byte aligned'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 1024, A, B, E, F + 1, 8, C, D, None), -1, 'nb_launch_boids_seen_step: seen_count and seen_ids must be 4-byte aligned'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 0, A, B, E, F, 8, C, D, None), -1, 'nb: boids: need count > 0 and [first, first+count) inside n_total'),
    ('nb_launch_boids_seen_step', (None, 1024, 1000, 25, A, B, E, F, 8, C, D, None), -1, 'nb: boids: need count > 0 and [first, first+count) inside n_total'),
    ('nb_launch_boids_seen_step', ('boids_badtile', 1024, 0, 1024, A, B, E, F, 8, C, D, None), -1, 'nb: boids params.tile must be 0, 256, 512 or 1024'),
    ('nb_launch_boids_seen_step', ('boids', 16777216, 0, 1024, A, B, E, F, 8, C, D, None), -6, 'nb: boids: neighbour counts are kept in binary32 and need n_total < 2^24'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 1024, A, B, C + 16, F, 8, C, D, None), -1, 'nb_launch_boids_seen_step: the outputs must not alias the lists'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 1024, A, B, E, D + 1024, 8, C, D, None), -1, 'nb_launch_boids_seen_step: the outputs must not alias the lists'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 512, 512, A, B, C + 8192, F, 8, C, D, None), -1, 'nb_launch_boids_seen_step: the outputs must not alias the lists'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 1024, A, B, E + 2, F, 0, C, D, None), -1, 'nb_launch_boids_seen_step: stride must be at least 1'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 0, A, B, E + 2, F, 8, C, D, None), -1, 'nb_launch_boids_seen_step: seen_count and seen_ids must be 4-byte aligned'),
    ('nb_launch_boids_seen_step', ('boids', 1024, 0, 0, A, B, C + 16, F, 8, C, D, None), -1, 'nb: boids: need count > 0 and [first, first+count) inside n_total'),
    # nb_launch_seen
    ('nb_launch_seen', (4, 8, None, B, C, D, E, F, None), -1, 'nb_launch_seen: ids_rows, seen_count and seen_ids must be non-null'),
    ('nb_launch_seen', (4, 8, A, B, None, D, E, F, None), -1, 'nb_launch_seen: ids_rows, seen_count and seen_ids must be non-null'),
    ('nb_launch_seen', (4, 8, A, B, C, None, E, F, None), -1, 'nb_launch_seen: ids_rows, seen_count and seen_ids must be non-null'),
    ('nb_launch_seen', (4, 8, A, None, C, D, E, F, None), -1, 'nb_launch_seen: seen_depth needs depth_rows'),
    ('nb_launch_seen', (4, 8, A + 2, B, C, D, E, F, None), -1, 'nb_launch_seen: ids_rows and depth_rows must be 4-byte aligned'),
    ('nb_launch_seen', (4, 8, A, B + 1, C, D, E, F, None), -1, 'nb_launch_seen: ids_rows and depth_rows must be 4-byte aligned'),
    ('nb_launch_seen', (4, 0, A, B, C, D, E, F, None), -1, 'nb_launch_seen: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_launch_seen', (4, 4097, A, B, C, D, E, F, None), -1, 'nb_launch_seen: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_launch_seen', (4, 8, A, B, C + 2, D, E, F, None), -1, 'nb_launch_seen: the outputs must be 4-byte aligned'),
    ('nb_launch_seen', (4, 8, A, B, C, D, E, F + 1, None), -1, 'nb_launch_seen: the outputs must be 4-byte aligned'),
    ('nb_launch_seen', (4, 8, A, B, C, C, E, F, None), -1, 'nb_launch_seen: the outputs must not alias each other or an input'),
    ('nb_launch_seen', (4, 8, A, B, C, D, E, D + 64, None), -1, 'nb_launch_seen: the outputs must not alias each other or an input'),
    ('nb_launch_seen', (4, 8, A, B, C, A + 64, None, None, None), -1, 'nb_launch_seen: the outputs must not alias each other or an input'),
    ('nb_launch_seen', (4, 8, A, B, B, D, None, None, None), -1, 'nb_launch_seen: the outputs must not alias each other or an input'),
    ('nb_launch_seen', (0, 8, A, B, C, D, E, F, None), 0, None),
    ('nb_launch_seen', (0, 0, A, B, C, D, E, F, None), -1, 'nb_launch_seen: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_launch_seen', (4, 0, A, None, C, D, E, F, None), -1, 'nb_launch_seen: seen_depth needs depth_rows'),
    ('nb_launch_seen', (4, 0, A + 2, B, C, D, E, F, None), -1, 'nb_launch_seen: ids_rows and depth_rows must be 4-byte aligned'),
    ('nb_launch_seen', (4, 0, A, B, C + 2, C + 2, E, F, None), -1, 'nb_launch_seen: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_launch_seen', (4, 8, A, B, C + 2, C + 2, E, F, None), -1, 'nb_launch_seen: the outputs must be 4-byte aligned'),
    # nb_launch_instances
    ('nb_launch_instances', (0, A, B, C, None), -1, 'nb_launch_instances: bad argument'),
    ('nb_launch_instances', (4, None, B, C, None), -1, 'nb_launch_instances: bad argument'),
    ('nb_launch_instances', (4, A, None, C, None), -1, 'nb_launch_instances: bad argument'),
    ('nb_launch_instances', (4, A, B, None, None), -1, 'nb_launch_instances: bad argument'),
    # nb_launch_cameras
    ('nb_launch_cameras', (0, A, B, C, D, E, None), -1, 'nb_launch_cameras: bad argument'),
    ('nb_launch_cameras', (4, None, B, C, D, E, None), -1, 'nb_launch_cameras: bad argument'),
    ('nb_launch_cameras', (4, A, None, C, D, E, None), -1, 'nb_launch_cameras: bad argument'),
    ('nb_launch_cameras', (4, A, B, None, D, E, None), -1, 'nb_launch_cameras: bad argument'),
    ('nb_launch_cameras', (4, A, B, C, None, E, None), -1, 'nb_launch_cameras: bad argument'),
    ('nb_launch_cameras', (4, A, B, C, D, None, None), -1, 'nb_launch_cameras: bad argument'),
    # nb_launch_random_step
    ('nb_launch_random_step', (0, 0, A, B, 1, 2, None), -1, 'nb_launch_random_step: bad argument'),
    ('nb_launch_random_step', (0, 4, None, B, 1, 2, None), -1, 'nb_launch_random_step: bad argument'),
    ('nb_launch_random_step', (0, 4, A, None, 1, 2, None), -1, 'nb_launch_random_step: bad argument'),
    # nb_launch_pack
    ('nb_launch_pack', (0, A, B, None), -1, 'nb_launch_pack: bad argument'),
    ('nb_launch_pack', (4, None, B, None), -1, 'nb_launch_pack: bad argument'),
    ('nb_launch_pack', (4, A, None, None), -1, 'nb_launch_pack: bad argument'),
    # nb_launch_unpack
    ('nb_launch_unpack', (0, A, B, None), -1, 'nb_launch_unpack: bad argument'),
    ('nb_launch_unpack', (4, None, B, None), -1, 'nb_launch_unpack: bad argument'),
    ('nb_launch_unpack', (4, A, None, None), -1, 'nb_launch_unpack: bad argument'),
    # nb_launch_eyes
    ('nb_launch_eyes', (16, 0, 4, None, B, 8, 0, C, D, None), -1, 'nb_launch_eyes: null argument'),
    ('nb_launch_eyes', (16, 0, 4, A, None, 8, 0, C, D, None), -1, 'nb_launch_eyes: null argument'),
    ('nb_launch_eyes', (16, 0, 4, A + 8, B, 8, 0, C, D, None), -1, 'nb_launch_eyes: cams_16 and inst_16n must be 16-byte aligned'),
    ('nb_launch_eyes', (16, 0, 4, A, B + 4, 8, 0, C, D, None), -1, 'nb_launch_eyes: cams_16 and inst_16n must be 16-byte aligned'),
    ('nb_launch_eyes', (16, 0, 4, A, B, 0, 0, C, D, None), -1, 'nb_launch_eyes: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_launch_eyes', (16, 0, 4, A, B, 4097, 0, C, D, None), -1, 'nb_launch_eyes: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_launch_eyes', (16, 14, 4, A, B, 8, 0, C, D, None), -1, 'nb_launch_eyes: eyes [first, first + count) exceed the set'),
    ('nb_launch_eyes', (16, 0xffffffff, 2, A, B, 8, 0, C, D, None), -1, 'nb_launch_eyes: eyes [first, first + count) exceed the set'),
    ('nb_launch_eyes', (16, 0, 4, A, B, 8, 2, C, D, None), -1, 'nb_launch_eyes: unknown flag bits'),
    ('nb_launch_eyes', (16, 0, 4, A, B, 8, 0, None, None, None), -1, 'nb_launch_eyes: ids and depth are both NULL'),
    ('nb_launch_eyes', (16, 0, 4, A, B, 8, 0, C, C, None), -1, 'nb_launch_eyes: the outputs must not alias each other or an input'),
    ('nb_launch_eyes', (16, 0, 4, A, B, 8, 0, C, C + 64, None), -1, 'nb_launch_eyes: the outputs must not alias each other or an input'),
    ('nb_launch_eyes', (16, 0, 4, A, B, 8, 1, A + 128, None, None), -1, 'nb_launch_eyes: the outputs must not alias each other or an input'),
    ('nb_launch_eyes', (16, 0, 4, A, B, 8, 1, None, B + 1000, None), -1, 'nb_launch_eyes: the outputs must not alias each other or an input'),
    ('nb_launch_eyes', (16, 0, 0, A, B, 8, 1, C, D, None), 0, None),
    ('nb_launch_eyes', (16, 16, 0, A, B, 8, 0, C + 1, None, None), 0, None),
    ('nb_launch_eyes', (16, 0, 0, A, B, 8, 0, None, None, None), -1, 'nb_launch_eyes: ids and depth are both NULL'),
    ('nb_launch_eyes', (16, 0, 4, None, B + 4, 0, 2, None, None, None), -1, 'nb_launch_eyes: null argument'),
    ('nb_launch_eyes', (16, 14, 4, A, B + 4, 0, 2, None, None, None), -1, 'nb_launch_eyes: cams_16 and inst_16n must be 16-byte aligned'),
    ('nb_launch_eyes', (16, 14, 4, A, B, 0, 2, None, None, None), -1, 'nb_launch_eyes: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_launch_eyes', (16, 14, 4, A, B, 8, 2, None, None, None), -1, 'nb_launch_eyes: eyes [first, first + count) exceed the set'),
    ('nb_launch_eyes', (16, 0, 4, A, B, 8, 2, None, None, None), -1, 'nb_launch_eyes: unknown flag bits'),
    # nb_launch_eyes_colour
    ('nb_launch_eyes_colour', (16, 0, 4, None, B, 8, 0, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_colour: null argument'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, None, 8, 0, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_colour: null argument'),
    ('nb_launch_eyes_colour', (16, 0, 4, A + 8, B, 8, 0, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_colour: cams_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, G + 4, 2, 2, C, D, E, F, None), -1, 'nb_launch_eyes_colour: cams_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, None, 0, 0, C, D, E + 8, F, None), -1, 'nb_launch_eyes_colour: cams_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, G, 0, 2, C, D, E, F, None), -1, 'nb_launch_eyes_colour: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, G, 2, 2049, C, D, E, F, None), -1, 'nb_launch_eyes_colour: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 0, 0, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_colour: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 4097, 0, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_colour: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_launch_eyes_colour', (16, 14, 4, A, B, 8, 0, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_colour: eyes [first, first + count) exceed the set'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 4, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_colour: unknown flag bits'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, None, 0, 0, C, D, None, None, None), -1, 'nb_launch_eyes_colour: rgba and bgra8 are both NULL (ids and depth alone: nb_eyes / nb_launch_eyes)'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, None, 0, 0, None, None, None, None, None), -1, 'nb_launch_eyes_colour: rgba and bgra8 are both NULL (ids and depth alone: nb_eyes / nb_launch_eyes)'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, None, 0, 0, C + 2, D, E, F, None), -1, 'nb_launch_eyes_colour: the outputs must be 4-byte aligned'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, None, 0, 0, C, D + 1, E, F, None), -1, 'nb_launch_eyes_colour: the outputs must be 4-byte aligned'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, None, 0, 0, C, D, E, F + 2, None), -1, 'nb_launch_eyes_colour: the outputs must be 4-byte aligned'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, None, 0, 0, C, D, E, E, None), -1, 'nb_launch_eyes_colour: the outputs must not alias each other or an input'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, None, 0, 0, C, D, E, E + 64, None), -1, 'nb_launch_eyes_colour: the outputs must not alias each other or an input'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, None, 0, 0, C, D, B + 256, F, None), -1, 'nb_launch_eyes_colour: the outputs must not alias each other or an input'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, G, 4, 4, C, D, E, G + 128, None), -1, 'nb_launch_eyes_colour: the outputs must not alias each other or an input'),
    ('nb_launch_eyes_colour', (16, 0, 0, A, B, 8, 1, G, 4, 4, C, D, E, F, None), 0, None),
    ('nb_launch_eyes_colour', (16, 0, 4, None, B, 8, 0, G + 4, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_colour: null argument'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 0, 0, G + 4, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_colour: cams_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 0, 0, G, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_colour: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_launch_eyes_colour', (16, 14, 4, A, B, 8, 4, None, 0, 0, C, D, None, None, None), -1, 'nb_launch_eyes_colour: eyes [first, first + count) exceed the set'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, None, 0, 0, C + 2, C + 2, None, None, None), -1, 'nb_launch_eyes_colour: rgba and bgra8 are both NULL (ids and depth alone: nb_eyes / nb_launch_eyes)'),
    ('nb_launch_eyes_colour', (16, 0, 4, A, B, 8, 0, None, 0, 0, C + 2, C + 2, None, F, None), -1, 'nb_launch_eyes_colour: the outputs must be 4-byte aligned'),
    # nb_launch_eyes_msaa
    ('nb_launch_eyes_msaa', (16, 0, 4, None, B, 8, 0, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_msaa: null argument'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, None, 8, 0, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_msaa: null argument'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A + 8, B, 8, 0, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_msaa: cams_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, G + 4, 2, 2, C, D, E, F, None), -1, 'nb_launch_eyes_msaa: cams_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, None, 0, 0, C, D, E + 8, F, None), -1, 'nb_launch_eyes_msaa: cams_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, G, 0, 2, C, D, E, F, None), -1, 'nb_launch_eyes_msaa: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, G, 2, 2049, C, D, E, F, None), -1, 'nb_launch_eyes_msaa: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 0, 0, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_msaa: width must be 1 .. NB_EYES_MSAA_MAX_WIDTH (2048)'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 2049, 0, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_msaa: width must be 1 .. NB_EYES_MSAA_MAX_WIDTH (2048)'),
    ('nb_launch_eyes_msaa', (16, 14, 4, A, B, 8, 0, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_msaa: eyes [first, first + count) exceed the set'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 4, None, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_msaa: unknown flag bits'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, None, 0, 0, None, None, None, None, None), -1, 'nb_launch_eyes_msaa: ids8, depth8, rgba and bgra8 are all NULL'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, None, 0, 0, C + 2, D, E, F, None), -1, 'nb_launch_eyes_msaa: the outputs must be 4-byte aligned'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, None, 0, 0, C, D + 1, E, F, None), -1, 'nb_launch_eyes_msaa: the outputs must be 4-byte aligned'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, None, 0, 0, C, D, E, F + 2, None), -1, 'nb_launch_eyes_msaa: the outputs must be 4-byte aligned'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, None, 0, 0, C, D, E, E, None), -1, 'nb_launch_eyes_msaa: the outputs must not alias each other or an input'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, None, 0, 0, C, D, E, E + 64, None), -1, 'nb_launch_eyes_msaa: the outputs must not alias each other or an input'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, None, 0, 0, C, D, B + 256, F, None), -1, 'nb_launch_eyes_msaa: the outputs must not alias each other or an input'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, G, 4, 4, C, D, E, G + 128, None), -1, 'nb_launch_eyes_msaa: the outputs must not alias each other or an input'),
    ('nb_launch_eyes_msaa', (16, 0, 0, A, B, 8, 1, G, 4, 4, C, D, E, F, None), 0, None),
    ('nb_launch_eyes_msaa', (16, 0, 4, None, B, 8, 0, G + 4, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_msaa: null argument'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 0, 0, G + 4, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_msaa: cams_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 0, 0, G, 0, 0, C, D, E, F, None), -1, 'nb_launch_eyes_msaa: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_launch_eyes_msaa', (16, 14, 4, A, B, 8, 4, None, 0, 0, C, D, None, None, None), -1, 'nb_launch_eyes_msaa: eyes [first, first + count) exceed the set'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, None, 0, 0, C + 2, C + 2, None, None, None), -1, 'nb_launch_eyes_msaa: the outputs must be 4-byte aligned'),
    ('nb_launch_eyes_msaa', (16, 0, 4, A, B, 8, 0, None, 0, 0, C + 2, C + 2, None, F, None), -1, 'nb_launch_eyes_msaa: the outputs must be 4-byte aligned'),
    # nb_frame_scratch_bytes
    ('nb_frame_scratch_bytes', (64, 32), 16384, None),
    ('nb_frame_scratch_bytes', (4096, 4096), 134217728, None),
    ('nb_frame_scratch_bytes', (0, 32), 0, None),
    ('nb_frame_scratch_bytes', (64, 4097), 0, None),
    # nb_frame_msaa_scratch_bytes
    ('nb_frame_msaa_scratch_bytes', (64, 32), 131072, None),
    ('nb_frame_msaa_scratch_bytes', (2048, 2048), 268435456, None),
    ('nb_frame_msaa_scratch_bytes', (2049, 32), 0, None),
    ('nb_frame_msaa_scratch_bytes', (64, 0), 0, None),
    # nb_launch_frame
    ('nb_launch_frame', (16, None, B, 8, 8, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame: null argument'),
    ('nb_launch_frame', (16, A, None, 8, 8, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame: null argument'),
    ('nb_launch_frame', (16, A, B, 8, 8, 0, None, 0, 0, None, C, D, E, F, None), -1, 'nb_launch_frame: null argument'),
    ('nb_launch_frame', (0, A, None, 8, 8, 0, None, 0, 0, H, None, None, None, None, None), -1, 'nb_launch_frame: ids, depth, rgba and bgra8 are all NULL'),
    ('nb_launch_frame', (16, A + 4, B, 8, 8, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame: cam_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_frame', (16, A, B + 8, 8, 8, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame: cam_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_frame', (16, A, B, 8, 8, 0, G + 4, 2, 2, H, C, D, E, F, None), -1, 'nb_launch_frame: cam_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_frame', (16, A, B, 8, 8, 0, None, 0, 0, H, C, D, E + 4, F, None), -1, 'nb_launch_frame: cam_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_frame', (16, A, B, 8, 8, 0, None, 0, 0, H + 4, C, D, E, F, None), -1, 'nb_launch_frame: scratch must be 8-byte aligned'),
    ('nb_launch_frame', (16, A, B, 8, 8, 0, G, 2, 0, H, C, D, E, F, None), -1, 'nb_launch_frame: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_launch_frame', (16, A, B, 8, 8, 0, G, 2049, 2, H, C, D, E, F, None), -1, 'nb_launch_frame: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_launch_frame', (16, A, B, 0, 8, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame: width and height must be 1 .. NB_FRAME_MAX_DIM (4096)'),
    ('nb_launch_frame', (16, A, B, 8, 0, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame: width and height must be 1 .. NB_FRAME_MAX_DIM (4096)'),
    ('nb_launch_frame', (16, A, B, 4097, 8, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame: width and height must be 1 .. NB_FRAME_MAX_DIM (4096)'),
    ('nb_launch_frame', (16, A, B, 8, 4097, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame: width and height must be 1 .. NB_FRAME_MAX_DIM (4096)'),
    ('nb_launch_frame', (16, A, B, 8, 8, 1, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame: flags must be 0'),
    ('nb_launch_frame', (16, A, B, 8, 8, 0, None, 0, 0, H, None, None, None, None, None), -1, 'nb_launch_frame: ids, depth, rgba and bgra8 are all NULL'),
    ('nb_launch_frame', (16, A, B, 8, 8, 0, None, 0, 0, H, C + 2, D, E, F, None), -1, 'nb_launch_frame: the outputs must be 4-byte aligned'),
    ('nb_launch_frame', (16, A, B, 8, 8, 0, None, 0, 0, H, C, D, E, F + 1, None), -1, 'nb_launch_frame: the outputs must be 4-byte aligned'),
    ('nb_launch_frame', (16, A, B, 8, 8, 0, None, 0, 0, H, C, C, E, F, None), -1, 'nb_launch_frame: the outputs must not alias each other, an input or the scratch'),
    ('nb_launch_frame', (16, A, B, 8, 8, 0, None, 0, 0, H, C, D, E, H + 64, None), -1, 'nb_launch_frame: the outputs must not alias each other, an input or the scratch'),
    ('nb_launch_frame', (16, A, B, 8, 8, 0, None, 0, 0, H, A + 32, D, E, F, None), -1, 'nb_launch_frame: the outputs must not alias each other, an input or the scratch'),
    ('nb_launch_frame', (16, A, B, 8, 8, 0, G, 4, 4, H, C, D, G + 32, F, None), -1, 'nb_launch_frame: the outputs must not alias each other, an input or the scratch'),
    ('nb_launch_frame', (16, None, B + 8, 8, 8, 0, None, 0, 0, H + 4, C, D, E, F, None), -1, 'nb_launch_frame: null argument'),
    ('nb_launch_frame', (16, A, B + 8, 8, 8, 0, None, 0, 0, H + 4, C, D, E, F, None), -1, 'nb_launch_frame: cam_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_frame', (16, A, B, 0, 8, 0, G, 0, 0, H + 4, C, D, E, F, None), -1, 'nb_launch_frame: scratch must be 8-byte aligned'),
    ('nb_launch_frame', (16, A, B, 0, 8, 1, G, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_launch_frame', (16, A, B, 0, 8, 1, None, 0, 0, H, None, None, None, None, None), -1, 'nb_launch_frame: width and height must be 1 .. NB_FRAME_MAX_DIM (4096)'),
    ('nb_launch_frame', (16, A, B, 8, 8, 1, None, 0, 0, H, None, None, None, None, None), -1, 'nb_launch_frame: flags must be 0'),
    # nb_launch_frame_msaa
    ('nb_launch_frame_msaa', (16, None, B, 8, 8, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame_msaa: null argument'),
    ('nb_launch_frame_msaa', (16, A, None, 8, 8, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame_msaa: null argument'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 0, None, 0, 0, None, C, D, E, F, None), -1, 'nb_launch_frame_msaa: null argument'),
    ('nb_launch_frame_msaa', (0, A, None, 8, 8, 0, None, 0, 0, H, None, None, None, None, None), -1, 'nb_launch_frame_msaa: ids8, depth8, rgba and bgra8 are all NULL'),
    ('nb_launch_frame_msaa', (16, A + 4, B, 8, 8, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame_msaa: cam_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_frame_msaa', (16, A, B + 8, 8, 8, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame_msaa: cam_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 0, G + 4, 2, 2, H, C, D, E, F, None), -1, 'nb_launch_frame_msaa: cam_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 0, None, 0, 0, H, C, D, E + 4, F, None), -1, 'nb_launch_frame_msaa: cam_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 0, None, 0, 0, H + 4, C, D, E, F, None), -1, 'nb_launch_frame_msaa: scratch must be 8-byte aligned'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 0, G, 2, 0, H, C, D, E, F, None), -1, 'nb_launch_frame_msaa: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 0, G, 2049, 2, H, C, D, E, F, None), -1, 'nb_launch_frame_msaa: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_launch_frame_msaa', (16, A, B, 0, 8, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame_msaa: width and height must be 1 .. NB_FRAME_MSAA_MAX_DIM (2048)'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 0, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame_msaa: width and height must be 1 .. NB_FRAME_MSAA_MAX_DIM (2048)'),
    ('nb_launch_frame_msaa', (16, A, B, 2049, 8, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame_msaa: width and height must be 1 .. NB_FRAME_MSAA_MAX_DIM (2048)'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 2049, 0, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame_msaa: width and height must be 1 .. NB_FRAME_MSAA_MAX_DIM (2048)'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 1, None, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame_msaa: flags must be 0'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 0, None, 0, 0, H, None, None, None, None, None), -1, 'nb_launch_frame_msaa: ids8, depth8, rgba and bgra8 are all NULL'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 0, None, 0, 0, H, C + 2, D, E, F, None), -1, 'nb_launch_frame_msaa: the outputs must be 4-byte aligned'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 0, None, 0, 0, H, C, D, E, F + 1, None), -1, 'nb_launch_frame_msaa: the outputs must be 4-byte aligned'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 0, None, 0, 0, H, C, C, E, F, None), -1, 'nb_launch_frame_msaa: the outputs must not alias each other, an input or the scratch'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 0, None, 0, 0, H, C, D, E, H + 64, None), -1, 'nb_launch_frame_msaa: the outputs must not alias each other, an input or the scratch'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 0, None, 0, 0, H, A + 32, D, E, F, None), -1, 'nb_launch_frame_msaa: the outputs must not alias each other, an input or the scratch'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 0, G, 4, 4, H, C, D, G + 32, F, None), -1, 'nb_launch_frame_msaa: the outputs must not alias each other, an input or the scratch'),
    ('nb_launch_frame_msaa', (16, None, B + 8, 8, 8, 0, None, 0, 0, H + 4, C, D, E, F, None), -1, 'nb_launch_frame_msaa: null argument'),
    ('nb_launch_frame_msaa', (16, A, B + 8, 8, 8, 0, None, 0, 0, H + 4, C, D, E, F, None), -1, 'nb_launch_frame_msaa: cam_16, inst_16n, skin and rgba must be 16-byte aligned'),
    ('nb_launch_frame_msaa', (16, A, B, 0, 8, 0, G, 0, 0, H + 4, C, D, E, F, None), -1, 'nb_launch_frame_msaa: scratch must be 8-byte aligned'),
    ('nb_launch_frame_msaa', (16, A, B, 0, 8, 1, G, 0, 0, H, C, D, E, F, None), -1, 'nb_launch_frame_msaa: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_launch_frame_msaa', (16, A, B, 0, 8, 1, None, 0, 0, H, None, None, None, None, None), -1, 'nb_launch_frame_msaa: width and height must be 1 .. NB_FRAME_MSAA_MAX_DIM (2048)'),
    ('nb_launch_frame_msaa', (16, A, B, 8, 8, 1, None, 0, 0, H, None, None, None, None, None), -1, 'nb_launch_frame_msaa: flags must be 0'),
    # nb_eyes
    ('nb_eyes', (None, 0, 4, A, B, 8, 0, C, D), -1, 'nb_eyes: ctx is null'),
    # nb_eyes_colour
    ('nb_eyes_colour', (None, 0, 4, A, B, 8, 0, C, D, E, F), -1, 'nb_eyes_colour: ctx is null'),
    # nb_eyes_msaa
    ('nb_eyes_msaa', (None, 0, 4, A, B, 8, 0, C, D, E, F), -1, 'nb_eyes_msaa: ctx is null'),
    # nb_eyes_seen
    ('nb_eyes_seen', (None, 0, 4, A, B, 8, 0, C, D, E, F), -1, 'nb_eyes_seen: ctx is null'),
    # nb_frame
    ('nb_frame', (None, A, 8, 8, 0, C, D, E, F), -1, 'nb_frame: ctx is null'),
    # nb_frame_msaa
    ('nb_frame_msaa', (None, A, 8, 8, 0, C, D, E, F), -1, 'nb_frame_msaa: ctx is null'),
    # nb_step_boids_seen
    ('nb_step_boids_seen', (None, 1, None, A, B, 8, 0), -1, 'nb_step_boids_seen: ctx is null'),
    # The base entries of the context without one (recorded before the context's preamble became one helper); "two faults": a second
    # argument the entry would refuse, which it never gets to.
    # nb_upload
    ('nb_upload', (None, A, B), -1, 'nb_upload: ctx is null'),
    ('nb_upload', (None, None, None), -1, 'nb_upload: ctx is null'),   # two faults
    # nb_step
    ('nb_step', (None, 1), -1, 'nb_step: ctx is null'),
    ('nb_step', (None, 0), -1, 'nb_step: ctx is null'),
    # nb_step_boids
    ('nb_step_boids', (None, 1, None), -1, 'nb_step_boids: ctx is null'),
    ('nb_step_boids', (None, 1, 'boids'), -1, 'nb_step_boids: ctx is null'),
    ('nb_step_boids', (None, 1, 'boids_badtile'), -1, 'nb_step_boids: ctx is null'),   # two faults
    # nb_step_random
    ('nb_step_random', (None, 1, 7), -1, 'nb_step_random: ctx is null'),
    # nb_device_state
    ('nb_device_state', (None, None, None, None), -1, 'nb_device_state: ctx is null'),
    # nb_cameras
    ('nb_cameras', (None, A, B, C), -1, 'nb_cameras: ctx is null'),
    ('nb_cameras', (None, None, B, C), -1, 'nb_cameras: ctx is null'),   # two faults
    ('nb_cameras', (None, None, None, None), -1, 'nb_cameras: ctx is null'),   # two faults
    # nb_camera_at
    ('nb_camera_at', (None, A, B, C, D, E), -1, 'nb_camera_at: ctx is null'),
    ('nb_camera_at', (None, A, B, C, D, None), -1, 'nb_camera_at: ctx is null'),   # two faults
    # nb_eyes_skin
    ('nb_eyes_skin', (None, A, 2, 2), -1, 'nb_eyes_skin: ctx is null'),
    ('nb_eyes_skin', (None, None, 0, 0), -1, 'nb_eyes_skin: ctx is null'),
    ('nb_eyes_skin', (None, A, 0, 2049), -1, 'nb_eyes_skin: ctx is null'),   # two faults
    # nb_sync
    ('nb_sync', (None,), -1, 'nb_sync: ctx is null'),
    # nb_download
    ('nb_download', (None, A, B, C), -1, 'nb_download: ctx is null'),
    ('nb_download', (None, None, None, None), -1, 'nb_download: ctx is null'),
]
BASE_CONTEXT_ENTRIES = {"nb_upload", "nb_step", "nb_step_boids", "nb_step_random", "nb_device_state", "nb_cameras", "nb_camera_at",
                        "nb_eyes_skin", "nb_sync", "nb_download"}


def test_no_row_expects_the_device():
    assert all(status != _lib.NB_ERR_NO_DEVICE and status != _lib.NB_ERR_HIP for _, _, status, _ in ROWS)
    entries = {entry for entry, _, _, _ in ROWS}
    stateless = {name for name in _lib.PROTOTYPES if name.startswith("nb_launch_") or "scratch_bytes" in name}
    assert stateless - entries == {"nb_launch_status"}
    assert {"nb_ring_partners", "nb_ring_phased", "nb_eyes", "nb_eyes_colour", "nb_eyes_msaa", "nb_frame", "nb_frame_msaa"} <= entries
    assert BASE_CONTEXT_ENTRIES <= entries
    # a context entry's rows here have no context: with one, the call would go on to the device
    assert all(args[0] is None for entry, args, _, _ in ROWS if entry in BASE_CONTEXT_ENTRIES)


@pytest.mark.parametrize("entry", sorted({entry for entry, _, _, _ in ROWS}))
def test_refusals_are_the_recorded_ones(nb, entry):
    lib = _lib.load()
    for name, args, status, message in ROWS:
        if name != entry:
            continue
        held = [PARAMS[a]() if isinstance(a, str) else a for a in args]   # (keeps the parameter blocks alive over the call)
        call = [ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in held]
        assert lib.nb_init_state(0, 0, None, None) == _lib.NB_ERR_INVALID   # a message of another entry's: "none written" shows
        untouched = _lib.last_error()
        got = getattr(lib, name)(*call)
        assert got == status, (name, args, _lib.last_error())
        if message is not None:
            assert _lib.last_error() == message, (name, args)
        elif name not in SIZE_QUERIES:
            assert _lib.last_error() == untouched, (name, args)
