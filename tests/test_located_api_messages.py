"""What the two stateless located entries (nb_seen_located_launch, nb_nbody_located_step_launch) answer to
arguments they must refuse: the status and the full nb_last_error() text, as a table in the manner of test_launch_api_messages.py.

Each row is an entry, arguments that fail validation before anything touches the device (the device addresses are fake and never
dereferenced; `up` and the camera constant are real host arrays, which the checks read), the status and the message.  A message of
None means the call writes none (count == 0 succeeds without work).  Rows marked "two faults" have two arguments wrong at once and
pin which check comes first.  No row may reach the device: on a machine with a GPU the fake addresses would be used.
"""
import ctypes

import pytest

from nenbody_amd import _lib

A, B, C, D, E, F, G, H = (0x100000 * k for k in range(1, 9))   # fake device addresses, 1 MiB apart, 16-byte aligned
R = H + 0x80000                                               # one more, half a MiB behind H


class Floats16(ctypes.Structure):
    """up to 16 floats of host memory, passed by reference"""
    _fields_ = [("m", ctypes.c_float * 16)]

    def __init__(self, *values):
        super().__init__((ctypes.c_float * 16)(*values))


# the blocks a row names: nb_params' defaults; `up`; a camera constant of nb_camera_constant's shape, and constants that L6 refuses
PARAMS = {
    "strict": lambda: _lib.default_params(),
    "up": lambda: Floats16(0, 0, 1),
    "cp": lambda: Floats16(1.25, 0, 0, 0, 0, 1300, 0, 0, 0, 0, -1.0001, -1, 0, 0, -1.0001, 0),
    "cp_ortho": lambda: Floats16(1.25, 0, 0, 0, 0, 1300, 0, 0, 0, 0, -1.0001, 0, 0, 0, -1.0001, 1),
    "cp_15": lambda: Floats16(1.25, 0, 0, 0, 0, 1300, 0, 0, 0, 0, -1.0001, -1, 0, 0, -1.0001, 1),
    "cp_0": lambda: Floats16(0, 0, 0, 0, 0, 1300, 0, 0, 0, 0, -1.0001, -1, 0, 0, -1.0001, 0),
    "cp_14": lambda: Floats16(1.25, 0, 0, 0, 0, 1300, 0, 0, 0, 0, -1.0001, -1, 0, 0, 0, 0),
}

# (entry, arguments, status, message)
ROWS = [
    ('nb_seen_located_launch', (4, 8, None, B, C, D, E, F, G, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: every argument but seen_col and stream must be non-null'),
    ('nb_seen_located_launch', (4, 8, A, None, C, D, E, F, G, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: every argument but seen_col and stream must be non-null'),
    ('nb_seen_located_launch', (4, 8, A, B, None, D, E, F, G, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: every argument but seen_col and stream must be non-null'),
    ('nb_seen_located_launch', (4, 8, A, B, C, None, E, F, G, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: every argument but seen_col and stream must be non-null'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, None, F, G, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: every argument but seen_col and stream must be non-null'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, None, G, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: every argument but seen_col and stream must be non-null'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, None, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: every argument but seen_col and stream must be non-null'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, None, 'cp', H, R, None), -1, 'nb_seen_located_launch: every argument but seen_col and stream must be non-null'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', None, H, R, None), -1, 'nb_seen_located_launch: every argument but seen_col and stream must be non-null'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', 'cp', H, None, None), -1, 'nb_seen_located_launch: every argument but seen_col and stream must be non-null'),
    ('nb_seen_located_launch', (4, 8, A + 2, B, C, D, E, F, G, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: the rows, the lists and seen_col must be 4-byte aligned'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E + 1, F, G, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: the rows, the lists and seen_col must be 4-byte aligned'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', 'cp', H + 2, R, None), -1, 'nb_seen_located_launch: the rows, the lists and seen_col must be 4-byte aligned'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F + 4, G, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: eyes, dirs and seen_rel must be 16-byte aligned'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G + 8, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: eyes, dirs and seen_rel must be 16-byte aligned'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', 'cp', H, R + 4, None), -1, 'nb_seen_located_launch: eyes, dirs and seen_rel must be 16-byte aligned'),
    ('nb_seen_located_launch', (4, 0, A, B, C, D, E, F, G, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_seen_located_launch', (4, 4097, A, B, C, D, E, F, G, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', 'cp_ortho', H, R, None), -1, 'nb_seen_located_launch: cp16 cannot be inverted: cp16[11] must be -1 (a perspective constant as nb_camera_constant forms it)'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', 'cp_15', H, R, None), -1, 'nb_seen_located_launch: cp16 cannot be inverted: cp16[15] must be 0 (a perspective constant as nb_camera_constant forms it)'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', 'cp_0', H, R, None), -1, 'nb_seen_located_launch: cp16 cannot be inverted: cp16[0] must not be 0 (a perspective constant as nb_camera_constant forms it)'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', 'cp_14', H, R, None), -1, 'nb_seen_located_launch: cp16 cannot be inverted: cp16[14] must not be 0 (a perspective constant as nb_camera_constant forms it)'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', 'cp', R, R, None), -1, 'nb_seen_located_launch: the outputs must not alias each other or an input'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', 'cp', R + 384, R, None), -1, 'nb_seen_located_launch: the outputs must not alias each other or an input'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', 'cp', H, A + 112, None), -1, 'nb_seen_located_launch: the outputs must not alias each other or an input'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', 'cp', C + 12, R, None), -1, 'nb_seen_located_launch: the outputs must not alias each other or an input'),
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', 'cp', None, G + 48, None), -1, 'nb_seen_located_launch: the outputs must not alias each other or an input'),
    ('nb_seen_located_launch', (0, 8, A, B, C, D, E, F, G, 'up', 'cp', H, R, None), 0, None),
    ('nb_seen_located_launch', (0, 8, A, B, C, D, E, F, G, 'up', 'cp_ortho', H, R, None), -1, 'nb_seen_located_launch: cp16 cannot be inverted: cp16[11] must be -1 (a perspective constant as nb_camera_constant forms it)'),
    ('nb_seen_located_launch', (4, 0, A, B, C, D, E, F, G, 'up', 'cp_ortho', H, R, None), -1, 'nb_seen_located_launch: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),   # two faults
    ('nb_seen_located_launch', (4, 0, A + 2, B, C, D, E, F, G, 'up', 'cp', H, R, None), -1, 'nb_seen_located_launch: the rows, the lists and seen_col must be 4-byte aligned'),   # two faults
    ('nb_seen_located_launch', (4, 8, A, B, C, D, E, F, G, 'up', 'cp_ortho', R, R, None), -1, 'nb_seen_located_launch: cp16 cannot be inverted: cp16[11] must be -1 (a perspective constant as nb_camera_constant forms it)'),   # two faults
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, None, B, E, F, 8, C, D, None), -1, 'nb_nbody_located_step_launch: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, None, E, F, 8, C, D, None), -1, 'nb_nbody_located_step_launch: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, B, None, F, 8, C, D, None), -1, 'nb_nbody_located_step_launch: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, B, E, None, 8, C, D, None), -1, 'nb_nbody_located_step_launch: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, B, E, F, 8, None, D, None), -1, 'nb_nbody_located_step_launch: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, B, E, F, 8, C, None, None), -1, 'nb_nbody_located_step_launch: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, B, E, F, 8, A, D, None), -1, 'nb_nbody_located_step_launch: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, B, E, F, 8, C, B, None), -1, 'nb_nbody_located_step_launch: buffers must be non-null and the outputs must not alias the inputs'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, B, E, F, 0, C, D, None), -1, 'nb_nbody_located_step_launch: stride must be at least 1'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 0, A, B, E, F, 8, C, D, None), -1, 'nb_nbody_located_step_launch: bodies [first, first + count) must be at least one and lie inside the set'),
    ('nb_nbody_located_step_launch', (None, 1024, 1000, 25, A, B, E, F, 8, C, D, None), -1, 'nb_nbody_located_step_launch: bodies [first, first + count) must be at least one and lie inside the set'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0xffffffff, 2, A, B, E, F, 8, C, D, None), -1, 'nb_nbody_located_step_launch: bodies [first, first + count) must be at least one and lie inside the set'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, B, E + 2, F, 8, C, D, None), -1, 'nb_nbody_located_step_launch: seen_count must be 4-byte aligned'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, B, E, F + 4, 8, C, D, None), -1, 'nb_nbody_located_step_launch: the records and seen_rel must be 16-byte aligned'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A + 8, B, E, F, 8, C, D, None), -1, 'nb_nbody_located_step_launch: the records and seen_rel must be 16-byte aligned'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, B, E, F, 8, C, D + 4, None), -1, 'nb_nbody_located_step_launch: the records and seen_rel must be 16-byte aligned'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, B, C + 16, F, 8, C, D, None), -1, 'nb_nbody_located_step_launch: the outputs must not alias the lists'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, B, E, D + 1024, 8, C, D, None), -1, 'nb_nbody_located_step_launch: the outputs must not alias the lists'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 512, 512, A, B, C + 8192, F, 8, C, D, None), -1, 'nb_nbody_located_step_launch: the outputs must not alias the lists'),
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 1024, A, B, E + 2, F, 0, C, D, None), -1, 'nb_nbody_located_step_launch: stride must be at least 1'),   # two faults
    ('nb_nbody_located_step_launch', ('strict', 1024, 0, 0, A, B, E + 2, F, 8, C, D, None), -1, 'nb_nbody_located_step_launch: bodies [first, first + count) must be at least one and lie inside the set'),   # two faults
]


def test_no_row_expects_the_device():
    assert all(status != _lib.NB_ERR_NO_DEVICE and status != _lib.NB_ERR_HIP for _, _, status, _ in ROWS)
    assert {entry for entry, _, _, _ in ROWS} == {"nb_seen_located_launch", "nb_nbody_located_step_launch"}


@pytest.mark.parametrize("entry", sorted({entry for entry, _, _, _ in ROWS}))
def test_refusals_are_the_recorded_ones(nb, entry):
    lib = _lib.load()
    for name, args, status, message in ROWS:
        if name != entry:
            continue
        held = [PARAMS[a]() if isinstance(a, str) else a for a in args]   # (keeps the blocks alive over the call)
        call = [ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in held]
        assert lib.nb_init_state(0, 0, None, None) == _lib.NB_ERR_INVALID   # a message of another entry's: "none written" shows
        before = _lib.last_error()
        assert getattr(lib, name)(*call) == status, (name, args)
        assert _lib.last_error() == (before if message is None else message), (name, args)
