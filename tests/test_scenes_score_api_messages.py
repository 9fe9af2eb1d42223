"""What the entries of the scene batches' score answer to arguments they must refuse: the status and the full
nb_last_error() text, as a table in the manner of test_scenes_policy_api_messages.py.

Each row is an entry, arguments that fail validation before anything touches the device (the device addresses are fake and never
dereferenced; sp is a host structure, which the launch does read), the status and the message.  Rows marked "two faults" have two
arguments wrong at once and pin which check comes first.  No row may put the device to work: on a machine with a GPU the fake
addresses would be used.  Two rows of the launch pass every check and end at NB_ERR_NO_DEVICE, which shows that the table's good
arguments are good; where a device is present they are left out.  (The context's own refusals need a context, hence a device:
tests/test_gpu_scenes_score.py.)
"""
import ctypes
import math

import numpy as np
import pytest

from nenbody_amd import _lib
from nenbody_amd._lib import SCENES_SCORE_PROTOTYPES   # (the parent commit has no such table: the file fails here)

POS, VEL, SCORE = 0x10000000, 0x20000000, 0x30000000       # 16-byte aligned, 256 MiB apart
FULL = (1 << 27) // 2048
INF, NAN = math.inf, math.nan
REC = 16 * 300                                               # bytes of the records of 3 scenes of 100 bodies

HOST = {"up": np.array([0, 0, 1], np.float32), "cp": np.zeros(16, np.float32), "out": np.zeros(64, np.uint8)}

La, Ss, Sc, Sr, Sd, Sp = ("nb_scenes_score_launch", "nb_scenes_set_score", "nb_scenes_score", "nb_scenes_score_reset", "nb_scenes_scores",
                          "nb_scenes_step_policy_scored")
NULLS = "{}: null argument"
SCENES = "{}: scenes must be at least 1"
BODIES = "{}: n must be 1 .. NB_SCENES_MAX_BODIES (2048)"
PRODUCT = "{}: scenes * n must be at most 2^27"
RADIUS = "{}: radius_sq must be at least 0 (+inf: every pair)"
GOAL = "{}: goal must be finite"
ALIGN16 = "{}: pos and vel must be 16-byte aligned"
PV = "{}: pos and vel must not overlap"
ALIGN8 = "{}: score must be 8-byte aligned"
OVERLAP = "{}: score must not overlap pos or vel"
CTX = "{}: ctx is null"


def sp(radius_sq=0.25, goal=(1.0, 2.0, 3.0)):
    return _lib.NbScoreParams(radius_sq, (ctypes.c_float * 3)(*goal))


def launch(prm="default", scenes=3, n=100, pos=POS, vel=VEL, score=SCORE):
    return (sp() if prm == "default" else prm, scenes, n, pos, vel, score, None)


# (entry, arguments, status, message)
ROWS = [
    (La, launch(prm=None), -1, NULLS), (La, launch(pos=None), -1, NULLS), (La, launch(vel=None), -1, NULLS), (La, launch(score=None), -1, NULLS),
    (La, launch(scenes=0), -1, SCENES), (La, launch(n=0), -1, BODIES), (La, launch(n=2049), -1, BODIES),
    (La, launch(scenes=FULL + 1, n=2048), -6, PRODUCT), (La, launch(scenes=0xFFFFFFFF, n=2048), -6, PRODUCT),
    (La, launch(prm=sp(radius_sq=-0.5)), -1, RADIUS), (La, launch(prm=sp(radius_sq=NAN)), -1, RADIUS), (La, launch(prm=sp(radius_sq=-INF)), -1, RADIUS),
    (La, launch(prm=sp(goal=(INF, 0, 0))), -1, GOAL), (La, launch(prm=sp(goal=(0, NAN, 0))), -1, GOAL), (La, launch(prm=sp(goal=(0, 0, -INF))), -1, GOAL),
    (La, launch(pos=POS + 4), -1, ALIGN16), (La, launch(vel=VEL + 8), -1, ALIGN16),
    (La, launch(vel=POS), -1, PV), (La, launch(vel=POS + REC - 16), -1, PV), (La, launch(pos=VEL + REC - 16), -1, PV),
    (La, launch(score=SCORE + 4), -1, ALIGN8), (La, launch(score=SCORE + 1), -1, ALIGN8), (La, launch(score=SCORE + 12), -1, ALIGN8),
    (La, launch(score=POS), -1, OVERLAP), (La, launch(score=POS + REC - 8), -1, OVERLAP), (La, launch(score=VEL), -1, OVERLAP),
    (La, launch(score=VEL + REC - 8), -1, OVERLAP), (La, launch(score=POS - 96 + 8), -1, OVERLAP), (La, launch(score=VEL - 8), -1, OVERLAP),
    (La, launch(prm=None, scenes=0), -1, NULLS),                                         # two faults
    (La, launch(scenes=0, n=0), -1, SCENES),                                             # two faults
    (La, launch(n=2049, prm=sp(radius_sq=-1.0)), -1, BODIES),                            # two faults
    (La, launch(prm=sp(radius_sq=NAN, goal=(NAN, 0, 0))), -1, RADIUS),                   # two faults
    (La, launch(prm=sp(goal=(NAN, 0, 0)), pos=POS + 4), -1, GOAL),                       # two faults
    (La, launch(pos=POS + 4, score=SCORE + 4), -1, ALIGN16),                             # two faults
    (La, launch(vel=POS, score=SCORE + 4), -1, PV),                                      # two faults
    (La, launch(score=POS + 4), -1, ALIGN8),                                             # two faults
    (La, launch(), -2, None), (La, launch(prm=sp(radius_sq=INF, goal=(0, 0, 0)), scenes=1, n=1, score=POS + 16), -2, None),   # good arguments: only the device is missing
    (La, launch(score=POS - 96), -2, None), (La, launch(score=VEL + REC), -2, None),     # the records next to the state
    (Ss, (None, sp()), -1, CTX), (Ss, (None, None), -1, CTX),                            # (the second: two faults)
    (Sc, (None,), -1, CTX),
    (Sr, (None,), -1, CTX),
    (Sd, (None, 0, 1, "out"), -1, CTX), (Sd, (None, 5, 5, None), -1, CTX),               # (the second: two faults)
    (Sp, (None, 1, "up", "cp", 1024), -1, CTX), (Sp, (None, 1, None, None, 0), -1, CTX),  # (the second: two faults)
]
ROWS = [(fn, args, status, None if message is None else message.format(fn)) for fn, args, status, message in ROWS]
ENTRIES = sorted({entry for entry, _, _, _ in ROWS})


def test_no_row_expects_work_of_the_device():
    """a row that passes every check ends at the missing device (NB_ERR_NO_DEVICE) on a machine without one; the test below skips those
    rows where there is a device, since the fake addresses would be used"""
    assert all(status != _lib.NB_ERR_HIP for _, _, status, _ in ROWS)
    assert set(ENTRIES) == {La, Ss, Sc, Sr, Sd, Sp} == set(SCENES_SCORE_PROTOTYPES)
    assert all(message is None or message.startswith(entry + ": ") for entry, _, _, message in ROWS)   # every message names its entry
    assert not any(name.startswith("nb_launch_") for name in SCENES_SCORE_PROTOTYPES)


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_are_the_recorded_ones(nb, entry):
    lib = _lib.load()
    device = lib.nb_device_count() > 0
    for name, args, status, message in ROWS:
        if name != entry or (status == _lib.NB_ERR_NO_DEVICE and device):
            continue
        call = [HOST[a].ctypes.data if isinstance(a, str) else (ctypes.byref(a) if isinstance(a, _lib.NbScoreParams) else a) for a in args]
        assert lib.nb_init_state(0, 0, None, None) == _lib.NB_ERR_INVALID   # a message of another entry's: "none written" shows
        before = _lib.last_error()
        assert getattr(lib, name)(*call) == status, (name, args)
        if status != _lib.NB_ERR_NO_DEVICE:
            assert _lib.last_error() == (before if message is None else message), (name, args)
            assert lib.nb_scenes_last_error(None).decode() == _lib.last_error()  # the batch's own reader of the thread's message
