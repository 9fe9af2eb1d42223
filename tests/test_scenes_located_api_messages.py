"""What the entries of the scene batches' gravity from located vision answer to arguments they must refuse:
the status and the full nb_last_error() text, as a table in the manner of test_scenes_seen_api_messages.py.

Each row is an entry, arguments that fail validation before anything touches the device (the device addresses are fake and never
dereferenced; up_xyz and cp16 are host arrays, which the checks do read), the status and the message.  A message of None means the
call writes none (count = 0 on good arguments succeeds without work).  Rows marked "two faults" have two arguments wrong at once and
pin which check comes first.  No row may reach the device: on a machine with a GPU the fake addresses would be used.  (The context's
own refusals need a context, hence a device: tests/test_gpu_scenes_located.py.)
"""
import ctypes

import numpy as np
import pytest

from nenbody_amd import _lib
from nenbody_amd._lib import SCENES_LOCATED_PROTOTYPES   # (the parent commit has no such table: the file fails here)

CAMS, INST, PI, VI, PO, VO = 0x10000000, 0x20000000, 0x30000000, 0x34000000, 0x38000000, 0x3C000000   # 16-byte aligned, 64 MiB apart at least
CNT, IDS, DEP, COL, REL = 0x40000000, 0x44000000, 0x48000000, 0x4C000000, 0x50000000
FULL = (1 << 27) // 2048


def _cp(**entries):
    """a constant of the shape nb_camera_constant forms, with the given entries replaced"""
    cp = np.zeros(16, np.float32)
    cp[0], cp[5], cp[10], cp[11], cp[14] = 1.5, 1.5, -1.0001, -1.0, -1.0001
    for k, v in entries.items():
        cp[int(k[1:])] = v
    return cp


HOST = {"up": np.array([0, 0, 1], np.float32), "cp": _cp(), "cp_11": _cp(e11=1.0), "cp_11_nan": _cp(e11=np.nan), "cp_4": _cp(e4=0.5),
        "cp_15": _cp(e15=1.0), "cp_0": _cp(e0=0.0), "cp_14": _cp(e14=0.0), "cp_11_4_0": _cp(e11=0.0, e4=1.0, e0=0.0),
        "cp_4_0": _cp(e4=1.0, e0=0.0), "cp_0_14": _cp(e0=0.0, e14=0.0)}

St, Lo, Sc, Ey = ("nb_scenes_nbody_located_step_launch", "nb_scenes_located_launch", "nb_scenes_step_nbody_located",
                  "nb_scenes_eyes_located")
NULLS = "{}: null argument"
SCENES = "{}: scenes must be at least 1"
BODIES = "{}: n must be 1 .. NB_SCENES_MAX_BODIES (2048)"
PRODUCT = "{}: scenes * n must be at most 2^27"
WIDTH = "{}: width must be 1 .. NB_EYES_MAX_WIDTH (4096)"
SHAPE = " (a perspective constant as nb_camera_constant forms it)"
CP11 = "{}: cp16 cannot be inverted: cp16[11] must be -1" + SHAPE
CPZ = "{{}}: cp16 cannot be inverted: cp16[{}] must be 0" + SHAPE
CPN = "{{}}: cp16 cannot be inverted: cp16[{}] must not be 0" + SHAPE
ALIGN_ST = "{}: cams_16, inst_16 and the four record buffers must be 16-byte aligned"
ALIGN_LO = "{}: cams_16, inst_16, vel_in and seen_rel must be 16-byte aligned"
ALIGN4 = "{}: the outputs must be 4-byte aligned"
OVERLAP = "{}: the outputs must not overlap each other or an input"
RANGE = "{}: eyes [first_eye, first_eye + count) exceed the batch"
NONE = "{}: seen_count, seen_ids, seen_depth, seen_col and seen_rel are all NULL"
REC = 16 * 300                                               # bytes of the records of 3 scenes of 100 bodies
CELLS = 300 * 1024                                           # slots of their lists at width 1024


def step(params=None, scenes=3, n=100, cams=CAMS, inst=INST, up="up", cp="cp", width=1024, pi=PI, vi=VI, po=PO, vo=VO):
    return (params, scenes, n, cams, inst, up, cp, width, pi, vi, po, vo, None)


def loc(scenes=3, n=100, first=0, count=300, cams=CAMS, inst=INST, vi=VI, up="up", cp="cp", width=1024, cnt=CNT, ids=IDS, dep=DEP, col=COL,
        rel=REL):
    return (scenes, n, first, count, cams, inst, vi, up, cp, width, cnt, ids, dep, col, rel, None)


ONLY_REL = dict(cnt=None, ids=None, dep=None, col=None)

# (entry, arguments, status, message)
ROWS = [
    (St, step(cams=None), -1, NULLS), (St, step(inst=None), -1, NULLS), (St, step(up=None), -1, NULLS), (St, step(cp=None), -1, NULLS),
    (St, step(pi=None), -1, NULLS), (St, step(vi=None), -1, NULLS), (St, step(po=None), -1, NULLS), (St, step(vo=None), -1, NULLS),
    (St, step(scenes=0), -1, SCENES), (St, step(n=0), -1, BODIES), (St, step(n=2049), -1, BODIES),
    (St, step(scenes=FULL + 1, n=2048), -6, PRODUCT), (St, step(scenes=0xFFFFFFFF, n=2048), -6, PRODUCT),
    (St, step(width=0), -1, WIDTH), (St, step(width=4097), -1, WIDTH), (St, step(width=0xFFFFFFFF), -1, WIDTH),
    (St, step(cp="cp_11"), -1, CP11), (St, step(cp="cp_11_nan"), -1, CP11),                                  # L6's three shapes
    (St, step(cp="cp_4"), -1, CPZ.format(4)), (St, step(cp="cp_15"), -1, CPZ.format(15)),
    (St, step(cp="cp_0"), -1, CPN.format(0)), (St, step(cp="cp_14"), -1, CPN.format(14)),
    (St, step(cp="cp_11_4_0"), -1, CP11), (St, step(cp="cp_4_0"), -1, CPZ.format(4)), (St, step(cp="cp_0_14"), -1, CPN.format(0)),
    (St, step(cams=CAMS + 4), -1, ALIGN_ST), (St, step(inst=INST + 8), -1, ALIGN_ST), (St, step(pi=PI + 4), -1, ALIGN_ST),
    (St, step(vi=VI + 4), -1, ALIGN_ST), (St, step(po=PO + 8), -1, ALIGN_ST), (St, step(vo=VO + 12), -1, ALIGN_ST),
    (St, step(po=PI), -1, OVERLAP), (St, step(vo=VI), -1, OVERLAP),                      # in place: it is an out-of-place step
    (St, step(po=VI), -1, OVERLAP), (St, step(vo=PI + REC - 16), -1, OVERLAP),
    (St, step(po=PI - REC + 16), -1, OVERLAP),
    (St, step(vo=PO), -1, OVERLAP), (St, step(vo=PO + REC - 16), -1, OVERLAP),           # the two outputs
    (St, step(po=CAMS + 4 * REC - 16), -1, OVERLAP), (St, step(vo=INST), -1, OVERLAP),   # an output in the matrices
    (St, step(scenes=0, cams=None), -1, NULLS),                                          # two faults
    (St, step(scenes=0, n=0), -1, SCENES),                                               # two faults
    (St, step(n=2049, width=0), -1, BODIES),                                             # two faults
    (St, step(scenes=FULL + 1, n=2048, width=0), -6, PRODUCT),                           # two faults
    (St, step(width=0, cp="cp_11"), -1, WIDTH),                                          # two faults
    (St, step(cp="cp_11", pi=PI + 4), -1, CP11),                                         # two faults
    (St, step(po=PI + 4), -1, ALIGN_ST),                                                 # two faults
    (Lo, loc(cams=None), -1, NULLS), (Lo, loc(inst=None), -1, NULLS), (Lo, loc(vi=None), -1, NULLS), (Lo, loc(up=None), -1, NULLS),
    (Lo, loc(cp=None), -1, NULLS),
    (Lo, loc(scenes=0), -1, SCENES), (Lo, loc(n=0), -1, BODIES), (Lo, loc(n=2049), -1, BODIES),
    (Lo, loc(scenes=FULL + 1, n=2048), -6, PRODUCT),
    (Lo, loc(width=0), -1, WIDTH), (Lo, loc(width=4097), -1, WIDTH),
    (Lo, loc(cp="cp_11"), -1, CP11), (Lo, loc(cp="cp_4"), -1, CPZ.format(4)), (Lo, loc(cp="cp_0"), -1, CPN.format(0)),
    (Lo, loc(cp="cp_14"), -1, CPN.format(14)),
    (Lo, loc(cams=CAMS + 4), -1, ALIGN_LO), (Lo, loc(inst=INST + 8), -1, ALIGN_LO), (Lo, loc(vi=VI + 4), -1, ALIGN_LO),
    (Lo, loc(rel=REL + 4), -1, ALIGN_LO), (Lo, loc(rel=REL + 8), -1, ALIGN_LO),
    (Lo, loc(first=1), -1, RANGE), (Lo, loc(first=300, count=1), -1, RANGE), (Lo, loc(first=0xFFFFFFFF, count=2), -1, RANGE),
    (Lo, loc(rel=None, **ONLY_REL), -1, NONE),
    (Lo, loc(cnt=CNT + 2), -1, ALIGN4), (Lo, loc(ids=IDS + 1), -1, ALIGN4), (Lo, loc(dep=DEP + 2), -1, ALIGN4),
    (Lo, loc(col=COL + 3), -1, ALIGN4),
    (Lo, loc(ids=CNT), -1, OVERLAP), (Lo, loc(ids=CNT + 1196), -1, OVERLAP), (Lo, loc(cnt=IDS + 4 * CELLS - 4), -1, OVERLAP),   # each pair
    (Lo, loc(dep=IDS), -1, OVERLAP), (Lo, loc(col=DEP + 4 * CELLS - 4), -1, OVERLAP), (Lo, loc(col=IDS), -1, OVERLAP),
    (Lo, loc(rel=COL), -1, OVERLAP), (Lo, loc(col=REL + 16 * CELLS - 16), -1, OVERLAP), (Lo, loc(dep=REL + 16), -1, OVERLAP),
    (Lo, loc(rel=CNT), -1, OVERLAP), (Lo, loc(dep=CNT), -1, OVERLAP), (Lo, loc(col=CNT + 4), -1, OVERLAP), (Lo, loc(rel=IDS + 16), -1, OVERLAP),
    (Lo, loc(cnt=CAMS), -1, OVERLAP), (Lo, loc(ids=INST + 64 * 300 - 4), -1, OVERLAP),   # an output in an input
    (Lo, loc(rel=VI), -1, OVERLAP), (Lo, loc(dep=VI + REC - 4), -1, OVERLAP),
    (Lo, loc(first=299, count=1, ids=INST), -1, OVERLAP),
    (Lo, loc(count=0), 0, None), (Lo, loc(first=300, count=0), 0, None),                 # count = 0: a checked no-op
    (Lo, loc(count=0, rel=REL, **ONLY_REL), 0, None), (Lo, loc(cnt=None, count=0), 0, None),   # one output is enough
    (Lo, loc(ids=CNT + 1200, count=0, first=0), 0, None),
    (Lo, loc(count=0, width=0), -1, WIDTH), (Lo, loc(count=0, cp="cp_11"), -1, CP11),
    (Lo, loc(scenes=0, cams=None), -1, NULLS),                                           # two faults
    (Lo, loc(n=0, width=0), -1, BODIES),                                                 # two faults
    (Lo, loc(width=0, cp="cp_4"), -1, WIDTH),                                            # two faults
    (Lo, loc(cp="cp_4", cams=CAMS + 4), -1, CPZ.format(4)),                              # two faults
    (Lo, loc(cams=CAMS + 4, first=301), -1, ALIGN_LO),                                   # two faults
    (Lo, loc(first=301, rel=None, **ONLY_REL), -1, RANGE),                               # two faults
    (Lo, loc(rel=None, count=0, **ONLY_REL), -1, NONE),
    (Lo, loc(cnt=CNT + 2, ids=CNT + 2), -1, ALIGN4),                                     # two faults
    (Sc, (None, 1, "up", "cp", 1024), -1, "{}: ctx is null"),
    (Sc, (None, 1, None, "cp_11", 0), -1, "{}: ctx is null"),                            # two faults
    (Ey, (None, 0, 1, "up", "cp", 1024, CNT, IDS, DEP, COL, REL), -1, "{}: ctx is null"),
    (Ey, (None, 0, 1, None, None, 0, None, None, None, None, None), -1, "{}: ctx is null"),   # two faults
]
ROWS = [(fn, args, status, None if message is None else message.format(fn)) for fn, args, status, message in ROWS]
ENTRIES = sorted({entry for entry, _, _, _ in ROWS})


def test_no_row_expects_the_device():
    assert all(status != _lib.NB_ERR_NO_DEVICE and status != _lib.NB_ERR_HIP for _, _, status, _ in ROWS)
    assert set(ENTRIES) == {St, Lo, Sc, Ey} == set(SCENES_LOCATED_PROTOTYPES)
    assert all(message is None or message.startswith(entry + ": ") for entry, _, _, message in ROWS)   # every message names its entry
    assert not any(name.startswith("nb_launch_") for name in SCENES_LOCATED_PROTOTYPES)


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_are_the_recorded_ones(nb, entry):
    lib = _lib.load()
    for name, args, status, message in ROWS:
        if name != entry:
            continue
        call = [HOST[a].ctypes.data if isinstance(a, str) else a for a in args]
        assert lib.nb_init_state(0, 0, None, None) == _lib.NB_ERR_INVALID   # a message of another entry's: "none written" shows
        before = _lib.last_error()
        assert getattr(lib, name)(*call) == status, (name, args)
        assert _lib.last_error() == (before if message is None else message), (name, args)
        assert lib.nb_scenes_last_error(None).decode() == _lib.last_error()  # the batch's own reader of the thread's message
