"""What the entries of the scene batches' seen boids step answer to arguments they must refuse: the status
and the full nb_last_error() text, as a table in the manner of test_scenes_api_messages.py.

Each row is an entry, arguments that fail validation before anything touches the device (the device addresses are fake and never
dereferenced), the status and the message.  A message of None means the call writes none (count = 0 on good arguments succeeds
without work).  Rows marked "two faults" have two arguments wrong at once and pin which check comes first.  No row may reach the
device: on a machine with a GPU the fake addresses would be used.  (The context's own refusals -- the eye set-up, the scene range,
NB_ERR_STATE before an upload -- need a context, hence a device: tests/test_gpu_scenes_seen.py.)
"""
import ctypes

import pytest

from nenbody_amd import _lib
from nenbody_amd._lib import SCENES_SEEN_PROTOTYPES   # (the parent commit has no such table: the file fails here)

CAMS, INST, PI, VI, PO, VO = 0x10000000, 0x20000000, 0x30000000, 0x34000000, 0x38000000, 0x3C000000   # 16-byte aligned, 64 MiB apart at least
CNT, IDS = 0x40000000, 0x44000000
FULL = (1 << 27) // 2048


def _boids(**kw):
    def make():
        p = _lib.default_boids_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    return make


PARAMS = {"boids": _boids(), "boids_tile100": _boids(tile=100)}

St, Se, Sb, Ey = "nb_scenes_boids_seen_step_launch", "nb_scenes_seen_launch", "nb_scenes_step_boids_seen", "nb_scenes_eyes_seen"
NULLS_ST = "{}: cams_16, inst_16 and the four record buffers must be non-null"
NULLS_SE = "{}: cams_16 and inst_16 must be non-null"
SCENES = "{}: scenes must be at least 1"
BODIES = "{}: n must be 1 .. NB_SCENES_MAX_BODIES (2048)"
PRODUCT = "{}: scenes * n must be at most 2^27"
WIDTH = "{}: width must be 1 .. NB_EYES_MAX_WIDTH (4096)"
TILE = "{}: params.tile must be 0, 256, 512 or 1024"
ALIGN_ST = "{}: cams_16, inst_16 and the four record buffers must be 16-byte aligned"
ALIGN_SE = "{}: cams_16 and inst_16 must be 16-byte aligned"
ALIGN4 = "{}: the outputs must be 4-byte aligned"
OVERLAP = "{}: the outputs must not overlap each other or an input"
RANGE = "{}: eyes [first_eye, first_eye + count) exceed the batch"
NONE = "{}: seen_count and seen_ids are both NULL"
REC = 16 * 300                                               # bytes of the records of 3 scenes of 100 bodies


def step(params="boids", scenes=3, n=100, cams=CAMS, inst=INST, width=1024, pi=PI, vi=VI, po=PO, vo=VO):
    return (params, scenes, n, cams, inst, width, pi, vi, po, vo, None)


def seen(scenes=3, n=100, first=0, count=300, cams=CAMS, inst=INST, width=1024, cnt=CNT, ids=IDS):
    return (scenes, n, first, count, cams, inst, width, cnt, ids, None)


# (entry, arguments, status, message)
ROWS = [
    (St, step(cams=None), -1, NULLS_ST), (St, step(inst=None), -1, NULLS_ST), (St, step(pi=None), -1, NULLS_ST),
    (St, step(vi=None), -1, NULLS_ST), (St, step(po=None), -1, NULLS_ST), (St, step(vo=None), -1, NULLS_ST),
    (St, step(params=None, vo=None), -1, NULLS_ST),
    (St, step(scenes=0), -1, SCENES), (St, step(n=0), -1, BODIES), (St, step(n=2049), -1, BODIES),
    (St, step(scenes=FULL + 1, n=2048), -6, PRODUCT), (St, step(scenes=0xFFFFFFFF, n=2048), -6, PRODUCT),
    (St, step(width=0), -1, WIDTH), (St, step(width=4097), -1, WIDTH), (St, step(width=0xFFFFFFFF), -1, WIDTH),
    (St, step(params="boids_tile100"), -1, TILE),
    (St, step(cams=CAMS + 4), -1, ALIGN_ST), (St, step(inst=INST + 8), -1, ALIGN_ST), (St, step(pi=PI + 4), -1, ALIGN_ST),
    (St, step(vi=VI + 4), -1, ALIGN_ST), (St, step(po=PO + 8), -1, ALIGN_ST), (St, step(vo=VO + 12), -1, ALIGN_ST),
    (St, step(po=PI), -1, OVERLAP), (St, step(vo=VI), -1, OVERLAP),                      # in place: it is an out-of-place step
    (St, step(po=VI), -1, OVERLAP), (St, step(vo=PI + REC - 16), -1, OVERLAP),
    (St, step(po=PI - REC + 16), -1, OVERLAP),
    (St, step(vo=PO), -1, OVERLAP), (St, step(vo=PO + REC - 16), -1, OVERLAP),           # the two outputs
    (St, step(po=CAMS + 4 * REC - 16), -1, OVERLAP), (St, step(vo=INST), -1, OVERLAP),   # an output in the matrices
    (St, step(scenes=0, cams=None), -1, NULLS_ST),                                       # two faults
    (St, step(scenes=0, n=0), -1, SCENES),                                               # two faults
    (St, step(n=2049, width=0), -1, BODIES),                                             # two faults
    (St, step(scenes=FULL + 1, n=2048, width=0), -6, PRODUCT),                           # two faults
    (St, step(width=0, params="boids_tile100"), -1, WIDTH),                              # two faults
    (St, step(params="boids_tile100", pi=PI + 4), -1, TILE),                             # two faults
    (St, step(po=PI + 4), -1, ALIGN_ST),                                                 # two faults
    (Se, seen(cams=None), -1, NULLS_SE), (Se, seen(inst=None), -1, NULLS_SE),
    (Se, seen(scenes=0), -1, SCENES), (Se, seen(n=0), -1, BODIES), (Se, seen(n=2049), -1, BODIES),
    (Se, seen(scenes=FULL + 1, n=2048), -6, PRODUCT),
    (Se, seen(width=0), -1, WIDTH), (Se, seen(width=4097), -1, WIDTH),
    (Se, seen(cams=CAMS + 4), -1, ALIGN_SE), (Se, seen(inst=INST + 8), -1, ALIGN_SE),
    (Se, seen(first=1), -1, RANGE), (Se, seen(first=300, count=1), -1, RANGE), (Se, seen(first=0xFFFFFFFF, count=2), -1, RANGE),
    (Se, seen(cnt=None, ids=None), -1, NONE),
    (Se, seen(cnt=CNT + 2), -1, ALIGN4), (Se, seen(ids=IDS + 1), -1, ALIGN4),
    (Se, seen(ids=CNT), -1, OVERLAP), (Se, seen(ids=CNT + 1196), -1, OVERLAP), (Se, seen(cnt=IDS + 4 * 300 * 1024 - 4), -1, OVERLAP),
    (Se, seen(cnt=CAMS), -1, OVERLAP), (Se, seen(ids=INST + 64 * 300 - 4), -1, OVERLAP),
    (Se, seen(first=299, count=1, ids=INST), -1, OVERLAP),
    (Se, seen(count=0), 0, None), (Se, seen(first=300, count=0), 0, None),               # count = 0: a checked no-op
    (Se, seen(cnt=None, count=0), 0, None), (Se, seen(ids=None, count=0), 0, None),      # one output is enough
    (Se, seen(ids=CNT + 1200, count=0, first=0), 0, None),
    (Se, seen(count=0, width=0), -1, WIDTH),
    (Se, seen(scenes=0, cams=None), -1, NULLS_SE),                                       # two faults
    (Se, seen(n=0, width=0), -1, BODIES),                                                # two faults
    (Se, seen(width=0, cams=CAMS + 4), -1, WIDTH),                                       # two faults
    (Se, seen(cams=CAMS + 4, first=301), -1, ALIGN_SE),                                  # two faults
    (Se, seen(first=301, cnt=None, ids=None), -1, RANGE),                                # two faults
    (Se, seen(cnt=None, ids=None, count=0), -1, NONE),
    (Se, seen(cnt=CNT + 2, ids=CNT + 2), -1, ALIGN4),                                    # two faults
    (Sb, (None, 1, None, CAMS, INST, 1024), -1, "{}: ctx is null"),
    (Sb, (None, 1, "boids_tile100", None, None, 0), -1, "{}: ctx is null"),              # two faults
    (Ey, (None, 0, 1, CAMS, INST, 1024, CNT, IDS), -1, "{}: ctx is null"),
    (Ey, (None, 0, 1, None, None, 0, None, None), -1, "{}: ctx is null"),                # two faults
]
ROWS = [(fn, args, status, None if message is None else message.format(fn)) for fn, args, status, message in ROWS]
ENTRIES = sorted({entry for entry, _, _, _ in ROWS})


def test_no_row_expects_the_device():
    assert all(status != _lib.NB_ERR_NO_DEVICE and status != _lib.NB_ERR_HIP for _, _, status, _ in ROWS)
    assert set(ENTRIES) == {St, Se, Sb, Ey} == set(SCENES_SEEN_PROTOTYPES)
    assert all(message is None or message.startswith(entry + ": ") for entry, _, _, message in ROWS)   # every message names its entry


@pytest.mark.parametrize("entry", ENTRIES)
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
        assert lib.nb_scenes_last_error(None).decode() == _lib.last_error()  # the batch's own reader of the thread's message
