"""What the entries of the scene batches' neural policy answer to arguments they must refuse: the status and
the full nb_last_error() text, as a table in the manner of test_scenes_located_api_messages.py.

Each row is an entry, arguments that fail validation before anything touches the device (the device addresses are fake and never
dereferenced; up_xyz is a host array, which the step does read), the status and the message.  A message of None means the call writes
none (count = 0 on good arguments succeeds without work).  Rows marked "two faults" have two arguments wrong at once and pin which
check comes first.  No row may put the device to work: on a machine with a GPU the fake addresses would be used.  Two rows of the
step pass every check and end at NB_ERR_NO_DEVICE, which shows that the table's good arguments are good; where a device is present
they are left out.  (The context's own refusals need a context, hence a device: tests/test_gpu_scenes_policy.py.)
"""
import ctypes
import math

import numpy as np
import pytest

from nenbody_amd import _lib
from nenbody_amd._lib import SCENES_POLICY_PROTOTYPES   # (the parent commit has no such table: the file fails here)

CAMS, INST, PI, VI, PO, VO = 0x10000000, 0x20000000, 0x30000000, 0x34000000, 0x38000000, 0x3C000000   # 16-byte aligned, 64 MiB apart at least
WTS, FEAT, ACT = 0x40000000, 0x44000000, 0x48000000
FULL = (1 << 27) // 2048
INF, NAN = math.inf, math.nan

HOST = {"up": np.array([0, 0, 1], np.float32), "cp": np.zeros(16, np.float32), "w": np.zeros(16578 * 3, np.float32)}

St, Ob, Sp, Sc, Ey = ("nb_scenes_policy_step_launch", "nb_scenes_policy_observe_launch", "nb_scenes_set_policy", "nb_scenes_step_policy",
                      "nb_scenes_eyes_policy")
NULLS = "{}: null argument"
SCENES = "{}: scenes must be at least 1"
BODIES = "{}: n must be 1 .. NB_SCENES_MAX_BODIES (2048)"
PRODUCT = "{}: scenes * n must be at most 2^27"
WIDTH = "{}: width must be 1 .. NB_EYES_MAX_WIDTH (4096)"
FEATURES = "{}: features must be 1 .. NB_POLICY_MAX_FEATURES (256)"
HIDDEN = "{}: hidden must be 1 .. NB_POLICY_MAX_HIDDEN (64)"
MULTIPLE = "{}: width must be a multiple of features"
POLICIES = "{}: policies must be 1 or scenes"
LIMIT = "{}: accel_limit must be at least 0 (+inf: no limit)"
MODE = "{}: params.mode must be NB_MODE_STRICT or NB_MODE_FAST"
FAST = "{}: a scene batch steps STRICT only (params.mode is NB_MODE_FAST)"
TILE = "{}: params.tile must be 0, 256, 512 or 1024"
ALIGN_W = "{}: weights must be 4-byte aligned"
ALIGN_ST = "{}: cams_16, inst_16 and the four record buffers must be 16-byte aligned"
ALIGN_OB = "{}: cams_16 and inst_16 must be 16-byte aligned"
ALIGN4 = "{}: the outputs must be 4-byte aligned"
OVERLAP = "{}: the outputs must not overlap each other or an input"
RANGE = "{}: eyes [first_eye, first_eye + count) exceed the batch"
NONE = "{}: feat_out and act_out are both NULL"
REC = 16 * 300                                               # bytes of the records of 3 scenes of 100 bodies
POLICY = 4 * (64 * 32 + 32 + 64 + 2)                         # bytes of one policy of shape (64, 32)


def params(**fields):
    p = _lib.NbParams(0.1, 0.001, 1e-7, 0, 0)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def step(prm=None, scenes=3, n=100, cams=CAMS, inst=INST, width=1024, up="up", f=64, h=32, pol=3, w=WTS, lim=0.5, pi=PI, vi=VI, po=PO,
         vo=VO):
    return (prm, scenes, n, cams, inst, width, up, f, h, pol, w, lim, pi, vi, po, vo, None)


def obs(scenes=3, n=100, first=0, count=300, cams=CAMS, inst=INST, width=1024, f=64, h=32, pol=3, w=WTS, lim=0.5, feat=FEAT, act=ACT):
    return (scenes, n, first, count, cams, inst, width, f, h, pol, w, lim, feat, act, None)


# (entry, arguments, status, message)
ROWS = [
    (St, step(cams=None), -1, NULLS), (St, step(inst=None), -1, NULLS), (St, step(up=None), -1, NULLS), (St, step(w=None), -1, NULLS),
    (St, step(pi=None), -1, NULLS), (St, step(vi=None), -1, NULLS), (St, step(po=None), -1, NULLS), (St, step(vo=None), -1, NULLS),
    (St, step(scenes=0), -1, SCENES), (St, step(n=0), -1, BODIES), (St, step(n=2049), -1, BODIES),
    (St, step(scenes=FULL + 1, n=2048, pol=1), -6, PRODUCT), (St, step(scenes=0xFFFFFFFF, n=2048), -6, PRODUCT),
    (St, step(width=0), -1, WIDTH), (St, step(width=4097), -1, WIDTH), (St, step(width=0xFFFFFFFF), -1, WIDTH),
    (St, step(f=0), -1, FEATURES), (St, step(f=257), -1, FEATURES), (St, step(f=512), -1, FEATURES),   # (512 divides 1024: the bound comes first)
    (St, step(h=0), -1, HIDDEN), (St, step(h=65), -1, HIDDEN),
    (St, step(f=3), -1, MULTIPLE), (St, step(width=1000, f=64), -1, MULTIPLE), (St, step(width=63, f=64), -1, MULTIPLE),
    (St, step(pol=0), -1, POLICIES), (St, step(pol=2), -1, POLICIES), (St, step(pol=4), -1, POLICIES),
    (St, step(lim=-0.5), -1, LIMIT), (St, step(lim=NAN), -1, LIMIT), (St, step(lim=-INF), -1, LIMIT),
    (St, step(prm=params(mode=7)), -1, MODE), (St, step(prm=params(mode=1)), -6, FAST), (St, step(prm=params(tile=100)), -1, TILE),
    (St, step(w=WTS + 2), -1, ALIGN_W), (St, step(w=WTS + 1), -1, ALIGN_W),
    (St, step(cams=CAMS + 4), -1, ALIGN_ST), (St, step(inst=INST + 8), -1, ALIGN_ST), (St, step(pi=PI + 4), -1, ALIGN_ST),
    (St, step(vi=VI + 4), -1, ALIGN_ST), (St, step(po=PO + 8), -1, ALIGN_ST), (St, step(vo=VO + 12), -1, ALIGN_ST),
    (St, step(po=PI), -1, OVERLAP), (St, step(vo=VI), -1, OVERLAP),                      # in place: it is an out-of-place step
    (St, step(po=VI), -1, OVERLAP), (St, step(vo=PI + REC - 16), -1, OVERLAP), (St, step(po=PI - REC + 16), -1, OVERLAP),
    (St, step(vo=PO), -1, OVERLAP), (St, step(vo=PO + REC - 16), -1, OVERLAP),           # the two outputs
    (St, step(po=CAMS + 4 * REC - 16), -1, OVERLAP), (St, step(vo=INST), -1, OVERLAP),   # an output in the matrices
    (St, step(po=WTS), -1, OVERLAP), (St, step(vo=WTS + 3 * POLICY // 16 * 16 - 16), -1, OVERLAP),   # an output in the policies
    (St, step(po=WTS + POLICY // 16 * 16, pol=1, w=WTS + 16), -1, OVERLAP),              # one policy is read whatever the batch
    (St, step(scenes=0, cams=None), -1, NULLS),                                          # two faults
    (St, step(scenes=0, n=0), -1, SCENES),                                               # two faults
    (St, step(n=2049, width=0), -1, BODIES),                                             # two faults
    (St, step(width=0, f=0), -1, WIDTH),                                                 # two faults
    (St, step(f=0, h=0), -1, FEATURES),                                                  # two faults
    (St, step(h=65, f=3), -1, HIDDEN),                                                   # two faults
    (St, step(f=3, pol=2), -1, MULTIPLE),                                                # two faults
    (St, step(pol=2, lim=-1.0), -1, POLICIES),                                           # two faults
    (St, step(lim=-1.0, prm=params(mode=7)), -1, LIMIT),                                 # two faults
    (St, step(prm=params(mode=1), w=WTS + 2), -6, FAST),                                 # two faults
    (St, step(w=WTS + 2, pi=PI + 4), -1, ALIGN_W),                                       # two faults
    (St, step(po=PI + 4), -1, ALIGN_ST),                                                 # two faults
    (St, step(lim=INF), -2, None), (St, step(lim=0.0, pol=1, f=1, h=1, width=1), -2, None),   # good arguments: only the device is missing
    (Ob, obs(cams=None), -1, NULLS), (Ob, obs(inst=None), -1, NULLS), (Ob, obs(w=None), -1, NULLS),
    (Ob, obs(scenes=0), -1, SCENES), (Ob, obs(n=0), -1, BODIES), (Ob, obs(n=2049), -1, BODIES),
    (Ob, obs(scenes=FULL + 1, n=2048, pol=1), -6, PRODUCT),
    (Ob, obs(width=0), -1, WIDTH), (Ob, obs(width=4097), -1, WIDTH),
    (Ob, obs(f=0), -1, FEATURES), (Ob, obs(f=257), -1, FEATURES), (Ob, obs(h=0), -1, HIDDEN), (Ob, obs(h=65), -1, HIDDEN),
    (Ob, obs(f=3), -1, MULTIPLE), (Ob, obs(pol=2), -1, POLICIES), (Ob, obs(pol=0), -1, POLICIES),
    (Ob, obs(lim=-0.5), -1, LIMIT), (Ob, obs(lim=NAN), -1, LIMIT),
    (Ob, obs(w=WTS + 2), -1, ALIGN_W),
    (Ob, obs(cams=CAMS + 4), -1, ALIGN_OB), (Ob, obs(inst=INST + 8), -1, ALIGN_OB),
    (Ob, obs(first=1), -1, RANGE), (Ob, obs(first=300, count=1), -1, RANGE), (Ob, obs(first=0xFFFFFFFF, count=2), -1, RANGE),
    (Ob, obs(feat=None, act=None), -1, NONE),
    (Ob, obs(feat=FEAT + 2), -1, ALIGN4), (Ob, obs(act=ACT + 1), -1, ALIGN4),
    (Ob, obs(act=FEAT), -1, OVERLAP), (Ob, obs(act=FEAT + 4 * 64 * 300 - 4), -1, OVERLAP), (Ob, obs(feat=ACT + 8 * 300 - 4), -1, OVERLAP),
    (Ob, obs(feat=CAMS), -1, OVERLAP), (Ob, obs(act=INST + 64 * 300 - 4), -1, OVERLAP),  # an output in an input
    (Ob, obs(feat=WTS), -1, OVERLAP), (Ob, obs(act=WTS + 3 * POLICY - 4), -1, OVERLAP),
    (Ob, obs(first=299, count=1, act=INST), -1, OVERLAP),
    (Ob, obs(count=0), 0, None), (Ob, obs(first=300, count=0), 0, None),                 # count = 0: a checked no-op
    (Ob, obs(count=0, feat=None), 0, None), (Ob, obs(count=0, act=None), 0, None),       # one output is enough
    (Ob, obs(act=FEAT + 4 * 64 * 300, count=0), 0, None),
    (Ob, obs(count=0, width=0), -1, WIDTH), (Ob, obs(count=0, f=3), -1, MULTIPLE), (Ob, obs(count=0, lim=-1.0), -1, LIMIT),
    (Ob, obs(count=0, feat=None, act=None), -1, NONE),
    (Ob, obs(scenes=0, cams=None), -1, NULLS),                                           # two faults
    (Ob, obs(n=0, width=0), -1, BODIES),                                                 # two faults
    (Ob, obs(width=0, f=257), -1, WIDTH),                                                # two faults
    (Ob, obs(lim=-1.0, w=WTS + 2), -1, LIMIT),                                           # two faults
    (Ob, obs(w=WTS + 2, cams=CAMS + 4), -1, ALIGN_W),                                    # two faults
    (Ob, obs(cams=CAMS + 4, first=301), -1, ALIGN_OB),                                   # two faults
    (Ob, obs(first=301, feat=None, act=None), -1, RANGE),                                # two faults
    (Ob, obs(feat=FEAT + 2, act=FEAT + 2), -1, ALIGN4),                                  # two faults
    (Sp, (None, 64, 32, 1, "w", 0.5), -1, "{}: ctx is null"),
    (Sp, (None, 0, 0, 0, None, -1.0), -1, "{}: ctx is null"),                            # two faults
    (Sc, (None, 1, "up", "cp", 1024), -1, "{}: ctx is null"),
    (Sc, (None, 1, None, None, 0), -1, "{}: ctx is null"),                               # two faults
    (Ey, (None, 0, 1, "up", "cp", 1024, FEAT, ACT), -1, "{}: ctx is null"),
    (Ey, (None, 0, 1, None, None, 0, None, None), -1, "{}: ctx is null"),                # two faults
]
ROWS = [(fn, args, status, None if message is None else message.format(fn)) for fn, args, status, message in ROWS]
ENTRIES = sorted({entry for entry, _, _, _ in ROWS})


def test_no_row_expects_work_of_the_device():
    """a row that passes every check ends at the missing device (NB_ERR_NO_DEVICE) on a machine without one; the test below skips those
    rows where there is a device, since the fake addresses would be used"""
    assert all(status != _lib.NB_ERR_HIP for _, _, status, _ in ROWS)
    assert set(ENTRIES) == {St, Ob, Sp, Sc, Ey} == set(SCENES_POLICY_PROTOTYPES) - {"nb_policy_floats"}
    assert all(message is None or message.startswith(entry + ": ") for entry, _, _, message in ROWS)   # every message names its entry
    assert not any(name.startswith("nb_launch_") for name in SCENES_POLICY_PROTOTYPES)


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_are_the_recorded_ones(nb, entry):
    lib = _lib.load()
    device = lib.nb_device_count() > 0
    for name, args, status, message in ROWS:
        if name != entry or (status == _lib.NB_ERR_NO_DEVICE and device):
            continue
        call = [HOST[a].ctypes.data if isinstance(a, str) else (ctypes.byref(a) if isinstance(a, _lib.NbParams) else a) for a in args]
        assert lib.nb_init_state(0, 0, None, None) == _lib.NB_ERR_INVALID   # a message of another entry's: "none written" shows
        before = _lib.last_error()
        assert getattr(lib, name)(*call) == status, (name, args)
        if status != _lib.NB_ERR_NO_DEVICE:
            assert _lib.last_error() == (before if message is None else message), (name, args)
            assert lib.nb_scenes_last_error(None).decode() == _lib.last_error()  # the batch's own reader of the thread's message
