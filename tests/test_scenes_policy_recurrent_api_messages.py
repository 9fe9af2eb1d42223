"""What the entries of the scene batches' recurrent policy answer to arguments they must refuse: the status
and the full nb_last_error() text, as a table in the manner of test_scenes_policy_api_messages.py.

Each row is an entry, arguments that fail validation before anything touches the device (the device addresses are fake and never
dereferenced; up_xyz is a host array, which the step does read), the status and the message.  A message of None means the call writes
none (count = 0 on good arguments succeeds without work).  Rows marked "two faults" have two arguments wrong at once and pin which
check comes first.  No row may put the device to work: on a machine with a GPU the fake addresses would be used.  Rows that pass
every check end at NB_ERR_NO_DEVICE, which shows that the table's good arguments are good; where a device is present they are left
out.  (The context's own refusals need a context, hence a device: tests/test_gpu_scenes_policy_recurrent.py.)
"""
import ctypes
import math

import numpy as np
import pytest

from nenbody_amd import _lib
from nenbody_amd._lib import SCENES_POLICY_RECURRENT_PROTOTYPES   # (the parent commit has no such table: the file fails here)

CAMS, INST, PI, VI, PO, VO = 0x10000000, 0x20000000, 0x30000000, 0x34000000, 0x38000000, 0x3C000000   # 16-byte aligned, 64 MiB apart at least
WTS, FEAT, ACT, MI, MO = 0x40000000, 0x44000000, 0x48000000, 0x4C000000, 0x50000000
MEAN, THETA, SCORE, RANK, FIT, REP, OUT = 0x60000000, 0x70000000, 0x80000000, 0x90000000, 0xA0000000, 0xB0000000, 0xC0000000
FULL = (1 << 27) // 2048
INF, NAN = math.inf, math.nan

HOST = {"up": np.array([0, 0, 1], np.float32), "cp": np.zeros(16, np.float32), "w": np.zeros(20674 * 3, np.float32),
        "out": np.zeros(64, np.float32)}

St, Ob, Pf, Uf = ("nb_scenes_policy_recurrent_step_launch", "nb_scenes_policy_recurrent_observe_launch", "nb_scenes_es_perturb_floats_launch",
                  "nb_scenes_es_update_floats_launch")
Sp, Ey, Mr, Mg, Ms, Es = ("nb_scenes_set_policy_recurrent", "nb_scenes_eyes_policy_memory", "nb_scenes_memory_reset", "nb_scenes_memory",
                          "nb_scenes_set_memory", "nb_scenes_es_set_recurrent")
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
MEMLIMIT = "{}: memory_limit must be at least 0 (+inf: no limit)"
MODE = "{}: params.mode must be NB_MODE_STRICT or NB_MODE_FAST"
FAST = "{}: a scene batch steps STRICT only (params.mode is NB_MODE_FAST)"
ALIGN_W = "{}: weights must be 4-byte aligned"
ALIGN_MEM = "{}: mem_in and mem_out must be 4-byte aligned"
ALIGN_M1 = "{}: mem must be 4-byte aligned"
ALIGN_ST = "{}: cams_16, inst_16 and the four record buffers must be 16-byte aligned"
ALIGN_OB = "{}: cams_16 and inst_16 must be 16-byte aligned"
ALIGN4 = "{}: the outputs must be 4-byte aligned"
OVERLAP = "{}: the outputs must not overlap each other or an input"
PARTIAL = "{}: mem_out must be mem_in itself or clear of it"
RANGE = "{}: eyes [first_eye, first_eye + count) exceed the batch"
NONE = "{}: feat_out, act_out and mem_out are all NULL"
FLOATS = "{}: floats must be 1 .. NB_ES_MAX_FLOATS (20674)"
SIGMA = "{}: sigma must be at least 0 and finite"
STEP = "{}: step must be finite"
COEF = "{}: coef must be finite"
ES_RANGE = "{}: scenes [first_scene, first_scene + count) must lie in 0 .. NB_ES_MAX_POPULATION (4096)"
POPULATION = "{}: scenes must be 1 .. NB_ES_MAX_POPULATION (4096)"
ALIGN_P = "{}: mean and theta_out must be 4-byte aligned"
OVERLAP_P = "{}: theta_out must not overlap mean"
ALIGN8 = "{}: score must be 8-byte aligned"
ALIGN_MEAN = "{}: mean must be 4-byte aligned"
CTX = "{}: ctx is null"
REC = 16 * 300                                               # bytes of the records of 3 scenes of 100 bodies
POLICY = 4 * (64 * 32 + 32 * 32 + 32 + 64 + 2)               # bytes of one recurrent policy of shape (64, 32)
MEM = 4 * 300 * 32                                           # bytes of the memory of 3 scenes of 100 bodies, H = 32
M = 128                                                      # policy_recurrent_floats(8, 7)
MB = 4 * M


def params(**fields):
    p = _lib.NbParams(0.1, 0.001, 1e-7, 0, 0)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def ep(sigma=0.5, step=0.01, coef=(0, 0, 0, 0, -1, 0), seed=1234):
    return _lib.NbEsParams(sigma, step, (ctypes.c_float * 6)(*coef), seed)


def step(prm=None, scenes=3, n=100, cams=CAMS, inst=INST, width=1024, up="up", f=64, h=32, pol=3, w=WTS, lim=0.5, s=1.0, pi=PI, vi=VI,
         mi=MI, po=PO, vo=VO, mo=MO):
    return (prm, scenes, n, cams, inst, width, up, f, h, pol, w, lim, s, pi, vi, mi, po, vo, mo, None)


def obs(scenes=3, n=100, first=0, count=300, cams=CAMS, inst=INST, width=1024, f=64, h=32, pol=3, w=WTS, lim=0.5, s=1.0, mem=MI, feat=FEAT,
        act=ACT, mo=MO):
    return (scenes, n, first, count, cams, inst, width, f, h, pol, w, lim, s, mem, feat, act, mo, None)


def perturb(prm="default", floats=M, g=0, first=0, count=3, mean=MEAN, theta=THETA):
    return (ep() if prm == "default" else prm, floats, g, first, count, mean, theta, None)


def update(prm="default", floats=M, g=0, scenes=3, score=SCORE, mean=MEAN, mean_out=OUT, rank=RANK, fit=FIT, rep=REP):
    return (ep() if prm == "default" else prm, floats, g, scenes, score, mean, mean_out, rank, fit, rep, None)


# (entry, arguments, status, message)
ROWS = [
    (St, step(cams=None), -1, NULLS), (St, step(inst=None), -1, NULLS), (St, step(up=None), -1, NULLS), (St, step(w=None), -1, NULLS),
    (St, step(pi=None), -1, NULLS), (St, step(vi=None), -1, NULLS), (St, step(po=None), -1, NULLS), (St, step(vo=None), -1, NULLS),
    (St, step(mi=None), -1, NULLS), (St, step(mo=None), -1, NULLS),
    (St, step(scenes=0), -1, SCENES), (St, step(n=0), -1, BODIES), (St, step(n=2049), -1, BODIES),
    (St, step(scenes=FULL + 1, n=2048, pol=1), -6, PRODUCT),
    (St, step(width=0), -1, WIDTH), (St, step(width=4097), -1, WIDTH),
    (St, step(f=0), -1, FEATURES), (St, step(f=257), -1, FEATURES), (St, step(h=0), -1, HIDDEN), (St, step(h=65), -1, HIDDEN),
    (St, step(f=3), -1, MULTIPLE), (St, step(pol=0), -1, POLICIES), (St, step(pol=2), -1, POLICIES),
    (St, step(lim=-0.5), -1, LIMIT), (St, step(lim=NAN), -1, LIMIT),
    (St, step(s=-0.5), -1, MEMLIMIT), (St, step(s=NAN), -1, MEMLIMIT), (St, step(s=-INF), -1, MEMLIMIT),
    (St, step(prm=params(mode=7)), -1, MODE), (St, step(prm=params(mode=1)), -6, FAST),
    (St, step(w=WTS + 2), -1, ALIGN_W),
    (St, step(mi=MI + 2), -1, ALIGN_MEM), (St, step(mo=MO + 1), -1, ALIGN_MEM), (St, step(mi=MI + 2, mo=MI + 2), -1, ALIGN_MEM),
    (St, step(cams=CAMS + 4), -1, ALIGN_ST), (St, step(po=PO + 8), -1, ALIGN_ST),
    (St, step(po=PI), -1, OVERLAP), (St, step(vo=PO), -1, OVERLAP), (St, step(po=WTS), -1, OVERLAP),       # the feedforward step's overlaps
    (St, step(mo=MI + 4), -1, PARTIAL), (St, step(mo=MI + MEM - 4), -1, PARTIAL), (St, step(mo=MI - MEM + 4), -1, PARTIAL),
    (St, step(mo=WTS), -1, OVERLAP), (St, step(mo=WTS + 3 * POLICY - 4), -1, OVERLAP),                    # the new memory in the policies
    (St, step(mi=WTS, mo=WTS), -1, OVERLAP),                                                              # and in place there
    (St, step(mo=PI), -1, OVERLAP), (St, step(mo=VI + REC - 4), -1, OVERLAP), (St, step(mo=CAMS), -1, OVERLAP),   # in the records, in the matrices
    (St, step(mo=PO), -1, OVERLAP), (St, step(mo=VO - MEM + 4), -1, OVERLAP), (St, step(po=MO + MEM - 16), -1, OVERLAP),   # in another output
    (St, step(mi=PO), -1, OVERLAP), (St, step(mi=VO + REC - 4, mo=MO), -1, OVERLAP),                      # an output in the old memory
    (St, step(mi=MO, mo=MO, vo=MO + MEM - 16), -1, OVERLAP),                                              # in place: the memory is an output
    (St, step(scenes=0, mi=None), -1, NULLS),                                            # two faults
    (St, step(lim=-1.0, s=-1.0), -1, LIMIT),                                             # two faults
    (St, step(s=-1.0, prm=params(mode=7)), -1, MEMLIMIT),                                # two faults
    (St, step(prm=params(mode=1), w=WTS + 2), -6, FAST),                                 # two faults
    (St, step(w=WTS + 2, mi=MI + 2), -1, ALIGN_W),                                       # two faults
    (St, step(mi=MI + 2, pi=PI + 4), -1, ALIGN_MEM),                                     # two faults
    (St, step(pi=PI + 4, mo=MI + 4), -1, ALIGN_ST),                                      # two faults
    (St, step(po=PI, mo=MI + 4), -1, OVERLAP),                                           # two faults
    (St, step(mo=MI + 4, vi=MI), -1, PARTIAL),                                           # two faults
    (St, step(), -2, None), (St, step(mo=MI), -2, None), (St, step(s=INF, lim=INF), -2, None),   # good arguments, out of place and in place
    (St, step(s=0.0, lim=0.0, pol=1, f=1, h=1, width=1, mo=MI + 4 * 300), -2, None),             # the new memory next to the old
    (Ob, obs(cams=None), -1, NULLS), (Ob, obs(inst=None), -1, NULLS), (Ob, obs(w=None), -1, NULLS), (Ob, obs(mem=None), -1, NULLS),
    (Ob, obs(scenes=0), -1, SCENES), (Ob, obs(n=2049), -1, BODIES), (Ob, obs(scenes=FULL + 1, n=2048, pol=1), -6, PRODUCT),
    (Ob, obs(width=0), -1, WIDTH), (Ob, obs(f=257), -1, FEATURES), (Ob, obs(h=65), -1, HIDDEN), (Ob, obs(f=3), -1, MULTIPLE),
    (Ob, obs(pol=2), -1, POLICIES), (Ob, obs(lim=NAN), -1, LIMIT), (Ob, obs(s=-0.5), -1, MEMLIMIT), (Ob, obs(s=NAN), -1, MEMLIMIT),
    (Ob, obs(w=WTS + 2), -1, ALIGN_W), (Ob, obs(mem=MI + 2), -1, ALIGN_M1),
    (Ob, obs(cams=CAMS + 4), -1, ALIGN_OB), (Ob, obs(inst=INST + 8), -1, ALIGN_OB),
    (Ob, obs(first=1), -1, RANGE), (Ob, obs(first=300, count=1), -1, RANGE), (Ob, obs(first=0xFFFFFFFF, count=2), -1, RANGE),
    (Ob, obs(feat=None, act=None, mo=None), -1, NONE),
    (Ob, obs(feat=FEAT + 2), -1, ALIGN4), (Ob, obs(act=ACT + 1), -1, ALIGN4), (Ob, obs(mo=MO + 2), -1, ALIGN4),
    (Ob, obs(act=FEAT), -1, OVERLAP), (Ob, obs(mo=FEAT + 4 * 64 * 300 - 4), -1, OVERLAP), (Ob, obs(mo=ACT - MEM + 4), -1, OVERLAP),
    (Ob, obs(mo=MI), -1, OVERLAP), (Ob, obs(mo=MI + MEM - 4), -1, OVERLAP), (Ob, obs(mo=MI - MEM + 4), -1, OVERLAP),   # m' must be clear of the memory
    (Ob, obs(first=299, count=1, mo=MI), -1, OVERLAP),                                   # the WHOLE batch's memory is an input
    (Ob, obs(feat=MI + 4), -1, OVERLAP), (Ob, obs(act=MI + MEM - 4), -1, OVERLAP),
    (Ob, obs(mo=WTS + 3 * POLICY - 4), -1, OVERLAP), (Ob, obs(mo=CAMS), -1, OVERLAP),
    (Ob, obs(count=0), 0, None), (Ob, obs(first=300, count=0), 0, None),                 # count = 0: a checked no-op
    (Ob, obs(count=0, feat=None, act=None), 0, None), (Ob, obs(count=0, mo=None, feat=None), 0, None), (Ob, obs(count=0, mo=None, act=None), 0, None),
    (Ob, obs(count=0, mo=MI), 0, None),                                                  # (an empty output overlaps nothing)
    (Ob, obs(count=0, s=-1.0), -1, MEMLIMIT), (Ob, obs(count=0, feat=None, act=None, mo=None), -1, NONE),
    (Ob, obs(lim=-1.0, s=-1.0), -1, LIMIT),                                              # two faults
    (Ob, obs(s=-1.0, w=WTS + 2), -1, MEMLIMIT),                                          # two faults
    (Ob, obs(w=WTS + 2, mem=MI + 2), -1, ALIGN_W),                                       # two faults
    (Ob, obs(mem=MI + 2, cams=CAMS + 4), -1, ALIGN_M1),                                  # two faults
    (Ob, obs(first=301, feat=None, act=None, mo=None), -1, RANGE),                       # two faults
    (Ob, obs(mo=MO + 2, act=MO + 2), -1, ALIGN4),                                        # two faults
    (Ob, obs(), -2, None), (Ob, obs(feat=None, act=None), -2, None), (Ob, obs(mo=None), -2, None),   # good arguments
    (Ob, obs(first=150, count=100, mo=MI + MEM), -2, None),
    (Pf, perturb(prm=None), -1, NULLS), (Pf, perturb(mean=None), -1, NULLS), (Pf, perturb(theta=None), -1, NULLS),
    (Pf, perturb(floats=0), -1, FLOATS), (Pf, perturb(floats=20675), -1, FLOATS), (Pf, perturb(floats=0xFFFFFFFF), -1, FLOATS),
    (Pf, perturb(prm=ep(sigma=-0.5)), -1, SIGMA), (Pf, perturb(prm=ep(step=NAN)), -1, STEP), (Pf, perturb(prm=ep(coef=(0, 0, INF, 0, 0, 0))), -1, COEF),
    (Pf, perturb(first=4096, count=1), -1, ES_RANGE), (Pf, perturb(first=1, count=0xFFFFFFFF), -1, ES_RANGE),
    (Pf, perturb(mean=MEAN + 2), -1, ALIGN_P), (Pf, perturb(theta=THETA + 1), -1, ALIGN_P),
    (Pf, perturb(theta=MEAN), -1, OVERLAP_P), (Pf, perturb(theta=MEAN + MB - 4), -1, OVERLAP_P), (Pf, perturb(theta=MEAN - 3 * MB + 4), -1, OVERLAP_P),
    (Pf, perturb(floats=20674, theta=MEAN + 4 * 20674 - 4), -1, OVERLAP_P),
    (Pf, perturb(prm=None, floats=0), -1, NULLS),                                        # two faults
    (Pf, perturb(floats=0, prm=ep(sigma=-1.0)), -1, FLOATS),                             # two faults
    (Pf, perturb(prm=ep(sigma=NAN), count=5000), -1, SIGMA),                             # two faults
    (Pf, perturb(count=0), 0, None), (Pf, perturb(first=4096, count=0), 0, None),        # count = 0: a checked no-op
    (Pf, perturb(count=0, floats=0), -1, FLOATS),
    (Pf, perturb(), -2, None), (Pf, perturb(floats=1), -2, None), (Pf, perturb(floats=20674, first=0, count=4096), -2, None),   # good arguments
    (Pf, perturb(theta=MEAN + MB), -2, None),
    (Uf, update(prm=None), -1, NULLS), (Uf, update(score=None), -1, NULLS), (Uf, update(mean=None), -1, NULLS), (Uf, update(mean_out=None), -1, NULLS),
    (Uf, update(rank=None), -1, NULLS),
    (Uf, update(floats=0), -1, FLOATS), (Uf, update(floats=20675), -1, FLOATS),
    (Uf, update(prm=ep(sigma=INF)), -1, SIGMA), (Uf, update(prm=ep(step=INF)), -1, STEP), (Uf, update(prm=ep(coef=(NAN, 0, 0, 0, 0, 0))), -1, COEF),
    (Uf, update(scenes=0), -1, POPULATION), (Uf, update(scenes=4097), -1, POPULATION),
    (Uf, update(score=SCORE + 4), -1, ALIGN8), (Uf, update(mean=MEAN + 2), -1, ALIGN_MEAN),
    (Uf, update(mean_out=OUT + 2), -1, ALIGN4), (Uf, update(rank=RANK + 1), -1, ALIGN4),
    (Uf, update(mean_out=MEAN + 4), -1, OVERLAP), (Uf, update(mean_out=MEAN - MB + 4), -1, OVERLAP),      # neither in place nor clear of the mean
    (Uf, update(rank=MEAN + MB - 4), -1, OVERLAP), (Uf, update(fit=RANK + 8), -1, OVERLAP), (Uf, update(rep=SCORE + 80), -1, OVERLAP),
    (Uf, update(floats=20674, rank=MEAN + 4 * 20674 - 4), -1, OVERLAP),
    (Uf, update(mean_out=MEAN, rank=MEAN + 8), -1, OVERLAP),                             # in place: the mean is an output
    (Uf, update(floats=0, scenes=0), -1, FLOATS),                                        # two faults
    (Uf, update(prm=ep(sigma=-1.0), scenes=0), -1, SIGMA),                               # two faults
    (Uf, update(), -2, None), (Uf, update(mean_out=MEAN), -2, None), (Uf, update(floats=1, fit=None, rep=None), -2, None),   # good arguments
    (Uf, update(floats=20674, scenes=4096, fit=None, rep=None), -2, None), (Uf, update(rank=MEAN + MB), -2, None),
    (Sp, (None, 64, 32, 1, "w", 0.5, 1.0), -1, CTX), (Sp, (None, 0, 0, 0, None, -1.0, -1.0), -1, CTX),   # (the second: two faults)
    (Ey, (None, 0, 1, "up", "cp", 1024, FEAT, ACT, MO), -1, CTX), (Ey, (None, 0, 1, None, None, 0, None, None, None), -1, CTX),
    (Mr, (None,), -1, CTX),
    (Mg, (None, 0, 1, "out"), -1, CTX), (Mg, (None, 0, 1, None), -1, CTX),
    (Ms, (None, "out"), -1, CTX), (Ms, (None, None), -1, CTX),
    (Es, (None, 8, 7, "w", 1.0, 1.0, ep()), -1, CTX), (Es, (None, 0, 0, None, -1.0, -1.0, None), -1, CTX),
]
ROWS = [(fn, args, status, None if message is None else message.format(fn)) for fn, args, status, message in ROWS]
ENTRIES = sorted({entry for entry, _, _, _ in ROWS})


def test_no_row_expects_work_of_the_device():
    """a row that passes every check ends at the missing device (NB_ERR_NO_DEVICE) on a machine without one; the test below skips those
    rows where there is a device, since the fake addresses would be used"""
    assert all(status != _lib.NB_ERR_HIP for _, _, status, _ in ROWS)
    assert set(ENTRIES) == {St, Ob, Pf, Uf, Sp, Ey, Mr, Mg, Ms, Es} == set(SCENES_POLICY_RECURRENT_PROTOTYPES) - {"nb_policy_recurrent_floats"}
    assert all(message is None or message.startswith(entry + ": ") for entry, _, _, message in ROWS)   # every message names its entry
    assert not any(name.startswith("nb_launch_") for name in SCENES_POLICY_RECURRENT_PROTOTYPES)


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_are_the_recorded_ones(nb, entry):
    lib = _lib.load()
    device = lib.nb_device_count() > 0
    for name, args, status, message in ROWS:
        if name != entry or (status == _lib.NB_ERR_NO_DEVICE and device):
            continue
        call = [HOST[a].ctypes.data if isinstance(a, str) else (ctypes.byref(a) if isinstance(a, (_lib.NbParams, _lib.NbEsParams)) else a)
                for a in args]
        assert lib.nb_init_state(0, 0, None, None) == _lib.NB_ERR_INVALID   # a message of another entry's: "none written" shows
        before = _lib.last_error()
        assert getattr(lib, name)(*call) == status, (name, args)
        if status != _lib.NB_ERR_NO_DEVICE:
            assert _lib.last_error() == (before if message is None else message), (name, args)
            assert lib.nb_scenes_last_error(None).decode() == _lib.last_error()  # the batch's own reader of the thread's message


def test_the_shape_launches_of_the_search_keep_their_texts(nb):
    """nb_scenes_es_perturb_launch and nb_scenes_es_update_launch became wrappers of the launches above: a refused shape still names the
    entry and the shape's bound, not the mean's length"""
    lib = _lib.load()
    e = ep()
    assert lib.nb_scenes_es_perturb_launch(ctypes.byref(e), 257, 7, 0, 0, 3, MEAN, THETA, None) == -1
    assert _lib.last_error() == FEATURES.format("nb_scenes_es_perturb_launch")
    assert lib.nb_scenes_es_update_launch(ctypes.byref(e), 8, 65, 0, 3, SCORE, MEAN, OUT, RANK, FIT, REP, None) == -1
    assert _lib.last_error() == HIDDEN.format("nb_scenes_es_update_launch")
