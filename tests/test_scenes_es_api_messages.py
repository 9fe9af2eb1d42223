"""What the entries of the scene batches' evolution-strategies generation answer to arguments they must
refuse: the status and the full nb_last_error() text, as a table in the manner of test_scenes_score_api_messages.py.

Each row is an entry, arguments that fail validation before anything touches the device (the device addresses are fake and never
dereferenced; ep is a host structure, which the launches do read), the status and the message.  Rows marked "two faults" have two
arguments wrong at once and pin which check comes first.  No row may put the device to work: on a machine with a GPU the fake
addresses would be used.  Some rows of the launches pass every check and end at NB_ERR_NO_DEVICE, which shows that the table's good
arguments are good; where a device is present they are left out.  (The context's own refusals need a context, hence a device:
tests/test_gpu_scenes_es.py.)
"""
import ctypes
import math

import numpy as np
import pytest

from nenbody_amd import _lib
from nenbody_amd._lib import ES_PROTOTYPES   # (the parent commit has no such table: the file fails here)

MEAN, THETA, SCORE, RANK, FIT, REP, OUT = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000   # 256 MiB apart
INF, NAN = math.inf, math.nan
M87 = 8 * 7 + 7 + 14 + 2                                     # policy_floats(8, 7) = 79
MB = 4 * M87                                                 # the bytes of a mean

HOST = {"mean": np.zeros(M87, np.float32), "out": np.zeros(64, np.uint8)}

Pl, Ul, Es, Ep, Eu, Em, Er, Eg, Ke, Rw = ("nb_scenes_es_perturb_launch", "nb_scenes_es_update_launch", "nb_scenes_es_set", "nb_scenes_es_perturb",
                                          "nb_scenes_es_update", "nb_scenes_es_mean", "nb_scenes_es_result", "nb_scenes_es_generation",
                                          "nb_scenes_keep", "nb_scenes_rewind")
NULLS = "{}: null argument"
FEATURES = "{}: features must be 1 .. NB_POLICY_MAX_FEATURES (256)"
HIDDEN = "{}: hidden must be 1 .. NB_POLICY_MAX_HIDDEN (64)"
SIGMA = "{}: sigma must be at least 0 and finite"
STEP = "{}: step must be finite"
COEF = "{}: coef must be finite"
RANGE = "{}: scenes [first_scene, first_scene + count) must lie in 0 .. NB_ES_MAX_POPULATION (4096)"
POPULATION = "{}: scenes must be 1 .. NB_ES_MAX_POPULATION (4096)"
ALIGN_P = "{}: mean and theta_out must be 4-byte aligned"
OVERLAP_P = "{}: theta_out must not overlap mean"
ALIGN8 = "{}: score must be 8-byte aligned"
ALIGN_M = "{}: mean must be 4-byte aligned"
ALIGN4 = "{}: the outputs must be 4-byte aligned"
ALIAS = "{}: the outputs must not overlap each other or an input"
CTX = "{}: ctx is null"


def ep(sigma=0.5, step=0.01, coef=(0, 0, 0, 0, -1, 0), seed=1234):
    return _lib.NbEsParams(sigma, step, (ctypes.c_float * 6)(*coef), seed)


def coef_with(i, v):
    c = [0.0] * 6
    c[i] = v
    return tuple(c)


def perturb(prm="default", features=8, hidden=7, g=0, first=0, count=3, mean=MEAN, theta=THETA):
    return (ep() if prm == "default" else prm, features, hidden, g, first, count, mean, theta, None)


def update(prm="default", features=8, hidden=7, g=0, scenes=3, score=SCORE, mean=MEAN, mean_out=OUT, rank=RANK, fit=FIT, rep=REP):
    return (ep() if prm == "default" else prm, features, hidden, g, scenes, score, mean, mean_out, rank, fit, rep, None)


# (entry, arguments, status, message)
ROWS = [
    (Pl, perturb(prm=None), -1, NULLS), (Pl, perturb(mean=None), -1, NULLS), (Pl, perturb(theta=None), -1, NULLS),
    (Pl, perturb(features=0), -1, FEATURES), (Pl, perturb(features=257), -1, FEATURES), (Pl, perturb(hidden=0), -1, HIDDEN), (Pl, perturb(hidden=65), -1, HIDDEN),
    (Pl, perturb(prm=ep(sigma=-0.5)), -1, SIGMA), (Pl, perturb(prm=ep(sigma=NAN)), -1, SIGMA), (Pl, perturb(prm=ep(sigma=INF)), -1, SIGMA),
    (Pl, perturb(prm=ep(sigma=-INF)), -1, SIGMA),
    (Pl, perturb(prm=ep(step=NAN)), -1, STEP), (Pl, perturb(prm=ep(step=INF)), -1, STEP), (Pl, perturb(prm=ep(step=-INF)), -1, STEP),
] + [(Pl, perturb(prm=ep(coef=coef_with(i, v))), -1, COEF) for i in range(6) for v in (NAN, INF, -INF)] + [
    (Pl, perturb(first=4096, count=1), -1, RANGE), (Pl, perturb(first=0, count=4097), -1, RANGE), (Pl, perturb(first=4097, count=0), -1, RANGE),
    (Pl, perturb(first=0xFFFFFFFF, count=2), -1, RANGE), (Pl, perturb(first=1, count=0xFFFFFFFF), -1, RANGE),
    (Pl, perturb(mean=MEAN + 2), -1, ALIGN_P), (Pl, perturb(theta=THETA + 1), -1, ALIGN_P), (Pl, perturb(mean=MEAN + 3, theta=THETA + 2), -1, ALIGN_P),
    (Pl, perturb(theta=MEAN), -1, OVERLAP_P), (Pl, perturb(theta=MEAN + MB - 4), -1, OVERLAP_P), (Pl, perturb(theta=MEAN - 3 * MB + 4), -1, OVERLAP_P),
    (Pl, perturb(prm=None, features=0), -1, NULLS),                                      # two faults
    (Pl, perturb(features=0, hidden=0), -1, FEATURES),                                   # two faults
    (Pl, perturb(hidden=65, prm=ep(sigma=-1.0)), -1, HIDDEN),                            # two faults
    (Pl, perturb(prm=ep(sigma=NAN, step=NAN)), -1, SIGMA),                               # two faults
    (Pl, perturb(prm=ep(step=NAN, coef=coef_with(0, NAN))), -1, STEP),                   # two faults
    (Pl, perturb(prm=ep(coef=coef_with(5, NAN)), count=5000), -1, COEF),                 # two faults
    (Pl, perturb(count=5000, mean=MEAN + 1), -1, RANGE),                                 # two faults
    (Pl, perturb(mean=MEAN + 2, theta=MEAN + 2), -1, ALIGN_P),                           # two faults
    (Pl, perturb(count=0, theta=MEAN + 2), -1, ALIGN_P),                                 # count = 0 is checked
    (Pl, perturb(count=0), 0, None), (Pl, perturb(first=4096, count=0), 0, None),        # count = 0: a checked no-op, no device needed
    (Pl, perturb(count=0, theta=MEAN), 0, None),                                         # (an empty output overlaps nothing)
    (Pl, perturb(), -2, None), (Pl, perturb(first=4095, count=1, g=0xFFFFFFFF, prm=ep(sigma=0.0, seed=(1 << 64) - 1)), -2, None),   # good arguments
    (Pl, perturb(theta=MEAN + MB), -2, None), (Pl, perturb(theta=MEAN - 3 * MB), -2, None),                                         # the population next to the mean
    (Ul, update(prm=None), -1, NULLS), (Ul, update(score=None), -1, NULLS), (Ul, update(mean=None), -1, NULLS), (Ul, update(mean_out=None), -1, NULLS),
    (Ul, update(rank=None), -1, NULLS),
    (Ul, update(features=0), -1, FEATURES), (Ul, update(features=257), -1, FEATURES), (Ul, update(hidden=0), -1, HIDDEN), (Ul, update(hidden=65), -1, HIDDEN),
    (Ul, update(prm=ep(sigma=-0.5)), -1, SIGMA), (Ul, update(prm=ep(sigma=NAN)), -1, SIGMA), (Ul, update(prm=ep(sigma=INF)), -1, SIGMA),
    (Ul, update(prm=ep(step=NAN)), -1, STEP), (Ul, update(prm=ep(step=-INF)), -1, STEP),
] + [(Ul, update(prm=ep(coef=coef_with(i, v))), -1, COEF) for i in range(6) for v in (NAN, INF)] + [
    (Ul, update(scenes=0), -1, POPULATION), (Ul, update(scenes=4097), -1, POPULATION), (Ul, update(scenes=0xFFFFFFFF), -1, POPULATION),
    (Ul, update(score=SCORE + 4), -1, ALIGN8), (Ul, update(score=SCORE + 1), -1, ALIGN8),
    (Ul, update(mean=MEAN + 2), -1, ALIGN_M), (Ul, update(mean=MEAN + 1, mean_out=MEAN + 1), -1, ALIGN_M),
    (Ul, update(mean_out=OUT + 2), -1, ALIGN4), (Ul, update(rank=RANK + 1), -1, ALIGN4), (Ul, update(fit=FIT + 2), -1, ALIGN4), (Ul, update(rep=REP + 3), -1, ALIGN4),
    (Ul, update(mean_out=MEAN + 4), -1, ALIAS), (Ul, update(mean_out=MEAN - MB + 4), -1, ALIAS),      # neither in place nor clear of the mean
    (Ul, update(rank=SCORE), -1, ALIAS), (Ul, update(rank=SCORE + 92), -1, ALIAS), (Ul, update(rank=MEAN + MB - 4), -1, ALIAS),
    (Ul, update(fit=SCORE + 32), -1, ALIAS), (Ul, update(fit=MEAN), -1, ALIAS), (Ul, update(fit=RANK), -1, ALIAS), (Ul, update(fit=RANK + 8), -1, ALIAS),
    (Ul, update(rep=RANK + 8), -1, ALIAS), (Ul, update(rep=FIT - 12), -1, ALIAS), (Ul, update(rep=SCORE + 80), -1, ALIAS), (Ul, update(rep=MEAN + MB - 4), -1, ALIAS),
    (Ul, update(mean_out=RANK - MB + 4), -1, ALIAS), (Ul, update(mean_out=SCORE + 92), -1, ALIAS),
    (Ul, update(mean_out=MEAN, rank=MEAN + 8), -1, ALIAS), (Ul, update(mean_out=MEAN, rep=MEAN + MB - 4), -1, ALIAS),   # in place: the mean is an output
    (Ul, update(prm=None, scenes=0), -1, NULLS),                                         # two faults
    (Ul, update(features=257, prm=ep(step=INF)), -1, FEATURES),                          # two faults
    (Ul, update(prm=ep(sigma=-1.0), scenes=0), -1, SIGMA),                               # two faults
    (Ul, update(scenes=0, score=SCORE + 4), -1, POPULATION),                             # two faults
    (Ul, update(score=SCORE + 4, mean=MEAN + 2), -1, ALIGN8),                            # two faults
    (Ul, update(mean=MEAN + 2, rank=RANK + 2), -1, ALIGN_M),                             # two faults
    (Ul, update(rank=SCORE + 2), -1, ALIGN4),                                            # two faults
    (Ul, update(), -2, None), (Ul, update(mean_out=MEAN), -2, None), (Ul, update(fit=None, rep=None), -2, None),   # good arguments: out of place, in place
    (Ul, update(scenes=4096, g=0xFFFFFFFF, features=256, hidden=64, rank=RANK, fit=None, rep=RANK + 4 * 4096), -2, None),
    (Ul, update(rank=SCORE + 96, fit=SCORE - 12, rep=MEAN + MB, mean_out=MEAN - MB), -2, None),                    # everything next to its neighbour
    (Es, (None, 8, 7, "mean", 1.0, ep()), -1, CTX), (Es, (None, 0, 0, None, -1.0, None), -1, CTX),                 # (the second: two faults)
    (Ep, (None,), -1, CTX),
    (Eu, (None,), -1, CTX),
    (Em, (None, "out"), -1, CTX), (Em, (None, None), -1, CTX),                           # (the second: two faults)
    (Er, (None, "out", None, None), -1, CTX), (Er, (None, None, None, None), -1, CTX),
    (Ke, (None,), -1, CTX),
    (Rw, (None,), -1, CTX),
]
ROWS = [(fn, args, status, None if message is None else message.format(fn)) for fn, args, status, message in ROWS]
ENTRIES = sorted({entry for entry, _, _, _ in ROWS})


def test_no_row_expects_work_of_the_device():
    """a row that passes every check ends at the missing device (NB_ERR_NO_DEVICE) on a machine without one; the test below skips those
    rows where there is a device, since the fake addresses would be used"""
    assert all(status != _lib.NB_ERR_HIP for _, _, status, _ in ROWS)
    assert set(ENTRIES) == {Pl, Ul, Es, Ep, Eu, Em, Er, Ke, Rw} == set(ES_PROTOTYPES) - {Eg}
    assert all(message is None or message.startswith(entry + ": ") for entry, _, _, message in ROWS)   # every message names its entry
    assert not any(name.startswith("nb_launch_") for name in ES_PROTOTYPES)
    assert ctypes.sizeof(_lib.NbEsParams) == 40 and _lib.NbEsParams.seed.offset == 32 and ctypes.sizeof(_lib.NbEsReport) == 16


def test_generation_of_no_context_is_zero(nb):
    assert _lib.load().nb_scenes_es_generation(None) == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_are_the_recorded_ones(nb, entry):
    lib = _lib.load()
    device = lib.nb_device_count() > 0
    for name, args, status, message in ROWS:
        if name != entry or (status == _lib.NB_ERR_NO_DEVICE and device):
            continue
        call = [HOST[a].ctypes.data if isinstance(a, str) else (ctypes.byref(a) if isinstance(a, _lib.NbEsParams) else a) for a in args]
        assert lib.nb_init_state(0, 0, None, None) == _lib.NB_ERR_INVALID   # a message of another entry's: "none written" shows
        before = _lib.last_error()
        assert getattr(lib, name)(*call) == status, (name, args)
        if status != _lib.NB_ERR_NO_DEVICE:
            assert _lib.last_error() == (before if message is None else message), (name, args)
            assert lib.nb_scenes_last_error(None).decode() == _lib.last_error()  # the batch's own reader of the thread's message
