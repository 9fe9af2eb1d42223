"""What the scene-batch entries answer to arguments they must refuse: the status and the full nb_last_error()
text, as a table in the manner of test_launch_api_messages.py.

Each row is an entry, arguments that fail validation before anything touches the device (the device addresses are fake and never
dereferenced), the status and the message.  A message of None means the call writes none (k = 0 on good arguments succeeds without
work).  Rows marked "two faults" have two arguments wrong at once and pin which check comes first.  No row may reach the device: on a
machine with a GPU the fake addresses would be used.  (NB_ERR_STATE before an upload needs a context, hence a device: tests/test_gpu_scenes.py.)
"""
import ctypes

import pytest

from nenbody_amd import _lib

A, B = 0x100000, 0x4000000                                    # fake device addresses, 16-byte aligned, 63 MiB apart
FULL = (1 << 27) // 2048                                      # scenes of 2 048 bodies that reach the product limit exactly


def _params(**kw):
    def make():
        p = _lib.default_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    return make


def _boids(**kw):
    def make():
        p = _lib.default_boids_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    return make


# the blocks a row names
PARAMS = {
    "strict": _params(),
    "tile512": _params(tile=512),
    "fast": _params(mode=_lib.NB_MODE_FAST),
    "mode7": _params(mode=7),
    "tile100": _params(tile=100),
    "fast_tile100": _params(mode=_lib.NB_MODE_FAST, tile=100),
    "boids": _boids(),
    "boids_tile100": _boids(tile=100),
    "out": ctypes.c_void_p,
}

G, Bo, C = "nb_scenes_nbody_step_launch", "nb_scenes_boids_step_launch", "nb_scenes_create"
NULLS = "{}: pos and vel must be non-null"
SCENES = "{}: scenes must be at least 1"
BODIES = "{}: n must be 1 .. NB_SCENES_MAX_BODIES (2048)"
PRODUCT = "{}: scenes * n must be at most 2^27"
MODE = "{}: params.mode must be NB_MODE_STRICT or NB_MODE_FAST"
FAST = "{}: a scene batch steps STRICT only (params.mode is NB_MODE_FAST)"
TILE = "{}: params.tile must be 0, 256, 512 or 1024"
ALIGN = "{}: pos and vel must be 16-byte aligned"
OVERLAP = "{}: pos and vel must not overlap"

# (entry, arguments, status, message)
ROWS = []
for fn, good in ((G, "strict"), (Bo, "boids")):
    ROWS += [
        (fn, (good, 3, 100, 1, None, B, None), -1, NULLS),
        (fn, (good, 3, 100, 1, A, None, None), -1, NULLS),
        (fn, (None, 3, 100, 1, None, None, None), -1, NULLS),
        (fn, (good, 0, 100, 1, A, B, None), -1, SCENES),
        (fn, (good, 3, 0, 1, A, B, None), -1, BODIES),
        (fn, (good, 3, 2049, 1, A, B, None), -1, BODIES),
        (fn, (None, 3, 0xFFFFFFFF, 1, A, B, None), -1, BODIES),
        (fn, (good, FULL + 1, 2048, 1, A, B, None), -6, PRODUCT),
        (fn, (good, (1 << 27) + 1, 1, 1, A, B, None), -6, PRODUCT),
        (fn, (good, 0xFFFFFFFF, 2048, 1, A, B, None), -6, PRODUCT),
        (fn, (good, 3, 100, 1, A + 4, B, None), -1, ALIGN),
        (fn, (good, 3, 100, 1, A, B + 8, None), -1, ALIGN),
        (fn, (good, 3, 100, 1, A, A, None), -1, OVERLAP),
        (fn, (good, 3, 100, 1, A, A + 16 * 299, None), -1, OVERLAP),
        (fn, (good, 3, 100, 1, A + 16 * 299, A, None), -1, OVERLAP),
        (fn, (good, 3, 100, 0, A, A + 16 * 300, None), 0, None),                 # adjacent, not overlapping; k = 0: no work
        (fn, (None, 3, 100, 0, A, B, None), 0, None),
        (fn, (good, FULL, 2048, 0, A, A + (16 << 27), None), 0, None),           # the product limit itself
        (fn, (good, 3, 100, 0, A + 4, B, None), -1, ALIGN),                      # k = 0 is a CHECKED no-op
        (fn, (good, 0, 100, 0, A, B, None), -1, SCENES),
        (fn, (good, 0, 100, 1, None, B, None), -1, NULLS),                       # two faults
        (fn, (good, 0, 0, 1, A, B, None), -1, SCENES),                           # two faults
        (fn, (good, FULL + 1, 2049, 1, A, B, None), -1, BODIES),                 # two faults
        (fn, (good, FULL + 1, 2048, 1, A + 4, B, None), -6, PRODUCT),            # two faults
        (fn, (good, 3, 100, 1, A + 4, A + 4, None), -1, ALIGN),                  # two faults
    ]
ROWS += [
    (G, ("tile512", 3, 100, 0, A, B, None), 0, None),
    (G, ("mode7", 3, 100, 1, A, B, None), -1, MODE),
    (G, ("fast", 3, 100, 1, A, B, None), -6, FAST),
    (G, ("fast", 3, 100, 0, A, B, None), -6, FAST),
    (G, ("tile100", 3, 100, 1, A, B, None), -1, TILE),
    (G, ("fast_tile100", 3, 100, 1, A, B, None), -6, FAST),                      # two faults
    (G, ("fast", FULL + 1, 2048, 1, A, B, None), -6, PRODUCT),                   # two faults
    (G, ("fast", 3, 100, 1, A + 4, B, None), -6, FAST),                          # two faults
    (G, ("tile100", 3, 100, 1, A, A, None), -1, TILE),                           # two faults
    (Bo, ("boids_tile100", 3, 100, 1, A, B, None), -1, TILE),
    (Bo, ("boids_tile100", 3, 2049, 1, A, B, None), -1, BODIES),                 # two faults
    (Bo, ("boids_tile100", 3, 100, 1, A + 8, B, None), -1, TILE),                # two faults
    (C, (3, 100, "strict", None), -1, "{}: out is null"),
    (C, (0, 100, "strict", None), -1, "{}: out is null"),                        # two faults
    (C, (0, 100, "strict", "out"), -1, SCENES),
    (C, (3, 0, None, "out"), -1, BODIES),
    (C, (3, 2049, "strict", "out"), -1, BODIES),
    (C, (FULL + 1, 2048, "strict", "out"), -6, PRODUCT),
    (C, (3, 100, "mode7", "out"), -1, MODE),
    (C, (3, 100, "fast", "out"), -6, FAST),
    (C, (3, 100, "tile100", "out"), -1, TILE),
    (C, (0, 100, "fast", "out"), -1, SCENES),                                    # two faults
    (C, (FULL + 1, 2048, "fast", "out"), -6, PRODUCT),                           # two faults
    ("nb_scenes_upload", (None, A, B), -1, "{}: ctx is null"),
    ("nb_scenes_step", (None, 1), -1, "{}: ctx is null"),
    ("nb_scenes_step_boids", (None, 1, None), -1, "{}: ctx is null"),
    ("nb_scenes_step_boids", (None, 1, "boids_tile100"), -1, "{}: ctx is null"),   # two faults
    ("nb_scenes_download", (None, A, A, A), -1, "{}: ctx is null"),
    ("nb_scenes_download", (None, None, None, None), -1, "{}: ctx is null"),       # two faults
    ("nb_scenes_device_state", (None, None, None, None), -1, "{}: ctx is null"),
    ("nb_scenes_sync", (None,), -1, "{}: ctx is null"),
]
ROWS = [(fn, args, status, None if message is None else message.format(fn)) for fn, args, status, message in ROWS]
ENTRIES = sorted({entry for entry, _, _, _ in ROWS})


def test_no_row_expects_the_device():
    assert all(status != _lib.NB_ERR_NO_DEVICE and status != _lib.NB_ERR_HIP for _, _, status, _ in ROWS)
    assert set(ENTRIES) == {G, Bo, C, "nb_scenes_upload", "nb_scenes_step", "nb_scenes_step_boids", "nb_scenes_download",
                            "nb_scenes_device_state", "nb_scenes_sync"}
    assert all(message is None or message.startswith(entry + ": ") for entry, _, _, message in ROWS)   # every message names its entry


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_are_the_recorded_ones(nb, entry):
    lib = _lib.load()
    for name, args, status, message in ROWS:
        if name != entry:
            continue
        held = [PARAMS[a]() if isinstance(a, str) else a for a in args]   # (keeps the blocks alive over the call)
        call = [ctypes.byref(a) if isinstance(a, (ctypes.Structure, ctypes.c_void_p)) else a for a in held]
        assert lib.nb_init_state(0, 0, None, None) == _lib.NB_ERR_INVALID   # a message of another entry's: "none written" shows
        before = _lib.last_error()
        assert getattr(lib, name)(*call) == status, (name, args)
        assert _lib.last_error() == (before if message is None else message), (name, args)
        got = lib.nb_scenes_last_error(None)                               # the batch's own reader of the thread's message
        assert got.decode() == _lib.last_error()
        for h in held:
            assert not isinstance(h, ctypes.c_void_p) or h.value is None   # a refused create hands out nothing


def test_null_context_readers(nb):
    lib = _lib.load()
    assert lib.nb_scenes_steps(None) == 0
    lib.nb_scenes_destroy(None)
