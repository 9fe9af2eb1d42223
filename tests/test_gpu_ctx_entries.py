"""GPU tests of the layer every context entry stands on (nb_api.hip: nb_ctx, its buffers and its entries' first checks): what the base
entries of a context answer without a context, on one that holds no state and on a live one, in which order they check, and where the
text goes; and the eye rows, which seven entries share, growing and being reused across those entries.

Every status and text of section 1 was recorded on the GPU from the library as it was BEFORE the context's buffers got one owner and its
entries one preamble; the table holds that refactor, and later ones, to them byte for byte.  The scenes context has its own tables
(tests/test_scenes_api_messages.py, tests/test_gpu_scenes.py), the vision entries theirs (tests/test_gpu_vision_entries.py)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
N = 8
SENT = 0x07070707        # what every host buffer holds before a call
GUARD = 4                # words behind every buffer's end, which no call may write

# the one state of this file: eight bodies in a row along x, 3 apart, all heading +x -- every eye but the last sees the next body
# 3 ahead (near plane 1), and a frame of one pixel a unit shows the bodies around the origin
POS = np.array([[3.0 * k - 10.5, 0.25 * (k % 2), 0.0] for k in range(N)], F)
VEL = np.tile(np.array([1.0, 0.0, 0.0], F), (N, 1))


# -- 1. refusals and their order ---------------------------------------------------------------------------------------------------------
# ctx: None, 'fresh' (created, nothing uploaded) or 'live' (POS, VEL uploaded).  The blocks a row names: `pos`, `vel`, `up`, the eye
# constant `cp`, a camera `cam`, `eye`, `dir`, a 2 x 2 `skin`; the outputs a .. d, 12 KiB apart, which only a refusal may be given;
# sinks w0 .. w3 for the calls that succeed; boids parameters with a tile that is none.  A message of None: the call writes none.
# (entry, ctx, arguments behind ctx, status, message)
ROWS = [
    ('nb_upload', None, ('pos', 'vel'), -1, 'nb_upload: ctx is null'),
    ('nb_upload', None, (None, None), -1, 'nb_upload: ctx is null'),   # two faults
    ('nb_upload', 'fresh', (None, 'vel'), -1, 'nb_upload: null array'),
    ('nb_upload', 'fresh', ('pos', None), -1, 'nb_upload: null array'),
    ('nb_upload', 'live', (None, None), -1, 'nb_upload: null array'),
    ('nb_upload', 'live', ('pos', 'vel'), 0, None),
    ('nb_step', None, (1,), -1, 'nb_step: ctx is null'),
    ('nb_step', 'fresh', (1,), -5, 'nb_step: no state uploaded (call nb_upload first)'),
    ('nb_step', 'fresh', (0,), -5, 'nb_step: no state uploaded (call nb_upload first)'),
    ('nb_step', 'live', (0,), 0, None),
    ('nb_step_boids', None, (1, None), -1, 'nb_step_boids: ctx is null'),
    ('nb_step_boids', None, (1, 'tile_100'), -1, 'nb_step_boids: ctx is null'),   # two faults
    ('nb_step_boids', 'fresh', (1, None), -5, 'nb_step_boids: no state uploaded (call nb_upload first)'),
    ('nb_step_boids', 'fresh', (0, None), -5, 'nb_step_boids: no state uploaded (call nb_upload first)'),
    ('nb_step_boids', 'fresh', (1, 'tile_100'), -5, 'nb_step_boids: no state uploaded (call nb_upload first)'),   # two faults
    ('nb_step_boids', 'live', (1, 'tile_100'), -1, 'nb: boids params.tile must be 0, 256, 512 or 1024'),
    ('nb_step_boids', 'live', (0, 'tile_100'), -1, 'nb: boids params.tile must be 0, 256, 512 or 1024'),   # two faults
    ('nb_step_boids', 'live', (0, None), 0, None),
    ('nb_step_random', None, (1, 7), -1, 'nb_step_random: ctx is null'),
    ('nb_step_random', 'fresh', (1, 7), -5, 'nb_step_random: no state uploaded (call nb_upload first)'),
    ('nb_step_random', 'fresh', (0, 7), -5, 'nb_step_random: no state uploaded (call nb_upload first)'),
    ('nb_step_random', 'live', (0, 7), 0, None),
    ('nb_device_state', None, (None, None, None), -1, 'nb_device_state: ctx is null'),
    ('nb_device_state', 'fresh', (None, None, None), -5, 'nb_device_state: no state uploaded'),
    ('nb_device_state', 'live', (None, None, None), 0, None),
    ('nb_cameras', None, ('up', 'cp', 'a'), -1, 'nb_cameras: ctx is null'),
    ('nb_cameras', None, (None, 'cp', 'a'), -1, 'nb_cameras: ctx is null'),   # two faults
    ('nb_cameras', 'fresh', ('up', 'cp', 'a'), -5, 'nb_cameras: no state uploaded'),
    ('nb_cameras', 'fresh', (None, 'cp', 'a'), -1, 'nb_cameras: null argument'),   # two faults: the arguments before the state
    ('nb_cameras', 'fresh', ('up', 'cp', None), -1, 'nb_cameras: null argument'),   # two faults
    ('nb_cameras', 'live', ('up', None, 'a'), -1, 'nb_cameras: null argument'),
    ('nb_cameras', 'live', ('up', 'cp', None), -1, 'nb_cameras: null argument'),
    ('nb_cameras', 'live', ('up', 'cp', 'w0'), 0, None),
    ('nb_camera_at', None, ('eye', 'dir', 'up', 'cp', 'a'), -1, 'nb_camera_at: ctx is null'),
    ('nb_camera_at', None, ('eye', 'dir', 'up', 'cp', None), -1, 'nb_camera_at: ctx is null'),   # two faults
    ('nb_camera_at', 'fresh', (None, 'dir', 'up', 'cp', 'a'), -1, 'nb_camera_at: null argument'),
    ('nb_camera_at', 'fresh', ('eye', 'dir', 'up', 'cp', None), -1, 'nb_camera_at: null argument'),
    ('nb_camera_at', 'fresh', ('eye', 'dir', 'up', 'cp', 'w0'), 0, None),   # (it needs no state)
    ('nb_camera_at', 'live', ('eye', None, 'up', 'cp', 'a'), -1, 'nb_camera_at: null argument'),
    ('nb_camera_at', 'live', ('eye', 'dir', 'up', 'cp', 'w0'), 0, None),
    ('nb_eyes_skin', None, ('skin', 2, 2), -1, 'nb_eyes_skin: ctx is null'),
    ('nb_eyes_skin', None, ('skin', 0, 2), -1, 'nb_eyes_skin: ctx is null'),   # two faults
    ('nb_eyes_skin', 'fresh', ('skin', 0, 2), -1, 'nb_eyes_skin: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),   # (it needs no state)
    ('nb_eyes_skin', 'fresh', ('skin', 2, 2049), -1, 'nb_eyes_skin: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_eyes_skin', 'fresh', (None, 0, 0), 0, None),
    ('nb_eyes_skin', 'fresh', ('skin', 2, 2), 0, None),
    ('nb_eyes_skin', 'fresh', (None, 0, 2049), 0, None),   # (no skin: the extent is not looked at)
    ('nb_eyes_skin', 'live', ('skin', 2, 0), -1, 'nb_eyes_skin: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)'),
    ('nb_eyes_skin', 'live', (None, 0, 0), 0, None),
    ('nb_sync', None, (), -1, 'nb_sync: ctx is null'),
    ('nb_sync', 'fresh', (), 0, None),
    ('nb_sync', 'live', (), 0, None),
    ('nb_download', None, ('a', 'b', 'c'), -1, 'nb_download: ctx is null'),
    ('nb_download', 'fresh', ('a', 'b', 'c'), -5, 'nb_download: no state uploaded'),
    ('nb_download', 'fresh', (None, None, None), -5, 'nb_download: no state uploaded'),
    ('nb_download', 'live', (None, None, None), 0, None),   # (it succeeds and waits)
    ('nb_download', 'live', ('w0', 'w1', 'w2'), 0, None),
    ('nb_eyes', None, (0, 8, 'up', 'cp', 8, 0, 'a', 'b'), -1, 'nb_eyes: ctx is null'),
    ('nb_eyes', 'fresh', (0, 8, 'up', 'cp', 8, 0, 'a', 'b'), -5, 'nb_eyes: no state uploaded'),
    ('nb_eyes', 'fresh', (0, 8, None, 'cp', 8, 0, 'a', 'b'), -1, 'nb_eyes: null argument'),   # two faults
    ('nb_eyes', 'fresh', (0, 8, 'up', 'cp', 0, 0, 'a', 'b'), -1, 'nb_eyes: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),   # two faults
    ('nb_eyes', 'fresh', (0, 0, 'up', 'cp', 8, 0, 'a', 'b'), -5, 'nb_eyes: no state uploaded'),   # two faults: the state before "nothing to do"
    ('nb_eyes', 'fresh', (0, 8, 'up', 'cp', 8, 0, None, None), -1, 'nb_eyes: ids and depth are both NULL'),   # two faults
    ('nb_eyes', 'live', (0, 0, 'up', 'cp', 8, 0, 'a', 'b'), 0, None),
    ('nb_eyes', 'live', (0, 8, 'up', 'cp', 8, 0, 'w0', 'w1'), 0, None),
    ('nb_eyes_colour', None, (0, 8, 'up', 'cp', 8, 0, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_colour: ctx is null'),
    ('nb_eyes_colour', 'fresh', (0, 8, 'up', 'cp', 8, 0, 'a', 'b', 'c', 'd'), -5, 'nb_eyes_colour: no state uploaded'),
    ('nb_eyes_colour', 'fresh', (0, 8, 'up', 'cp', 8, 0, 'a', 'b', None, None), -1,
     'nb_eyes_colour: rgba and bgra8 are both NULL (ids and depth alone: nb_eyes / nb_launch_eyes)'),   # two faults
    ('nb_eyes_msaa', None, (0, 8, 'up', 'cp', 8, 0, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_msaa: ctx is null'),
    ('nb_eyes_msaa', 'fresh', (0, 8, 'up', 'cp', 8, 0, 'a', 'b', 'c', 'd'), -5, 'nb_eyes_msaa: no state uploaded'),
    ('nb_eyes_msaa', 'fresh', (0, 8, 'up', 'cp', 2049, 0, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_msaa: width must be 1 .. NB_EYES_MSAA_MAX_WIDTH (2048)'),   # two faults
    ('nb_frame', None, ('cam', 8, 8, 0, 'a', 'b', 'c', 'd'), -1, 'nb_frame: ctx is null'),
    ('nb_frame', 'fresh', ('cam', 8, 8, 0, 'a', 'b', 'c', 'd'), -5, 'nb_frame: no state uploaded'),
    ('nb_frame', 'fresh', ('cam', 8, 8, 1, 'a', 'b', 'c', 'd'), -1, 'nb_frame: flags must be 0'),   # two faults
    ('nb_frame', 'fresh', (None, 8, 8, 0, 'a', 'b', 'c', 'd'), -1, 'nb_frame: null argument'),   # two faults
    ('nb_frame_msaa', None, ('cam', 8, 8, 0, 'a', 'b', 'c', 'd'), -1, 'nb_frame_msaa: ctx is null'),
    ('nb_frame_msaa', 'fresh', ('cam', 8, 8, 0, 'a', 'b', 'c', 'd'), -5, 'nb_frame_msaa: no state uploaded'),
    ('nb_frame_msaa', 'fresh', ('cam', 8, 0, 0, 'a', 'b', 'c', 'd'), -1, 'nb_frame_msaa: width and height must be 1 .. NB_FRAME_MSAA_MAX_DIM (2048)'),   # two faults
]
BASE = ("nb_upload", "nb_step", "nb_step_boids", "nb_step_random", "nb_device_state", "nb_cameras", "nb_camera_at", "nb_eyes_skin", "nb_sync",
        "nb_download")
VIEWS = ("nb_eyes", "nb_eyes_colour", "nb_eyes_msaa", "nb_frame", "nb_frame_msaa")


def ortho_camera(side):
    """a caller camera that shows the square of `side` units around the origin, one pixel a unit at side x side, depth 0.5"""
    cam = np.zeros((4, 4), F)
    cam[0, 0], cam[1, 1], cam[3, 2], cam[3, 3] = 2 / side, 2 / side, 0.5, 1
    return cam.reshape(16)


def refusal_blocks(nb):
    """name -> a host block that outlives every call (numpy array or ctypes structure)"""
    blocks = {"pos": POS.copy(), "vel": VEL.copy(), "up": np.array([0, 0, 1], F), "cp": np.ascontiguousarray(nb.eye_constant(8), F).reshape(16),
              "cam": ortho_camera(8), "eye": np.array([0, 0, 5], F), "dir": np.array([0, 0, -1], F), "skin": np.full(16, 0.5, F),
              "tile_100": nb._lib.default_boids_params(tile=100)}
    outs = np.zeros(4 * 0x3000, np.uint8)
    blocks["outs"] = outs
    for k, name in enumerate("abcd"):
        blocks[name] = outs[k * 0x3000:(k + 1) * 0x3000]
    for k in range(4):
        blocks[f"w{k}"] = np.zeros(0x3000, np.uint8)
    return blocks


def resolve(blocks, a):
    if not isinstance(a, str):
        return a
    b = blocks[a]
    return ctypes.byref(b) if isinstance(b, ctypes.Structure) else b.ctypes.data


def test_the_table_covers_the_entries_and_the_contexts():
    assert {r[0] for r in ROWS} == set(BASE) | set(VIEWS)
    for entry in BASE:
        assert {r[1] for r in ROWS if r[0] == entry} == {None, "fresh", "live"}, entry
    for entry in VIEWS:
        mine = [r for r in ROWS if r[0] == entry]
        assert {None, "fresh"} <= {r[1] for r in mine} and {-1, -5} <= {r[3] for r in mine}, entry
    # who needs a state says so on a fresh context; nb_camera_at, nb_eyes_skin and nb_sync need none, nb_upload brings it
    needs = {r[0] for r in ROWS if r[1] == "fresh" and r[3] == -5}
    assert needs == (set(BASE) | set(VIEWS)) - {"nb_upload", "nb_camera_at", "nb_eyes_skin", "nb_sync"}


@pytest.mark.parametrize("entry", BASE + VIEWS)
def test_context_refusals_are_the_recorded_ones(nb, entry):
    from nenbody_amd import _lib

    lib = _lib.load()
    blocks = refusal_blocks(nb)
    fresh = ctypes.c_void_p()
    _lib.check(lib.nb_create(N, 1, None, ctypes.byref(fresh)))
    try:
        with nb.Scene(POS, VEL) as sc:
            for name, which, args, status, message in ROWS:
                if name != entry:
                    continue
                ctx = {None: None, "live": sc._ctx, "fresh": fresh}[which]
                # messages of other entries', so that "none written" shows: the thread's, and the context's
                assert lib.nb_init_state(0, 0, None, None) == _lib.NB_ERR_INVALID
                thread_before = _lib.last_error(None)
                assert thread_before == "nb_init_state: null array"
                if ctx is not None:
                    seeded = lib.nb_cameras(ctx, None, None, None) if name == "nb_upload" else lib.nb_upload(ctx, None, None)
                    assert seeded == _lib.NB_ERR_INVALID
                    ctx_before = _lib.last_error(ctx)
                    assert ctx_before and not ctx_before.startswith(name + ":")
                got = getattr(lib, name)(ctx, *[resolve(blocks, a) for a in args])
                assert got == status, (name, which, args, _lib.last_error(ctx))
                if ctx is None:     # the text goes to the thread
                    assert _lib.last_error(None) == message, (name, which, args)
                else:               # the text goes to the context, and the thread's stays
                    assert _lib.last_error(ctx) == (ctx_before if message is None else message), (name, which, args)
                    assert _lib.last_error(None) == thread_before, (name, which, args)
            assert sc.steps_done == 0 and not blocks["outs"].any()       # no row stepped, no refusal wrote an output
            assert lib.nb_steps_done(fresh) == 0
            p, v = sc.state()
            assert (p.view(np.uint32) == POS.view(np.uint32)).all() and (v.view(np.uint32) == VEL.view(np.uint32)).all()
    finally:
        lib.nb_destroy(fresh)


# -- 2. the eye rows across the seven entries that share them -----------------------------------------------------------------------------
# One context goes through the sequence below; every output of every call is, bit for bit, what the same call gives on a context that
# has done nothing else (same state; the same skin where the call samples one).  The rows' capacities count different things -- words of
# ids and depth, columns of rgba and bgra8, eight words a column under 8 samples -- and the sizes are the smallest at which a capacity
# kept in the wrong unit, or a row not regrown, shows: width 16 under 8 samples needs 1 024 words of ids where width 64 left 512.
def guarded_call(sc, entry, head, words):
    """`entry` on sc's context with the arguments `head` and one output of words[k] words each: those outputs as uint32 arrays.
    Every output has GUARD words behind it, which the call must leave alone."""
    from nenbody_amd import _lib

    bufs = [np.full(w + GUARD, SENT, np.uint32) for w in words]
    _lib.check(getattr(sc._lib, entry)(sc._ctx, *head, *[b.ctypes.data for b in bufs]), sc._ctx)
    for k, b in enumerate(bufs):
        assert (b[-GUARD:] == SENT).all(), (entry, k)
    return [b[:-GUARD] for b in bufs]


def test_eye_rows_are_shared_across_the_entries(nb):
    from nenbody_amd import _lib

    up = np.array([0, 0, 1], F)
    cp = {w: np.ascontiguousarray(nb.eye_constant(w), F).reshape(16) for w in (8, 16, 64)}
    cam = {s: ortho_camera(s) for s in (8, 16)}
    skins = {2: (np.arange(2 * 2 * 4, dtype=F) + 1) / F(17), 4: (np.arange(4 * 4 * 4, dtype=F)[::-1] + 1) / F(65)}
    NONE = _lib.NB_EYES_NONE

    def eye_head(width):
        return (0, N, up.ctypes.data, cp[width].ctypes.data, width, 0)

    def frame_head(side):
        return (cam[side].ctypes.data, side, side, 0)

    colour8 = ("nb_eyes_colour", eye_head(8), (N * 8, N * 8, N * 8 * 4, N * 8))
    # (what the call is, the skin's side it samples -- None: whatever is set, which is none --, entry, arguments, words of each output)
    sequence = [
        ("eyes at width 8", None, "nb_eyes", eye_head(8), (N * 8, N * 8)),
        ("colour at width 64", None, "nb_eyes_colour", eye_head(64), (N * 64, N * 64, N * 64 * 4, N * 64)),
        ("8 samples at width 16", None, "nb_eyes_msaa", eye_head(16), (N * 16 * 8, N * 16 * 8, N * 16 * 4, N * 16)),
        ("frame 8 x 8", None, "nb_frame", frame_head(8), (64, 64, 64 * 4, 64)),
        ("frame 16 x 16 under 8 samples", None, "nb_frame_msaa", frame_head(16), (256 * 8, 256 * 8, 256 * 4, 256)),
        ("eyes at width 8 again", None, "nb_eyes", eye_head(8), (N * 8, N * 8)),
        ("located at width 64", None, "nb_eyes_located", eye_head(64), (N, N * 64, N * 64, N * 64, N * 64, N * 64 * 4)),
        ("colour at width 8, skin 2 x 2", 2) + colour8,
        ("colour at width 8, skin 4 x 4", 4) + colour8,
        ("colour at width 8, no skin", 0) + colour8,
        ("download", None, "nb_download", (), (N * 3, N * 3, N * 16)),
    ]

    def set_skin(sc, side):
        if side is None:
            return
        a = skins.get(side)
        _lib.check(sc._lib.nb_eyes_skin(sc._ctx, None if a is None else a.ctypes.data, side, side), sc._ctx)

    results = {}
    with nb.Scene(POS, VEL) as veteran:
        for what, side, entry, head, words in sequence:
            set_skin(veteran, side)
            got = guarded_call(veteran, entry, head, words)
            with nb.Scene(POS, VEL) as novice:
                set_skin(novice, side)
                want = guarded_call(novice, entry, head, words)
            for k, (g, x) in enumerate(zip(got, want)):
                assert (g == x).all(), (what, k, np.nonzero(g != x)[0][:8])
            results[what] = got
        assert veteran.steps_done == 0
    # the calls show something: eyes that see a body, pixels a body covers, a skin that colours what the white one leaves white
    for what in ("eyes at width 8", "colour at width 64", "8 samples at width 16", "frame 8 x 8", "frame 16 x 16 under 8 samples"):
        ids = results[what][0]
        assert (ids != NONE).any() and (ids == NONE).any() and (ids[ids != NONE] < N).all(), what
    assert (results["eyes at width 8"][0] == results["eyes at width 8 again"][0]).all()
    assert (results["located at width 64"][0] > 0).sum() >= N - 2
    assert (results["colour at width 8, skin 2 x 2"][2] != results["colour at width 8, no skin"][2]).any()
    assert (results["colour at width 8, skin 2 x 2"][2] != results["colour at width 8, skin 4 x 4"][2]).any()
    assert (results["download"][0] == POS.view(np.uint32).reshape(-1)).all() and (results["download"][1] == VEL.view(np.uint32).reshape(-1)).all()
