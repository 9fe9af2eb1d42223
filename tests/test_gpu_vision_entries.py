"""GPU tests of the host side of the vision entries (nb_vision_api.inc; DESIGN.md sections 12 and 13): what the four context entries
nb_eyes_seen, nb_eyes_located, nb_step_boids_seen and nb_step_nbody_located refuse and in which order, which device rows the row
entries compute for every subset of their outputs, the context's chain against the stateless launches chained by hand, and the
context's rows growing and shrinking across the entries.  The kernels themselves are tests/test_gpu_seen.py's and
tests/test_gpu_located.py's to check."""
import ctypes
import itertools

import numpy as np
import pytest

import located_restatement as L
import seen_restatement as S
import test_gpu_located as TL
import test_gpu_seen as TS

pytestmark = pytest.mark.gpu

F = np.float32
UP = np.array([0, 0, 1], F)
SENT = 0x07070707        # what every host buffer holds before a call
GUARD = 4                # words behind every buffer's end, which no call may write


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# -- 1. refusals of the context entries, a live context -------------------------------------------------------------------------------------
# A Scene of 8 bodies, rows of 64 pixels.  The blocks a row names: `up`; the eye constant `cp` and four constants that L6 refuses;
# the host outputs a .. f, 12 KiB apart (the largest, seen_rel of 8 eyes, has 8 KiB); boids parameters with a tile that is none.
# ctx: 'live' (the Scene's), 'fresh' (created, nothing uploaded) or None.  A message of None: the call writes none.
# (entry, ctx, arguments behind ctx, status, message)
ROWS = [
    ('nb_eyes_seen', None, (0, 8, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_seen: ctx is null'),
    ('nb_eyes_seen', 'live', (0, 8, None, 'cp', 64, 0, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_seen: null argument'),
    ('nb_eyes_seen', 'live', (0, 8, 'up', None, 64, 0, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_seen: null argument'),
    ('nb_eyes_seen', 'live', (0, 8, 'up', 'cp', 0, 0, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_seen: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_eyes_seen', 'live', (0, 1, 'up', 'cp', 4097, 0, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_seen: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_eyes_seen', 'live', (4, 5, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_seen: eyes [first, first + count) exceed the set'),
    ('nb_eyes_seen', 'live', (0xffffffff, 2, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_seen: eyes [first, first + count) exceed the set'),
    ('nb_eyes_seen', 'live', (0, 8, 'up', 'cp', 64, 2, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_seen: unknown flag bits'),
    ('nb_eyes_seen', 'live', (0, 8, 'up', 'cp', 64, 0, None, None, None, None), -1, 'nb_eyes_seen: seen_count, seen_ids, seen_depth and seen_cols are all NULL'),
    ('nb_eyes_seen', 'live', (0, 8, 'up', 'cp', 64, 0, 'a', 'b', 'b', 'd'), -1, 'nb_eyes_seen: the outputs must not alias each other or an input'),
    ('nb_eyes_seen', 'live', (0, 8, 'up', 'cp', 64, 0, None, 'b', None, 'b+2044'), -1, 'nb_eyes_seen: the outputs must not alias each other or an input'),
    ('nb_eyes_seen', 'live', (0, 8, 'up', 'cp', 64, 0, 'up', 'b', 'c', 'd'), -1, 'nb_eyes_seen: the outputs must not alias each other or an input'),
    ('nb_eyes_seen', 'live', (0, 8, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'cp+60'), -1, 'nb_eyes_seen: the outputs must not alias each other or an input'),
    ('nb_eyes_seen', 'fresh', (0, 8, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd'), -5, 'nb_eyes_seen: no state uploaded'),
    ('nb_eyes_seen', 'fresh', (0, 0, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd'), -5, 'nb_eyes_seen: no state uploaded'),
    ('nb_eyes_seen', 'live', (0, 0, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd'), 0, None),
    ('nb_eyes_seen', 'live', (8, 0, 'up', 'cp', 64, 1, 'a', None, None, None), 0, None),
    ('nb_eyes_seen', 'live', (0, 8, None, 'cp', 0, 0, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_seen: null argument'),   # two faults
    ('nb_eyes_seen', 'live', (4, 5, 'up', 'cp', 0, 2, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_seen: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),   # two faults
    ('nb_eyes_seen', 'live', (4, 5, 'up', 'cp', 64, 2, 'a', 'b', 'c', 'd'), -1, 'nb_eyes_seen: eyes [first, first + count) exceed the set'),   # two faults
    ('nb_eyes_seen', 'live', (0, 8, 'up', 'cp', 64, 2, None, None, None, None), -1, 'nb_eyes_seen: unknown flag bits'),   # two faults
    ('nb_eyes_seen', 'fresh', (0, 8, 'up', 'cp', 64, 0, None, None, None, None), -1, 'nb_eyes_seen: seen_count, seen_ids, seen_depth and seen_cols are all NULL'),   # two faults
    ('nb_eyes_seen', 'fresh', (0, 8, 'up', 'cp', 64, 0, 'a', 'a', 'c', 'd'), -1, 'nb_eyes_seen: the outputs must not alias each other or an input'),   # two faults
    ('nb_eyes_located', None, (0, 8, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: ctx is null'),
    ('nb_eyes_located', 'live', (0, 8, None, 'cp', 64, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: null argument'),
    ('nb_eyes_located', 'live', (0, 8, 'up', None, 64, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: null argument'),
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp', 0, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_eyes_located', 'live', (0, 1, 'up', 'cp', 4097, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_eyes_located', 'live', (4, 5, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: eyes [first, first + count) exceed the set'),
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp', 64, 2, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: unknown flag bits'),
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp_ortho', 64, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: cp16 cannot be inverted: cp16[11] must be -1 (a perspective constant as nb_camera_constant forms it)'),
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp_15', 64, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: cp16 cannot be inverted: cp16[15] must be 0 (a perspective constant as nb_camera_constant forms it)'),
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp_0', 64, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: cp16 cannot be inverted: cp16[0] must not be 0 (a perspective constant as nb_camera_constant forms it)'),
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp_14', 64, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: cp16 cannot be inverted: cp16[14] must not be 0 (a perspective constant as nb_camera_constant forms it)'),
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp', 64, 0, None, None, None, None, None, None), -1, 'nb_eyes_located: seen_count, seen_ids, seen_depth, seen_cols, seen_col and seen_rel are all NULL'),
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd', 'e', 'e'), -1, 'nb_eyes_located: the outputs must not alias each other or an input'),
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp', 64, 0, None, None, None, None, 'f+8188', 'f'), -1, 'nb_eyes_located: the outputs must not alias each other or an input'),
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp', 64, 0, 'a', None, None, None, None, 'a+16'), -1, 'nb_eyes_located: the outputs must not alias each other or an input'),
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd', 'up+8', 'f'), -1, 'nb_eyes_located: the outputs must not alias each other or an input'),
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd', 'e', 'cp'), -1, 'nb_eyes_located: the outputs must not alias each other or an input'),
    ('nb_eyes_located', 'fresh', (0, 8, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -5, 'nb_eyes_located: no state uploaded'),
    ('nb_eyes_located', 'fresh', (0, 0, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -5, 'nb_eyes_located: no state uploaded'),
    ('nb_eyes_located', 'live', (0, 0, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd', 'e', 'f'), 0, None),
    ('nb_eyes_located', 'live', (8, 0, 'up', 'cp', 64, 1, None, None, None, None, None, 'f'), 0, None),
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp_ortho', 0, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),   # two faults
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp_ortho', 64, 2, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: unknown flag bits'),   # two faults
    ('nb_eyes_located', 'live', (0, 8, 'up', 'cp_ortho', 64, 0, None, None, None, None, None, None), -1, 'nb_eyes_located: cp16 cannot be inverted: cp16[11] must be -1 (a perspective constant as nb_camera_constant forms it)'),   # two faults
    ('nb_eyes_located', 'live', (0, 0, 'up', 'cp_14', 64, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: cp16 cannot be inverted: cp16[14] must not be 0 (a perspective constant as nb_camera_constant forms it)'),   # two faults
    ('nb_eyes_located', 'fresh', (0, 8, 'up', 'cp', 64, 0, None, None, None, None, None, None), -1, 'nb_eyes_located: seen_count, seen_ids, seen_depth, seen_cols, seen_col and seen_rel are all NULL'),   # two faults
    ('nb_eyes_located', 'fresh', (0, 8, 'up', 'cp', 64, 0, 'a', 'b', 'c', 'd', 'f', 'f'), -1, 'nb_eyes_located: the outputs must not alias each other or an input'),   # two faults
    ('nb_eyes_located', 'fresh', (0, 8, 'up', 'cp_0', 64, 0, 'a', 'b', 'c', 'd', 'e', 'f'), -1, 'nb_eyes_located: cp16 cannot be inverted: cp16[0] must not be 0 (a perspective constant as nb_camera_constant forms it)'),   # two faults
    ('nb_step_boids_seen', None, (1, None, 'up', 'cp', 64, 0), -1, 'nb_step_boids_seen: ctx is null'),
    ('nb_step_boids_seen', 'live', (1, None, None, 'cp', 64, 0), -1, 'nb_step_boids_seen: null argument'),
    ('nb_step_boids_seen', 'live', (1, None, 'up', None, 64, 0), -1, 'nb_step_boids_seen: null argument'),
    ('nb_step_boids_seen', 'live', (1, None, 'up', 'cp', 0, 0), -1, 'nb_step_boids_seen: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_step_boids_seen', 'live', (1, None, 'up', 'cp', 4097, 0), -1, 'nb_step_boids_seen: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_step_boids_seen', 'live', (1, 'tile_100', 'up', 'cp', 64, 0), -1, 'nb: boids params.tile must be 0, 256, 512 or 1024'),
    ('nb_step_boids_seen', 'fresh', (1, None, 'up', 'cp', 64, 0), -5, 'nb_step_boids_seen: no state uploaded (call nb_upload first)'),
    ('nb_step_boids_seen', 'live', (0, None, 'up', 'cp', 64, 0), 0, None),
    ('nb_step_boids_seen', 'live', (0, None, 'up', 'cp_ortho', 64, 5), 0, None),   # (a constant the rows take as it is)
    ('nb_step_boids_seen', 'live', (1, 'tile_100', 'up', 'cp', 0, 0), -1, 'nb_step_boids_seen: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),   # two faults
    ('nb_step_boids_seen', 'fresh', (1, None, 'up', 'cp', 0, 0), -1, 'nb_step_boids_seen: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),   # two faults
    ('nb_step_boids_seen', 'fresh', (1, 'tile_100', 'up', 'cp', 64, 0), -5, 'nb_step_boids_seen: no state uploaded (call nb_upload first)'),   # two faults
    ('nb_step_boids_seen', 'fresh', (0, None, 'up', 'cp', 64, 0), -5, 'nb_step_boids_seen: no state uploaded (call nb_upload first)'),   # two faults
    ('nb_step_boids_seen', 'live', (0, 'tile_100', 'up', 'cp', 64, 0), -1, 'nb: boids params.tile must be 0, 256, 512 or 1024'),   # two faults
    ('nb_step_nbody_located', None, (1, 'up', 'cp', 64, 0), -1, 'nb_step_nbody_located: ctx is null'),
    ('nb_step_nbody_located', 'live', (1, None, 'cp', 64, 0), -1, 'nb_step_nbody_located: null argument'),
    ('nb_step_nbody_located', 'live', (1, 'up', None, 64, 0), -1, 'nb_step_nbody_located: null argument'),
    ('nb_step_nbody_located', 'live', (1, 'up', 'cp', 0, 0), -1, 'nb_step_nbody_located: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_step_nbody_located', 'live', (1, 'up', 'cp', 4097, 0), -1, 'nb_step_nbody_located: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),
    ('nb_step_nbody_located', 'live', (1, 'up', 'cp_ortho', 64, 0), -1, 'nb_step_nbody_located: cp16 cannot be inverted: cp16[11] must be -1 (a perspective constant as nb_camera_constant forms it)'),
    ('nb_step_nbody_located', 'live', (1, 'up', 'cp_15', 64, 0), -1, 'nb_step_nbody_located: cp16 cannot be inverted: cp16[15] must be 0 (a perspective constant as nb_camera_constant forms it)'),
    ('nb_step_nbody_located', 'live', (1, 'up', 'cp_0', 64, 0), -1, 'nb_step_nbody_located: cp16 cannot be inverted: cp16[0] must not be 0 (a perspective constant as nb_camera_constant forms it)'),
    ('nb_step_nbody_located', 'live', (1, 'up', 'cp_14', 64, 0), -1, 'nb_step_nbody_located: cp16 cannot be inverted: cp16[14] must not be 0 (a perspective constant as nb_camera_constant forms it)'),
    ('nb_step_nbody_located', 'fresh', (1, 'up', 'cp', 64, 0), -5, 'nb_step_nbody_located: no state uploaded (call nb_upload first)'),
    ('nb_step_nbody_located', 'live', (0, 'up', 'cp', 64, 0), 0, None),
    ('nb_step_nbody_located', 'live', (0, 'up', 'cp', 64, 3), 0, None),
    ('nb_step_nbody_located', 'live', (1, 'up', 'cp_ortho', 0, 0), -1, 'nb_step_nbody_located: width must be 1 .. NB_EYES_MAX_WIDTH (4096)'),   # two faults
    ('nb_step_nbody_located', 'fresh', (1, 'up', 'cp_ortho', 64, 0), -1, 'nb_step_nbody_located: cp16 cannot be inverted: cp16[11] must be -1 (a perspective constant as nb_camera_constant forms it)'),   # two faults
    ('nb_step_nbody_located', 'live', (0, 'up', 'cp_14', 64, 0), -1, 'nb_step_nbody_located: cp16 cannot be inverted: cp16[14] must not be 0 (a perspective constant as nb_camera_constant forms it)'),   # two faults
    ('nb_step_nbody_located', 'fresh', (0, 'up', 'cp', 64, 0), -5, 'nb_step_nbody_located: no state uploaded (call nb_upload first)'),   # two faults
]


def refusal_blocks(nb):
    """name -> a host block that outlives every call (numpy array or ctypes structure)"""
    cp = np.ascontiguousarray(nb.eye_constant(64), F).reshape(16)
    blocks = {"up": UP.copy(), "cp": cp, "tile_100": nb._lib.default_boids_params(tile=100)}
    for name, edits in (("cp_ortho", {11: 0, 15: 1}), ("cp_15", {15: 1}), ("cp_0", {0: 0}), ("cp_14", {14: 0})):
        blocks[name] = cp.copy()
        for i, v in edits.items():
            blocks[name][i] = v
    outs = np.zeros(6 * 0x3000, np.uint8)
    blocks["outs"] = outs
    for k, name in enumerate("abcdef"):
        blocks[name] = outs[k * 0x3000:(k + 1) * 0x3000]
    return blocks


def resolve(blocks, a):
    if not isinstance(a, str):
        return a
    name, _, off = a.partition("+")
    b = blocks[name]
    if isinstance(b, ctypes.Structure):
        return ctypes.byref(b)
    return b.ctypes.data + int(off or 0)


def test_the_table_covers_the_four_entries_and_their_checks():
    assert {r[0] for r in ROWS} == {"nb_eyes_seen", "nb_eyes_located", "nb_step_boids_seen", "nb_step_nbody_located"}
    for entry in {r[0] for r in ROWS}:
        mine = [r for r in ROWS if r[0] == entry]
        assert {r[1] for r in mine} == {None, "live", "fresh"} and {r[3] for r in mine} == {0, -1, -5}, entry


@pytest.mark.parametrize("entry", sorted({r[0] for r in ROWS}))
def test_context_refusals_are_the_recorded_ones(nb, oracle, entry):
    from nenbody_amd import _lib

    lib = _lib.load()
    blocks = refusal_blocks(nb)
    pos, vel = oracle.init_state(8, 1)
    fresh = ctypes.c_void_p()
    _lib.check(lib.nb_create(8, 1, None, ctypes.byref(fresh)))
    try:
        with nb.Scene(pos, vel) as sc:
            for name, which, args, status, message in ROWS:
                if name != entry:
                    continue
                ctx = {None: None, "live": sc._ctx, "fresh": fresh}[which]
                # a message of another entry's, so that "none written" shows: the thread's, or the context's
                assert (lib.nb_init_state(0, 0, None, None) if ctx is None else lib.nb_cameras(ctx, None, None, None)) == _lib.NB_ERR_INVALID
                before = _lib.last_error(ctx)
                assert before and not before.startswith(name)
                got = getattr(lib, name)(ctx, *[resolve(blocks, a) for a in args])
                assert got == status, (name, which, args, _lib.last_error(ctx))
                assert _lib.last_error(ctx) == (before if message is None else message), (name, which, args)
            assert sc.steps_done == 0 and not blocks["outs"].any()       # no row stepped, none wrote an output
    finally:
        lib.nb_destroy(fresh)


# -- 2. every non-empty subset of the row entries' outputs ---------------------------------------------------------------------------------
N2, W2, FIRST2, COUNT2 = 9, 8, 2, 5
WORDS = {"nb_eyes_seen": (COUNT2, COUNT2 * W2, COUNT2 * W2, COUNT2 * W2),
         "nb_eyes_located": (COUNT2, COUNT2 * W2, COUNT2 * W2, COUNT2 * W2, COUNT2 * W2, COUNT2 * W2 * 4)}


def call_with_outputs(sc, entry, flags, wanted):
    """the entry with the outputs of ``wanted`` (a tuple of bools), the others NULL: a list of uint32 arrays (None: not wanted), each
    with its GUARD words, every word SENT before the call"""
    import nenbody_amd as nb
    from nenbody_amd import _lib

    cp = np.ascontiguousarray(nb.eye_constant(W2), F).reshape(16)
    up = UP.copy()
    bufs = [np.full(words + GUARD, SENT, np.uint32) if w else None for words, w in zip(WORDS[entry], wanted)]
    ptrs = [None if b is None else b.ctypes.data for b in bufs]
    _lib.check(getattr(sc._lib, entry)(sc._ctx, FIRST2, COUNT2, up.ctypes.data, cp.ctypes.data, W2, flags, *ptrs), sc._ctx)
    return bufs


@pytest.mark.parametrize("see_self", [False, True])
@pytest.mark.parametrize("entry", ["nb_eyes_seen", "nb_eyes_located"])
def test_every_subset_of_outputs_is_the_full_calls(nb, oracle, entry, see_self):
    from nenbody_amd import _lib

    pos, vel = oracle.init_state(N2, 3)       # (three of the five eyes see somebody at this width)
    flags = _lib.NB_EYES_SEE_SELF if see_self else 0
    k = len(WORDS[entry])
    with nb.Scene(pos, vel) as sc:
        full = call_with_outputs(sc, entry, flags, (True,) * k)
        assert all((b[-GUARD:] == SENT).all() for b in full)
        assert sum(int((b[:-GUARD] != SENT).sum()) for b in full) > sum(WORDS[entry]) // 2       # the call wrote its outputs
        subsets = [w for w in itertools.product((False, True), repeat=k) if any(w)]
        assert len(subsets) == 2 ** k - 1
        # ascending, then descending: a row that one subset leaves out is stale or missing when the next one wants it
        for wanted in subsets + subsets[::-1]:
            got = call_with_outputs(sc, entry, flags, wanted)
            for a, (g, f) in enumerate(zip(got, full)):
                assert (g is not None) == wanted[a]
                if g is None:
                    continue
                # every word the full call's: so the sentinel stands nowhere but where the full result holds that same word
                assert (g[:-GUARD] == f[:-GUARD]).all(), (entry, wanted, a, np.nonzero(g[:-GUARD] != f[:-GUARD])[0][:8])
                assert (g[-GUARD:] == SENT).all(), (entry, wanted, a)
    if entry == "nb_eyes_seen":     # the full call is Scene.seen's, which tests/test_gpu_seen.py holds to the restatement
        assert full[0][:COUNT2].max() > 0


# -- 3. the context's chain against the stateless launches ---------------------------------------------------------------------------------
def test_the_context_chain_is_the_stateless_chain(nb, oracle):
    import torch

    from nenbody_amd import _lib

    n, w, first, count = 65, 65, 5, 57
    lib = _lib.load()
    pos, vel = oracle.init_state(n, 1065)
    cp = np.ascontiguousarray(nb.eye_constant(w), F).reshape(16)
    up = UP.copy()
    dev = torch.device("cuda", 0)
    with nb.Scene(pos, vel) as sc:
        located = sc.located(width=w, first=first, count=count)
        seen = sc.seen(width=w, first=first, count=count)
        sc.sync()
        p, v, _ = sc.device_state(with_instances=False)
        eyes, dirs = p + 16 * first, v + 16 * first
        i32 = lambda *shape: torch.full(shape, SENT, dtype=torch.int32, device=dev)
        inst, cams = i32(n, 16), i32(count, 16)
        ids, depth = i32(count, w), i32(count, w)
        o_count, o_ids, o_depth, o_cols, o_col, o_rel = i32(count), i32(count, w), i32(count, w), i32(count, w), i32(count, w), i32(count, w, 4)
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            _lib.check(lib.nb_launch_instances(n, p, v, inst.data_ptr(), s.cuda_stream))
            _lib.check(lib.nb_launch_cameras(count, eyes, dirs, up.ctypes.data, cp.ctypes.data, cams.data_ptr(), s.cuda_stream))
            _lib.check(lib.nb_launch_eyes(n, first, count, cams.data_ptr(), inst.data_ptr(), w, 0, ids.data_ptr(), depth.data_ptr(), s.cuda_stream))
            _lib.check(lib.nb_launch_seen(count, w, ids.data_ptr(), depth.data_ptr(), o_count.data_ptr(), o_ids.data_ptr(), o_depth.data_ptr(),
                                          o_cols.data_ptr(), s.cuda_stream))
            _lib.check(lib.nb_seen_located_launch(count, w, ids.data_ptr(), depth.data_ptr(), o_count.data_ptr(), o_ids.data_ptr(),
                                                  o_depth.data_ptr(), eyes, dirs, up.ctypes.data, cp.ctypes.data, o_col.data_ptr(),
                                                  o_rel.data_ptr(), s.cuda_stream))
        s.synchronize()
        want = [t.cpu().numpy().view(np.uint32) for t in (o_count, o_ids, o_depth, o_cols, o_col, o_rel)]
    names = ("seen_count", "seen_ids", "seen_depth", "seen_cols", "seen_col", "seen_rel")
    for name, g, x in zip(names, located, want):
        assert bits(g).shape == x.shape and (bits(g) == x).all(), f"nb_eyes_located: {name} differs at {np.argwhere(bits(g) != x)[:4]}"
    for name, g, x in zip(names, seen, want):
        assert bits(g).shape == x.shape and (bits(g) == x).all(), f"nb_eyes_seen: {name} differs at {np.argwhere(bits(g) != x)[:4]}"
    assert (want[0] > 0).mean() > 0.5 and (want[4][:, 0][want[0] > 0] != L.NONE).all()     # eyes that see, members with a column


# -- 4. the context's rows grow and are reused across the entries -----------------------------------------------------------------------------
def test_rows_grow_and_are_reused_across_the_entries(nb, oracle):
    n, w = 257, 65
    pos, vel = oracle.init_state(n, 1257)

    def assert_seen(sc, what, **kw):
        ids, depth = sc.eyes(width=w, **kw)
        got = sc.seen(width=w, **kw)
        TS.assert_lists((got[0], got[1], bits(got[2]), got[3]), S.seen_rows(ids, depth), what)

    with nb.Scene(pos, vel) as sc:
        assert_seen(sc, "seen of one eye", first=0, count=1)
        TS.assert_step(sc, "step_boids_seen, batch 100", width=w, batch=100)
        TL.assert_scene_located(sc, sc.state()[1], "located of 57 eyes", width=w, first=200, count=57)
        TL.assert_step(sc, "step_nbody_located, one batch", width=w, batch=257)
        TL.assert_step(sc, "step_nbody_located, batch 1", width=w, batch=1)
        assert_seen(sc, "seen of the whole set")
        assert sc.steps_done == 3
