"""CPU tests of every entity's eye view (nb_eyes / nb_launch_eyes): the numpy restatement of the rule
(tests/eyes_restatement.py) on hand-checked scenes, and the new entry points' argument checks, which run before any device work."""
import ctypes

import numpy as np
import pytest

import eyes_restatement as R

F = np.float32
UP = np.array([0, 0, 1], np.float32)


def view(oracle, pos, vel, width=1024, cp=None, first=0, count=None, see_self=False):
    """the rule for eyes [first, first + count) of (pos, vel), cameras and model matrices by the oracle"""
    pos, vel = np.asarray(pos, np.float32), np.asarray(vel, np.float32)
    count = len(pos) - first if count is None else count
    cp = R.eye_constant(oracle, width) if cp is None else cp
    cams = oracle.cameras(pos[first:first + count], vel[first:first + count], UP, cp)
    return R.eyes(cams, oracle.instances(pos, vel), first, width, see_self)


def covered(ids_row):
    return np.nonzero(ids_row != R.NONE)[0]


def test_hand_check_one_body_straight_ahead(oracle):
    """eye at the origin heading +x, one body at (10, 0, 0) heading +x: its rear edge at view distance 9 spans
    x/w = +-(f / 1024) / 9 with f = 1 / tan(90 / 2048 degrees), columns 440 .. 583; the depth is that edge's, 10000/9999 * 8/9"""
    ids, depth = view(oracle, [[0, 0, 0], [10, 0, 0]], [[1, 0, 0], [1, 0, 0]])
    c = covered(ids[0])
    assert (c == np.arange(440, 584)).all() and len(c) == 144
    assert (ids[0, c] == 1).all()
    want = 10000.0 / 9999.0 * 8.0 / 9.0
    assert np.abs(depth[0, c].astype(np.float64) - want).max() <= 2 * np.spacing(F(want))
    rest = np.setdiff1d(np.arange(1024), c)
    assert (ids[0, rest] == R.NONE).all() and (depth[0, rest] == 1).all()
    # body 1's own eye looks away from body 0, and does not see itself
    assert (ids[1] == R.NONE).all()


def test_a_body_behind_the_eye_is_not_seen(oracle):
    ids, depth = view(oracle, [[0, 0, 0], [-10, 0, 0]], [[1, 0, 0], [1, 0, 0]], count=1)
    assert (ids == R.NONE).all() and (depth == 1).all()


def test_the_far_plane_clips(oracle):
    """far = 50: a body at x = 60 lies wholly beyond it; one at x = 49.5 has its rear edge (48.5) inside and its two side edges cut
    at 50 (their far ends land on depth 1 within rounding), and still covers 26 columns"""
    cp = R.eye_constant(oracle, far=50.0)
    ids, _ = view(oracle, [[0, 0, 0], [60, 0, 0]], [[1, 0, 0], [1, 0, 0]], cp=cp, count=1)
    assert (ids == R.NONE).all()
    pos, vel = np.array([[0, 0, 0], [49.5, 0, 0]], F), np.array([[1, 0, 0], [1, 0, 0]], F)
    ids, depth = view(oracle, pos, vel, cp=cp, count=1)
    c = covered(ids[0])
    assert len(c) == 26 and (c == np.arange(499, 525)).all() and (ids[0, c] == 1).all() and (depth[0, c] < 1).all()
    cams = oracle.cameras(pos[:1], vel[:1], UP, cp)
    keep, xs0, d0, xs1, d1 = R.segments(cams, R.world_vertices(oracle.instances(pos, vel)), 1024)
    assert keep[0, 1].all()
    assert abs(float(d1[0, 1, 0]) - 1) < 1e-5 and abs(float(d0[0, 1, 1]) - 1) < 1e-5   # a0 -> a1 ends, a1 -> a2 starts on the far plane
    _, _, _, _, d1_unclipped = R.segments(oracle.cameras(pos[:1], vel[:1], UP, R.eye_constant(oracle)),
                                          R.world_vertices(oracle.instances(pos, vel)), 1024)
    assert float(d1_unclipped[0, 1, 0]) < 0.99999


def test_a_nearer_body_occludes_a_farther_one(oracle):
    """bodies at 20 and 10 ahead: the nearer one (the HIGHER index here) is seen on every column it shares with the farther one"""
    for near, far in ((2, 1), (1, 2)):
        pos = np.zeros((3, 3), F)
        pos[near, 0], pos[far, 0] = 10, 20
        ids, _ = view(oracle, pos, np.tile(F([1, 0, 0]), (3, 1)), count=1)
        c = covered(ids[0])
        assert len(c) == 144 and (ids[0, c] == near).all()


def test_coincident_bodies_tie_to_the_lower_index(oracle):
    pos = np.array([[0, 0, 0], [10, 0, 0], [10, 0, 0]], F)
    ids, depth = view(oracle, pos, np.tile(F([1, 0, 0]), (3, 1)), count=1)
    c = covered(ids[0])
    assert len(c) == 144 and (ids[0, c] == 1).all()
    _, alone = view(oracle, pos[:2], np.tile(F([1, 0, 0]), (2, 1)), count=1)
    assert (depth.view(np.uint32) == alone.view(np.uint32)).all()


def test_a_zero_velocity_eye_sees_nothing(oracle):
    """look_at_dir normalises the velocity: a zero one gives a NaN camera, and a NaN covers nothing"""
    pos = np.array([[0, 0, 0], [10, 0, 0]], F)
    vel = np.array([[0, 0, 0], [1, 0, 0]], F)
    cams = oracle.cameras(pos[:1], vel[:1], UP, R.eye_constant(oracle))
    assert np.isnan(cams).any()
    ids, depth = view(oracle, pos, vel, count=1)
    assert (ids == R.NONE).all() and (depth == 1).all()


def test_the_eye_skips_its_own_body_unless_asked(oracle):
    """the eye's own triangle straddles its near plane; with near = 0.5 its side edges reach in front of it.  Without
    NB_EYES_SEE_SELF it is skipped (the controllers' n != i); with it, it goes through the rule like any other body"""
    cp = R.eye_constant(oracle, near=0.5)
    ids, _ = view(oracle, [[0, 0, 0]], [[1, 0, 0]], cp=cp)
    assert (ids == R.NONE).all()
    ids, depth = view(oracle, [[0, 0, 0]], [[1, 0, 0]], cp=cp, see_self=True)
    c = covered(ids[0])
    assert len(c) > 100 and (ids[0, c] == 0).all() and (depth[0, c] < 1).all()
    # the reference's constant (near = 1): the triangle only touches the near plane at its tip, a zero-length span
    ids, _ = view(oracle, [[0, 0, 0]], [[1, 0, 0]], see_self=True)
    assert (ids == R.NONE).all()


def test_a_row_of_one_pixel(oracle):
    """W = 1: the constant is perspective(90 degrees, 1, ...), the one column centre 0.5 lies inside the rear edge's span"""
    ids, depth = view(oracle, [[0, 0, 0], [10, 0, 0]], [[1, 0, 0], [1, 0, 0]], width=1, count=1)
    assert ids.shape == (1, 1) and ids[0, 0] == 1
    want = 10000.0 / 9999.0 * 8.0 / 9.0
    assert abs(float(depth[0, 0]) - want) <= 2 * np.spacing(F(want))


def test_exact_lattice(oracle):
    """R.lattice_expectation: edge ends exactly on column centres, vertices exactly on B3 / B4 = 0, one edge cut by B4"""
    cams = np.repeat(R.lattice_camera()[None], 4, 0)
    ids, depth = R.eyes(cams, oracle.instances(R.LATTICE_POS, R.LATTICE_VEL), 0, 1024, see_self=True)
    want_ids, want_depth = R.lattice_expectation()
    for e in range(4):
        assert (ids[e] == want_ids).all(), np.nonzero(ids[e] != want_ids)
        assert (depth[e].view(np.uint32) == want_depth.view(np.uint32)).all()


def test_eye_constant_is_the_references(oracle):
    import nenbody_amd as nb

    for w in (1, 3, 1024, 4096):
        assert (nb.eye_constant(w).view(np.uint32) == R.eye_constant(oracle, w).view(np.uint32)).all()
        assert (nb.eye_constant(w) == nb.camera_constant(90.0 / w, float(w), 1.0, 10000.0)).all()


def test_eye_entry_points_validate_before_touching_the_device(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    up, cp = np.array([0, 0, 1], F), np.zeros(16, F)
    ids, depth = np.zeros((2, 8), np.uint32), np.zeros((2, 8), F)
    assert lib.nb_eyes(None, 0, 1, up.ctypes.data, cp.ctypes.data, 8, 0, ids.ctypes.data, depth.ctypes.data) == _lib.NB_ERR_INVALID
    assert "ctx is null" in _lib.last_error()
    fn = lib.nb_launch_eyes
    cams, inst, a, b = 0x100000, 0x200000, 0x300000, 0x400000      # 16-byte aligned, never dereferenced: the checks come first

    def rc(n=4, first=0, count=2, cams=cams, inst=inst, width=8, flags=0, ids=a, depth=b):
        return fn(n, first, count, cams, inst, width, flags, ids, depth, None)

    cases = {
        "width 0": dict(width=0), "width above the maximum": dict(width=_lib.NB_EYES_MAX_WIDTH + 1),
        "range past n": dict(first=3), "count past n": dict(count=5), "unknown flag": dict(flags=2), "flag bit 31": dict(flags=1 << 31),
        "no output": dict(ids=None, depth=None), "outputs alias": dict(depth=a), "outputs overlap": dict(depth=a + 60),
        "ids over cams": dict(ids=cams + 16), "depth over inst": dict(depth=inst + 200), "ids over inst end": dict(ids=inst + 4 * 64 - 4),
        "null cams": dict(cams=None), "null inst": dict(inst=None), "misaligned cams": dict(cams=cams + 4),
        "misaligned inst": dict(inst=inst + 8),
    }
    for what, kw in cases.items():
        assert rc(**kw) == _lib.NB_ERR_INVALID, what
    assert "alias" in (rc(depth=a) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "width" in (rc(width=0) == _lib.NB_ERR_INVALID and _lib.last_error())
    # right up against each other is not an overlap; count = 0 is a no-op (no device needed); one output alone is enough
    assert rc(count=0) == _lib.NB_OK and rc(count=0, first=4) == _lib.NB_OK
    if lib.nb_device_count() == 0:
        for kw in (dict(), dict(depth=a + 2 * 8 * 4), dict(ids=None), dict(depth=None), dict(flags=_lib.NB_EYES_SEE_SELF),
                   dict(width=_lib.NB_EYES_MAX_WIDTH), dict(width=1), dict(first=2)):
            assert rc(**kw) == _lib.NB_ERR_NO_DEVICE, kw
        with pytest.raises(nb.NbError):
            nb.Scene.new(4)
