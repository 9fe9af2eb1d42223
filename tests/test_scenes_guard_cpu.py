"""What tests/test_gpu_scenes_guard.py rests on, checked without a GPU on the very arrays of tests/scenes_guard_cases.py: the corner
scenes lie inside their range, reach the extremes family A claims, and leave the range with step one; the reference is finite on
every corner, outlier and velocity scene after every step the GPU file compares, so that it may compare bits plainly and a NaN there
is the device's own; and the places and the grid are the ones the kernel's flag logic calls for."""
import numpy as np
import pytest

import guard_corners as gc
import scenes_guard_cases as K

F = np.float32


def in_range(pos, a, b):
    mag = np.abs(pos)
    return (mag == 0) | ((mag >= F(2.0 ** a)) & (mag <= F(2.0 ** b)))


def corner_scene_premises(oracle, case, pos, vel):
    """the premises of one corner scene, each asserted; `pos`, `vel`: (n, 3)"""
    G, bias = case
    a, b = gc.guard(G, bias)[:2]
    assert in_range(pos, a, b).all(), "a coordinate outside the range"
    origin = (pos == 0).all(axis=1)
    assert origin.any() and ((pos[:, 2] == 0) & (pos[:, 0] != 0)).any(), "no body at the origin or none with z = 0 only"
    assert len(np.unique(pos, axis=0)) < len(pos) - origin.sum(), "no coincident bodies besides those at the origin"
    assert gc.coverage(pos, G, bias) == gc.expected_coverage(G, bias), "the extremes are not reached"
    consts = K.corner_constants(case)
    p1, v1 = oracle.run(pos, vel, 1, **consts)
    assert np.isfinite(p1).all() and np.isfinite(v1).all(), "the reference is not finite after one step"
    assert (~in_range(p1, a, b)).any(), "every body is still in range after step one"
    if 2 in K.corner_steps(case):
        p2, v2 = oracle.run(pos, vel, 2, **consts)
        assert np.isfinite(p2).all() and np.isfinite(v2).all(), "the reference is not finite after two steps"


@pytest.mark.parametrize("case", gc.CORNER_CONSTANTS, ids=gc.corner_id)
def test_every_corner_scene_holds_its_premises(oracle, case):
    shapes = [n for c, n in K.corner_grid() if c == case]
    assert shapes
    for n in shapes:
        pos, vel = K.corner_batch(case, n)
        assert pos.shape == vel.shape == (K.CORNER_SCENES, n, 3) and pos.dtype == vel.dtype == F
        for s in range(K.CORNER_SCENES):
            corner_scene_premises(oracle, case, pos[s], vel[s])


def test_the_premises_fail_below_64_bodies(oracle):
    """the check above can fail: under the first constants, seed 11 at n = 33 (and seeds 1, 3, 6 and 11 at n = 16) keeps every body
    in range after step one, so the second step would hand nothing over -- why SHAPES starts at 64"""
    case = gc.CORNER_CONSTANTS[0]
    a, b = gc.guard(*case)[:2]
    for n, seed in ((33, 11), (16, 1)):
        with pytest.raises(AssertionError, match="still in range after step one"):
            corner_scene_premises(oracle, case, *gc.corner_state(n, a, b, seed))
    corner_scene_premises(oracle, case, *gc.corner_state(64, a, b, 11))


def test_the_corner_grid_meets_the_thinning_rule():
    grid = K.corner_grid()
    assert len(set(grid)) == len(grid) and {n for _, n in grid} == set(K.SHAPES) and {c for c, _ in grid} == set(gc.CORNER_CONSTANTS)
    for case in gc.CORNER_CONSTANTS:
        assert {n for c, n in grid if c == case} >= set(K.MUST_MEET_SHAPES), case
    for n in K.SHAPES:
        met = {c for c, m in grid if m == n}
        assert len(met) >= 3 and met >= set(K.MUST_MEET_CONSTANTS), n
    assert K.MUST_MEET_SHAPES == (64, 1024, 1537, 2048) and K.MUST_MEET_CONSTANTS == ((0.3, 2.0 ** -100), (2.0 ** 100, 4.0))
    assert all(c in gc.CORNER_CONSTANTS for c in K.MUST_MEET_CONSTANTS)
    assert [K.corner_steps(c) for c in gc.CORNER_CONSTANTS] == [(1, 2)] * 9 + [(1,)]
    assert K.corner_seeds(gc.CORNER_CONSTANTS[4]) == [40, 41, 42]


def test_shapes_and_places():
    assert K.SHAPES == [64, 100, 128, 256, 300, 512, 1024, 1537, 2048]
    assert [K.lanes(n) for n in K.SHAPES] == [64, 128, 128, 256, 512, 512, 1024, 1024, 1024]
    assert [len(K.places(n)) for n in K.SHAPES] == [2, 4, 4, 8, 10, 16, 32, 49, 64]
    assert K.places(100) == [0, 63, 64, 99] and K.places(300) == [0, 63, 64, 127, 128, 191, 192, 255, 256, 299]
    assert K.places(1537)[-3:] == [1024 + 448, 1024 + 448 + 63, 1536] and 1024 + 512 + 63 not in K.places(1537)
    for n in K.SHAPES:
        pl = K.places(n)
        assert pl[0] == 0 and pl[-1] == n - 1 and all(p % 64 in (0, 63) or p == n - 1 for p in pl)
        assert (n > 1024) == any(p >= 1024 for p in pl)
    assert {K.place_value(s) for s in range(9)} == {(v, c) for v in gc.OUTLIER_VALUES for c in range(3)}


def assert_place_batch(oracle, n, pos, vel, where, into, steps):
    """one scene per place, one replaced coordinate per scene, clean scenes around; the reference finite after every step and the
    outlier body's velocity the one it started with"""
    pl = K.places(n)
    assert len(pos) == len(pl) + 2 and [(s, body) for s, body, _, _ in where] == [(i + 1, p) for i, p in enumerate(pl)]
    big = np.abs(np.stack([pos, vel])) >= F(2.0 ** 64)
    assert not big[1 - into].any() and (big[into].reshape(len(pos), -1).sum(1) == [0] + [1] * len(pl) + [0]).all()
    for scene, body, value, component in where:
        assert (pos, vel)[into][scene, body, component] == F(value) and abs(value) >= 2.0 ** 64
        for k in range(1, steps + 1):
            p, v = oracle.run(pos[scene], vel[scene], k)
            assert np.isfinite(p).all() and np.isfinite(v).all(), (n, scene, body, k)
            # a position outlier: every term of its sum is +/-0; a velocity outlier: what step 1 adds to 2^64 is far below its last bit
            kept = slice(None) if into == 0 else component
            assert (v[body, kept].view(np.uint32) == vel[scene, body, kept].view(np.uint32)).all(), (n, scene, body, k)
        if into == 1:                                              # in range at launch, outside from step 1 on
            a, b = gc.guard(float(oracle.G), float(oracle.BIAS))[:2]
            assert in_range(pos[scene], a, b).all()
            assert abs(oracle.run(pos[scene], vel[scene], 1)[0][body, component]) >= F(2.0 ** 64)
    for scene in (0, len(pos) - 1):
        p, v = oracle.run(pos[scene], vel[scene], steps)
        assert np.isfinite(p).all() and np.isfinite(v).all()


@pytest.mark.parametrize("n", K.SHAPES)
def test_every_outlier_scene_has_a_finite_reference_and_a_still_outlier(oracle, n):
    assert_place_batch(oracle, n, *K.outlier_batch(oracle, n), into=0, steps=K.OUTLIER_STEPS)


@pytest.mark.parametrize("n", K.SHAPES)
def test_every_velocity_scene_is_in_range_at_launch_and_has_a_finite_reference(oracle, n):
    assert_place_batch(oracle, n, *K.velocity_batch(oracle, n), into=1, steps=K.VELOCITY_STEPS)


def test_the_grid_stride_batch_orders_clean_and_outlier_scenes_every_way(oracle):
    pos, vel, where = K.grid_stride_batch(oracle)
    assert pos.shape == (K.GRID_CAP + 40, 5, 3) and K.GRID_CAP == 2048
    marked = sorted(s for s, _, _, _ in where)
    assert marked == sorted(K.GRID_OUTLIERS) and set(marked) >= {3, 2047, 2048 + 3, len(pos) - 1}
    assert (np.nonzero((np.abs(pos) >= F(2.0 ** 64)).any(axis=(1, 2)))[0] == marked).all()
    # the scenes of one workgroup are s, s + GRID_CAP: outlier after clean, clean after outlier, outlier after outlier
    pairs = {(s in marked, s + K.GRID_CAP in marked) for s in range(len(pos) - K.GRID_CAP)}
    assert pairs == {(False, False), (False, True), (True, False), (True, True)}
    for scene, body, _, _ in where:
        for k in range(1, K.GRID_STEPS + 1):
            p, v = oracle.run(pos[scene], vel[scene], k)
            assert np.isfinite(p).all() and np.isfinite(v).all()
            assert (v[body].view(np.uint32) == vel[scene, body].view(np.uint32)).all()
