"""STRICT's divide guard on scene batches: the data of tests/test_gpu_scenes_guard.py, built on guard_corners.py (no test in here).

TEST INFRASTRUCTURE.  scenes_nbody_kernel (nb_scenes.inc) is a launch shape of STRICT with flag logic of its own: every lane flags the
record it writes, one LDS word per wave and per buffer holds the wave's OR, the words are written again every step, a lane of a scene
above 1 024 bodies owns a second body, and a workgroup reuses the words from scene to scene in its grid-stride loop.  Four families:

  * corner batches: three scenes of guard_corners.corner_state (family A there) per pair of constants and shape, everything inside
    {0} U [2^a, 2^b] at launch; one step is all ladder, the second hands over to '/'.  The grid is the FULL one, every one of
    gc.CORNER_CONSTANTS at every one of SHAPES (corner_grid()); should it ever be thinned, the rule tests/test_scenes_guard_cpu.py
    asserts is: every constant meets 64, 1024, 1537 and 2048, and every shape meets at least three constants, among them
    (0.3, 2^-100) and (2^100, 4.0).
  * outlier batches: per shape ONE batch with one scene per place of places(n), the scene's one outlier (>= 2^64: the ladder gives
    NaN, '/' gives 0) sitting at that place, between a clean scene in front and a clean scene behind;
  * velocity batches: the same layout with the outlier in the VELOCITY, so that every position is in range at launch and the flag
    arises in the record step 1 writes: only the words written per step catch it;
  * the grid-stride batch: more scenes of five bodies than workgroups, a few of them with an outlier, so that one workgroup steps an
    outlier scene after a clean one, an outlier scene after an outlier scene and a clean one after an outlier scene.

tests/test_scenes_guard_cpu.py asserts on these very arrays what the GPU file takes for granted."""
import numpy as np

import guard_corners as gc

F = np.float32
SHAPES = [64, 100, 128, 256, 300, 512, 1024, 1537, 2048]   # every workgroup size, a ragged scene in the larger ones, both two-bodies-per-lane cases
GRID_CAP = 2048                                            # nb_scenes.h: kScenesMaxGrid
CORNER_SCENES = 3
MUST_MEET_SHAPES = (64, 1024, 1537, 2048)                  # the thinning rule: every constant meets these ...
MUST_MEET_CONSTANTS = ((0.3, 2.0 ** -100), (2.0 ** 100, 4.0))   # ... and every shape these, among at least three


def lanes(n):
    """the workgroup a scene of n bodies takes (nb_scenes.inc:scenes_by_size)"""
    return next(w for w in (64, 128, 256, 512, 1024) if n <= w or w == 1024)


def places(n):
    """the bodies where THIS kernel can forget a flag: the scene's first and last body and, for every wave of the workgroup, the wave's
    first and last lane -- as the lane's first body and, above 1 024 bodies, as its second"""
    out = {0, n - 1}
    for w in range(lanes(n) // 64):
        out |= {64 * w, 64 * w + 63}
        if n > 1024:
            out |= {1024 + 64 * w, 1024 + 64 * w + 63}
    return sorted(p for p in out if p < n)


# ---- corner batches -------------------------------------------------------------------------------------------------------------------
def corner_grid():
    """(case, n) of every corner batch: the full grid"""
    return [(case, n) for case in gc.CORNER_CONSTANTS for n in SHAPES]


def corner_id(item):
    return f"{gc.corner_id(item[0])}_n{item[1]}"


def corner_seeds(case):
    return [10 * gc.CORNER_CONSTANTS.index(case) + s for s in range(CORNER_SCENES)]


def corner_steps(case):
    """the step counts a corner batch is compared after (the tenth constant's second step is NaN in the reference itself: guard_corners.py)"""
    return (1, 2) if case in gc.CORNER_TWO_STEPS else (1,)


def corner_constants(case):
    """oracle.run's keywords"""
    return dict(dt=F(gc.CORNER_DT), g=F(case[0]), bias=F(case[1]))


def corner_params(nb, case):
    p = nb.default_params()
    p.dt, p.G, p.bias = float(gc.CORNER_DT), float(case[0]), float(case[1])
    return p


def corner_batch(case, n):
    """(pos, vel), (3, n, 3) each: gc.corner_state for the case's range and three seeds"""
    a, b = gc.guard(*case)[:2]
    out = [gc.corner_state(n, a, b, seed) for seed in corner_seeds(case)]
    return np.stack([p for p, _ in out]), np.stack([v for _, v in out])


# ---- outlier and velocity batches -----------------------------------------------------------------------------------------------------
OUTLIER_STEPS = 2
VELOCITY_STEPS = 3


def place_value(s):
    """(value, component) of the s-th place: the value rotates through gc.OUTLIER_VALUES, the component through x, y, z one place later
    every three, so that nine places meet all nine pairs"""
    return gc.OUTLIER_VALUES[s % 3], (s + s // 3) % 3


def _place_batch(oracle, n, seed, into):
    pl = places(n)
    out = [oracle.init_state(n, seed + s) for s in range(len(pl) + 2)]
    pos, vel = np.stack([p for p, _ in out]).astype(F), np.stack([v for _, v in out]).astype(F)
    where = []
    for s, body in enumerate(pl):
        value, component = place_value(s)
        (pos, vel)[into][s + 1, body, component] = F(value)
        where.append((s + 1, body, value, component))
    return pos, vel, where


def outlier_batch(oracle, n):
    """(pos, vel, where): len(places(n)) + 2 scenes, scene s the reference's initial state for seed 500 + n + s; `where` lists
    (scene, body, value, component) of the one replaced POSITION coordinate of scenes 1 .. len(places(n)); the first and the last scene
    are clean"""
    return _place_batch(oracle, n, 500 + n, 0)


def velocity_batch(oracle, n):
    """the same with the VELOCITY coordinate replaced (seed 700 + n + s): every position is in range at launch"""
    return _place_batch(oracle, n, 700 + n, 1)


# ---- the grid-stride batch ------------------------------------------------------------------------------------------------------------
GRID_N = 5
GRID_SCENES = GRID_CAP + 40
GRID_STEPS = 2
# workgroup 39 steps scene 39 (clean), then the last scene (outlier); workgroup 3 scene 3, then 2048 + 3 (outlier after outlier);
# workgroup 2047 one outlier scene alone; workgroup 5 scene 5 (outlier), then 2048 + 5 (clean)
GRID_OUTLIERS = [3, 5, GRID_CAP - 1, GRID_CAP + 3, GRID_SCENES - 1]


def grid_stride_batch(oracle):
    """(pos, vel, where): GRID_SCENES scenes of five bodies, every one clean but GRID_OUTLIERS"""
    out = [oracle.init_state(GRID_N, 9100 + s) for s in range(GRID_SCENES)]
    pos, vel = np.stack([p for p, _ in out]).astype(F), np.stack([v for _, v in out]).astype(F)
    where = []
    for i, scene in enumerate(GRID_OUTLIERS):
        value, component = place_value(i)
        pos[scene, i % GRID_N, component] = F(value)
        where.append((scene, i % GRID_N, value, component))
    return pos, vel, where
