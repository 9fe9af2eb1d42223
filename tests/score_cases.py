"""Inputs of the tests of the scene batches' score: tests/test_scenes_score_cpu.py,
tests/test_gpu_scenes_score.py.

TEST INFRASTRUCTURE.  A case is (kind, n): a batch of B = 3 distinct scenes of n bodies drawn from a seed, a goal, and a radius_sq that
is a d2 some pair of the batch attains -- the median of the finite d2 of all its pairs, or an attained d2 next to it that tells a
fused d2 from the rule's (attained_radius) --, so that `near` is neither 0 nor n(n-1)/2
wherever a scene has three pairs to count, and `<` and `<=` differ.  The sizes are every workgroup of the kernel's ladder, both
sides of every step of it, powers of two and their neighbours, and a lane's second body (n > 1 024)."""
import numpy as np

import score_restatement as Q

F32 = np.float32
SCENES = 3
SIZES = (1, 2, 5, 64, 65, 100, 128, 129, 256, 300, 512, 513, 1024, 1025, 1537, 2048)
KINDS = ("planar", "random", "clustered", "large", "tiny", "lattice", "nonfinite")
CASES = [(kind, n) for kind in KINDS for n in SIZES]
SCALE = {"large": 1e5, "tiny": 1e-20}
GOAL = F32([0.25, -0.5, 0.125])
OFFSET = np.array([0.5, -0.25, 0.75])

_made = {}


def outliers(n):
    """where the nonfinite kind puts its components: the first lane of the first and of the last wave that holds a body, the last lane
    of a wave and the last body, and a lane's second body where there is one"""
    first = sorted({0, 64 * ((n - 1) // 64)})
    last = sorted({min(63, n - 1), n - 1})
    second = sorted({1024, n - 1}) if n > 1024 else []
    return first, last, second


def attained_radius(pos, fused):
    """the median of the finite d2 of all pairs of the batch -- or, where `fused` asks for it, the attained d2 nearest to the median in
    rank that a fused multiply-add would round below its value AND for which the batch's count of fused d2 below it differs from the
    rule's: a contracted d2 then moves `near`, whatever else it leaves alone"""
    n = pos.shape[1]
    upper = np.triu_indices(n, 1)
    d2 = np.concatenate([Q.pair_d2(p)[upper] for p in pos])
    ok = np.isfinite(d2)
    if not ok.any():
        return F32(1)
    order = np.argsort(d2[ok], kind="stable")
    ds = d2[ok][order]
    mid = len(ds) // 2
    if fused:
        fs = np.concatenate([Q.pair_d2(p, "fma")[upper] for p in pos])[ok][order]
        below = np.nonzero(fs < ds)[0]
        for at in below[np.argsort(np.abs(below - mid), kind="stable")][:64]:
            if int((fs < ds[at]).sum()) != int((ds < ds[at]).sum()):
                return F32(ds[at])
        raise AssertionError("no attained d2 tells a fused d2 from the rule's")
    return F32(ds[mid])


def make(kind, n):
    """(positions (B, n, 3), velocities (B, n, 3), radius_sq, goal) of a case; the same arrays every time"""
    if (kind, n) in _made:
        return _made[kind, n]
    rng = np.random.default_rng([1405, KINDS.index(kind), n])
    if kind == "lattice":                                      # small integers: every sum exact, many pairs at every attained d2
        pos = rng.integers(-6, 7, (SCENES, n, 3)).astype(F32)
        vel = rng.integers(-3, 4, (SCENES, n, 3)).astype(F32)
        goal = F32([1, -2, 3])
    else:
        pos = rng.uniform(-1, 1, (SCENES, n, 3))
        vel = rng.uniform(-1, 1, (SCENES, n, 3))
        if kind == "clustered":                                # one clump a scene, 2^-12 wide: a body's distance from the centroid is
            pos *= 2.0 ** -13                                  # some thousand ulps of the centroid, whose last bit moves every square
        if kind == "planar":
            pos[..., 2] = 0.0
            vel[..., 2] = 0.0
        pos += OFFSET * (1, 1, kind != "planar")                # a centroid of the size of the coordinates: its last bit moves a square
        scale = SCALE.get(kind, 1.0)
        pos, vel = (pos * scale).astype(F32), (vel * scale).astype(F32)
        goal = (GOAL * F32(scale)).astype(F32)
    if kind == "nonfinite":
        first, last, second = outliers(n)
        for i in first:
            pos[0, i, 0] = np.inf                              # scene 0: positions only, so speed2 and momentum2 stay finite
            vel[1, i, 1] = np.nan                              # scene 1: velocities only, so near, spread and goal2 stay finite
        for i in last:
            pos[0, i, 1] = np.nan
            vel[1, i, 2] = -np.inf
        for i in second + first[:1]:                           # scene 2: both records of one body, which counts once
            pos[2, i, 2] = -np.inf
            vel[2, i, 0] = np.nan
    radius_sq = attained_radius(pos, kind not in ("lattice", "tiny") and n >= 64)   # (thirty pairs need not hold such a d2)
    for a in (pos, vel):
        a.setflags(write=False)
    _made[kind, n] = (pos, vel, radius_sq, goal)
    return _made[kind, n]


_want = {}


def want(kind, n):
    """the records of the case after one snapshot from cleared records, by the restatement; computed once"""
    if (kind, n) not in _want:
        pos, vel, radius_sq, goal = make(kind, n)
        _want[kind, n] = Q.batch(pos, vel, radius_sq, goal)
        _want[kind, n].setflags(write=False)
    return _want[kind, n]


# the three bodies of the hand case (tests/test_scenes_score_cpu.py derives its record in exact rationals)
HAND_POS = F32([[0.1, 0.2, 0.3], [1.7, -0.4, 0.9], [-0.6, 1.1, 0.05]])
HAND_VEL = F32([[0.3, -0.7, 0.2], [-0.9, 0.1, 0.6], [0.45, 0.8, -1.3]])
HAND_GOAL = F32([0.7, -0.2, 1.3])
HAND_RADIUS_SQ = F32(3.5)
