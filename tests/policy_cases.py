"""Inputs of the tests of the scene batches' neural policy: tests/test_scenes_policy_cpu.py,
tests/test_gpu_scenes_policy.py.

TEST INFRASTRUCTURE.  A batch is drawn by scenes_seen_cases.batch from a row (seed, n, width, scale, scenes): scene s is the
reference's initial state of n bodies for seed + s, its positions multiplied by `scale`; narrow rows look at a scene drawn together,
as the seen and located cases do.  The policies of a case are drawn by policies() at scales where a blind eye's first hidden unit is
off and a seeing eye's is on, and where a seeing eye's outputs pass the limit and a blind eye's do not; the CPU file asserts both on
every case that has both kinds of eye."""
import numpy as np

import policy_restatement as P
from scenes_seen_cases import UP, batch  # noqa: F401  (the tests' K.*)

F32 = np.float32
SCENES = 3
LIMIT = F32(0.5)
SIZES = (5, 128, 129, 300)             # both lane shapes, both sides of the line at 128 bodies
WIDTHS = (8, 64, 1024)
HIDDEN = (1, 7, 64)
SCALE = {8: 0.1, 64: 0.1, 1024: 1.0}   # positions drawn together for narrow rows


def feature_counts(width):
    """F in {1, 8, W}, where the shape is one (F <= NB_POLICY_MAX_FEATURES)"""
    return sorted({f for f in (1, 8, width) if f <= P.MAX_FEATURES})


def limit(n, width):
    """the limit of a case: the scenes of 128 bodies and more drawn together for a narrow row put somebody near in every bin of nearly
    every eye (x about 1), so that LIMIT would clip every seeing eye; twice LIMIT clips about half of them"""
    return F32(1.0) if n >= 128 and width <= 64 else LIMIT


def row(n, width):
    return (1100, n, width, 0.05 if n == 5 else SCALE[width], SCENES)


# (n, width, F, H): 84 cases
CASES = [(n, w, f, h) for n in SIZES for w in WIDTHS for f in feature_counts(w) for h in HIDDEN]


def policies(features, hidden, count, seed=7):
    """(count, policy_floats) float32.  Unit 0 of every policy: b1 = -2^-7 and w1 in [0.5, 1.5) / F, so it is off for an eye that
    sees nothing, on for one that sees something near, and about the mean of x_f; its w2 has magnitude in [1, 2), so an eye with
    somebody near in most bins passes LIMIT and one that sees little does not.  The other units: w1 in [-1, 1) / F,
    b1 in [-0.02, 0.02), w2 in [-2, 2) / H; b2 in [-0.01, 0.01), inside the limit."""
    rng = np.random.default_rng([seed, features, hidden])
    out = []
    for _ in range(count):
        w1 = (rng.uniform(-1, 1, (features, hidden)) / features).astype(F32)
        w1[:, 0] = (rng.uniform(0.5, 1.5, features) / features).astype(F32)
        b1 = rng.uniform(-0.02, 0.02, hidden).astype(F32)
        b1[0] = F32(-2.0 ** -7)
        w2 = (rng.uniform(-2, 2, (2, hidden)) / hidden).astype(F32)
        w2[:, 0] = (rng.uniform(1, 2, 2) * rng.choice([-1, 1], 2)).astype(F32)
        b2 = rng.uniform(-0.01, 0.01, 2).astype(F32)
        out.append(P.pack(w1, b1, w2, b2))
    return np.stack(out)


# DESIGN.md sections 12 and 13's two bodies under a policy of one hidden unit that reads bins 3 and 4 of 8
HAND_POS = np.array([[0, 0, 0], [10, 0, 0]], F32)
HAND_VEL = np.array([[1, 0, 0], [1, 0, 0]], F32)
HAND_SHAPE = (1024, 8, 1)              # W, F, H
HAND_DEPTH_BITS = 0x3F63940C           # what eye 0 sees over columns 440 .. 583


def hand_policy():
    w1 = np.zeros((8, 1), F32)
    w1[3] = w1[4] = 1
    return P.pack(w1, np.zeros(1, F32), np.array([[1], [0.5]], F32), np.zeros(2, F32))


def special_scene():
    """One scene of 6 bodies close together along x: body 1 has zero velocity, body 2 moves along `up`, body 3's velocity is not
    finite; the others head +x or -x and see somebody.  (positions, velocities) (1, 6, 3)"""
    pos = np.array([[0, 0, 0], [4, 0.5, 0], [8, -0.5, 0], [12, 0.25, 0], [16, 0, 0], [20, 0.1, 0]], F32)
    vel = np.array([[1, 0, 0], [0, 0, 0], [0, 0, 2], [np.inf, 0, 0], [-1, 0, 0], [-1, 0.01, 0]], F32)
    return pos[None], vel[None]
