"""Inputs of the tests of the scene batches' seen boids step: tests/test_scenes_seen_cpu.py,
tests/test_gpu_scenes_seen.py.

TEST INFRASTRUCTURE.  Every batch the GPU file steps is drawn here from a row (seed, n, width, scale, scenes): scene s is the
reference's initial state of n bodies for seed + s -- what SceneBatch.new draws --, its positions multiplied by `scale`.  The CPU
file checks on these very rows that the GPU tests can tell something: each scene has a blind body, most bodies see somebody, and
the seen step differs from the plain one.  Rows of fewer than PREMISE_MIN_N bodies or narrower than PREMISE_MIN_WIDTH columns
cannot hold those premises (a scene of one body sees nobody; one column holds one id) and are compared for equality alone."""
import numpy as np

F = np.float32
UP = np.array([0, 0, 1], F)
PREMISE_MIN_N = 63
PREMISE_MIN_WIDTH = 63

# (seed, n, width, scale, scenes): the sizes on both sides of every line the launcher draws (one wave per eye up to 128 bodies, four
# above; a second pass over the bodies above 64 / 256), three scenes each (B = 1 takes the first), two at n = 2 048
SIZES = {n: (1100, n, 1024, 1.0, 3) for n in (1, 2, 3, 63, 64, 65, 100, 128, 129, 257)}
SIZES[2048] = (5, 2048, 1024, 1.0, 2)
# widths at n = 65: below, at and above a wave's 64 columns, no power of two, the maximum; narrow rows look at a scene drawn together
WIDTHS = {1: (1100, 65, 1, 0.1, 3), 63: (1100, 65, 63, 0.1, 3), 64: (1100, 65, 64, 0.1, 3), 65: (1100, 65, 65, 0.1, 3),
          1000: (1100, 65, 1000, 1.0, 3), 4096: (1100, 65, 4096, 1.0, 3)}
# SV3: the lists
LISTS = {(n, w): (1100, n, w, 0.1 if w == 64 else 1.0, 3) for n in (64, 100, 129) for w in (64, 1024)}
FLOOR = (1100, 100, 1024, 1.0, 64)
ROWS = list(SIZES.values()) + list(WIDTHS.values()) + list(LISTS.values()) + [FLOOR]


def batch(oracle, row, scenes=None):
    """(pos, vel), (scenes, n, 3) each, of a row"""
    seed, n, _, scale, b = row
    b = b if scenes is None else scenes
    states = [oracle.init_state(n, seed + s) for s in range(b)]
    return (np.stack([p for p, _ in states]) * F(scale)).astype(F), np.stack([v for _, v in states]).astype(F)


def holds_premises(row):
    return row[1] >= PREMISE_MIN_N and row[2] >= PREMISE_MIN_WIDTH
