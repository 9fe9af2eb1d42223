"""Inputs of the scene-batch tests (tests/test_scenes_cpu.py, tests/test_gpu_scenes.py): scenes drawn from different seeds.

TEST INFRASTRUCTURE.  The CPU file checks on these arrays that the GPU tests can tell leakage from isolation; the GPU file feeds
them to the kernels."""
import numpy as np

from test_gpu_boids import cloud

F = np.float32
ALT_GRAVITY = dict(dt=0.05, g=0.0025, bias=1e-5)          # a second set of gravity constants (oracle.run's keywords)


def scenes(oracle, law, batch, n, seed):
    """(pos, vel), (batch, n, 3) each: gravity scenes are the reference's planar initial state, boids scenes 3-D clouds; scene s is
    drawn with seed + s"""
    draw = oracle.init_state if law == "nbody" else (lambda m, sd: cloud(oracle, m, sd))
    out = [draw(n, seed + s) for s in range(batch)]
    return np.stack([p for p, _ in out]).astype(F), np.stack([v for _, v in out]).astype(F)


def gravity_params(nb, dt, g, bias):
    p = nb.default_params()
    p.dt, p.G, p.bias = dt, g, bias
    return p
