"""The rule of a scene batch, stated again: the C oracle applied scene by scene.  A loop and nothing more.

TEST INFRASTRUCTURE.  pos, vel: (B, n, 3) float32; the result has the same shape."""
import numpy as np


def nbody(oracle, pos, vel, k, **constants):
    """k update_instance_nbody of every scene; constants: oracle.run's dt, g, bias"""
    out = [oracle.run(pos[s], vel[s], k, **constants) for s in range(len(pos))]
    return np.stack([p for p, _ in out]), np.stack([v for _, v in out])


def boids(oracle, pos, vel, k, params=None):
    """k update_instance_boids of every scene; params: an oracle BoidsParams, None for the reference's constants"""
    out = [oracle.boids_run(pos[s], vel[s], k, params) for s in range(len(pos))]
    return np.stack([p for p, _ in out]), np.stack([v for _, v in out])
