"""Inputs of the tests of the scene batches' evolution-strategies generation: tests/test_scenes_es_cpu.py,
tests/test_gpu_scenes_es.py.

TEST INFRASTRUCTURE.  A population case is (F, H, B, generation, seed, sigma, first_scene); an update case is (F, H, B, kind) with
crafted score records of a `kind` below and the coefficients that go with it.  Expected values are the restatement's
(tests/es_restatement.py), computed once per case and cached; the CPU file holds the premises: which control arm bears on which
case."""
import functools

import numpy as np

import es_restatement as E
import score_restatement as Q

F32 = np.float32
SHAPES = ((1, 1), (2, 1), (8, 7), (64, 32))                  # M = 6, 7, 79, 2 146
POPULATIONS = (1, 2, 3, 64, 65, 256)
LIMIT_B = E.MAX_POPULATION
SEED = 1234
SEED_HIGH = 0x9E3779B97F4A7C15                               # a seed with a non-zero high word
SIGMA = F32(0.05)
SUBNORMAL = np.uint32(0x00000300).view(F32)                  # sigma * e stays subnormal: |e| < 4
STEP = F32(3e-5)
COEF_GOAL = (0.0, 0.0, 0.0, 0.0, -1.0, 0.0)                  # the nearer the goal, the better
COEF_MIX = (-2.0 ** -12, 0.5, 0.0, -0.25, -1.0, -3.0)        # speed2 is not weighed
COEF_NEAR = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0)                   # phi = (float)near
NEAR_EDGES = ((1 << 24) + 1, (1 << 60) + (1 << 36) + 1, (1 << 64) - 1)
KINDS = ("random", "ties", "special", "near", "equal")


def floats(features, hidden):
    return E.policy_floats(features, hidden)


def mean_of(m, seed=11):
    return (np.random.default_rng([seed, m]).standard_normal(m) * 0.1).astype(F32)


# (F, H, B, generation, seed, sigma, first_scene)
def population_cases():
    cases = [(f, h, b, 1, SEED, SIGMA, 0) for f, h in SHAPES for b in POPULATIONS]
    cases += [(256, 64, 3, 1, SEED, SIGMA, 0), (2, 1, LIMIT_B, 1, SEED, SIGMA, 0), (8, 7, LIMIT_B, 2, SEED_HIGH, SIGMA, 0)]
    cases += [(8, 7, 65, 0, SEED, SIGMA, 0), (8, 7, 65, 0xFFFFFFFF, SEED, SIGMA, 0), (8, 7, 65, 1, SEED_HIGH, SIGMA, 0)]
    cases += [(8, 7, 65, 1, SEED, F32(0), 0), (8, 7, 65, 1, SEED, SUBNORMAL, 0)]
    cases += [(8, 7, 64, 1, SEED, SIGMA, 3), (2, 1, 2, 1, SEED, SIGMA, 4093), (8, 7, 1, 1, SEED, SIGMA, 4095), (1, 1, 3, 1, SEED, SIGMA, 1)]   # odd first scenes
    return cases


@functools.lru_cache(maxsize=None)
def population(case, variant=None):
    f, h, b, g, seed, sigma, first = case
    out = E.population(mean_of(floats(f, h)), sigma, seed, g, first, b, variant)
    out.setflags(write=False)
    return out


def records(b, kind, seed=5):
    """crafted score records (Q.DTYPE, (B,)) and the coefficients that go with them"""
    rng = np.random.default_rng([seed, b, KINDS.index(kind)])
    rec = np.zeros(b, Q.DTYPE)
    rec["near"] = rng.integers(0, 1 << 20, b)
    for f in Q.FLOATS:
        rec[f] = rng.uniform(0.0, 100.0, b).astype(F32)
    rec["steps"] = 8
    rec["nonfinite"] = rng.integers(0, 4, b)
    coef = COEF_MIX
    if kind == "ties":                                       # four values of goal2 only: exact ties from B = 5 on, many from 64
        coef = COEF_GOAL
        rec["goal2"] = F32([1.5, 0.25, 1.5, 7.0])[rng.integers(0, 4, b)]
    elif kind == "special":                                  # specials in weighed fields (goal2) and in one that is not (speed2)
        rec["speed2"] = F32([np.nan, np.inf, -np.inf, 1.0])[np.arange(b) % 4]
        for at, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0, -np.nan)):
            if 2 * at + 1 < b:
                rec["goal2"][2 * at + 1] = F32(v)
                rec["near"][2 * at + 1], rec["spread"][2 * at + 1], rec["momentum2"][2 * at + 1], rec["nonfinite"][2 * at + 1] = 0, 0, 0, 0
    elif kind == "near":
        coef = COEF_NEAR
        for at, v in enumerate(NEAR_EDGES + ((1 << 24), (1 << 60), (1 << 53) + 1)):
            if at < b:
                rec["near"][b - 1 - at] = v
        rec["spread"] = F32(np.inf)                          # not weighed
    elif kind == "equal":
        coef = COEF_GOAL
        rec["goal2"] = F32(2.5)
    return rec, tuple(float(c) for c in coef)


# (F, H, B, kind)
def update_cases():
    cases = [(8, 7, b, kind) for b in POPULATIONS for kind in KINDS]
    cases += [(2, 1, 65, "random"), (1, 1, 256, "random"), (64, 32, 256, "random"), (64, 32, 3, "special")]
    cases += [(2, 1, LIMIT_B, "random"), (8, 7, LIMIT_B, "ties"), (8, 7, LIMIT_B, "special")]
    return cases


def update_generation(case):
    return 0xFFFFFFFF if case[1] == 1 else 3


@functools.lru_cache(maxsize=None)
def update(case, variant=None, step=STEP, seed=SEED):
    """(ranks, fitnesses, report, mean') of an update case"""
    f, h, b, kind = case
    rec, coef = records(b, kind)
    out = E.rank_and_update(mean_of(floats(f, h)), SIGMA, step, coef, seed, update_generation(case), rec, variant)
    for a in out:
        a.setflags(write=False)
    return out


def differs(a, b):
    """the two results (arrays or tuples of arrays) differ in a word, a NaN equal to a NaN"""
    if isinstance(a, tuple):
        return any(differs(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == E.REPORT_DTYPE:
        return not E.same_report(a, b)
    if a.dtype == F32:
        return not E.same_floats(a, b)
    return not (a == b).all()
