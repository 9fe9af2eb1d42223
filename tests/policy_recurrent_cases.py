"""Inputs of the tests of the scene batches' recurrent policy: tests/test_scenes_policy_recurrent_cpu.py,
tests/test_gpu_scenes_policy_recurrent.py.

TEST INFRASTRUCTURE.  The batches are policy_cases' (scenes_seen_cases.batch from policy_cases.row), at the smallest shapes at which
the recurrent kernel can go wrong: both launch shapes and both sides of the switch at 128 bodies, a narrow and a wider row, one
feature and several, one hidden unit, a count that is no power of two and every lane of a 64-lane workgroup.  A case's recurrent
policy is policy_cases.policies' (w1, b1, w2, b2) with a wr drawn here: wr[0, 0] = 0.7f, so that unit 0, which is on for an eye that
sees somebody near, feeds itself; the other words in [-1, 1) / H.  The memory limit S = 0.017f lies inside the range of the hidden
values: b1 lies in [-0.02, 0.02) and a seeing eye's unit 0 is about the mean of x, far above S.  Neither 0.7f nor 0.017f is a power of
two, so the product of a clipped memory word and its weight is not exact and a fused chain can be told from the rule with H = 1."""
import numpy as np

import policy_cases as K
import policy_recurrent_restatement as RR
import policy_restatement as P
from policy_cases import LIMIT, SCENES, UP, batch, limit, row, special_scene  # noqa: F401  (the tests' C.*)

F32 = np.float32
SIZES = (5, 128, 129)                  # both lane shapes, both sides of the line at 128 bodies
WIDTHS = (8, 64)
FEATURES = (1, 8)
HIDDEN = (1, 7, 64)
STEPS = 3                              # memory written by step 1 is read by step 2 and overwritten in place by step 3
MEMORY_LIMIT = F32(0.017)


def memory_limit(own):
    """S of a case's run: MEMORY_LIMIT with a policy per scene, none with one policy for all -- there every rounding of the chain
    reaches the memory, where the limit would hide it for every unit above S"""
    return MEMORY_LIMIT if own else F32(np.inf)


# (n, width, F, H): 36 cases
CASES = [(n, w, f, h) for n in SIZES for w in WIDTHS for f in FEATURES for h in HIDDEN]


def recurrent_weights(features, hidden, count, seed=7):
    """wr of `count` policies, (count, H, H) float32"""
    rng = np.random.default_rng([seed, features, hidden, 14_8])
    wr = (rng.uniform(-1, 1, (count, hidden, hidden)) / hidden).astype(F32)
    wr[:, 0, 0] = F32(0.7)
    return wr


def policies(features, hidden, count, seed=7, zero_wr=False):
    """(count, policy_recurrent_floats) float32: policy_cases.policies with wr between w1 and b1; zero_wr: every word of wr +0 (R6)"""
    wr = np.zeros((count, hidden, hidden), F32) if zero_wr else recurrent_weights(features, hidden, count, seed)
    out = []
    for pol, r in zip(K.policies(features, hidden, count, seed), wr):
        w1, b1, w2, b2 = P.unpack(pol, features, hidden)
        out.append(RR.pack(w1, r, b1, w2, b2))
    return np.stack(out)


def feedforward(pol, features, hidden):
    """the P-rule policies of recurrent ones, (count, policy_floats)"""
    return np.stack([RR.feedforward(p, features, hidden) for p in pol])


# -- the hand case: DESIGN.md sections 12 and 13's two bodies, F = 8, H = 2, two steps -------------------------------------------------------
HAND_SHAPE = (1024, 8, 2)              # W, F, H
HAND_MEMORY_LIMIT = F32(0.125)


def hand_policy():
    """unit 0 reads bins 3 and 4 and half of its own memory; unit 1 reads a quarter of unit 0's memory and nothing else; o_0 = h_0,
    o_1 = h_1"""
    w1 = np.zeros((8, 2), F32)
    w1[3, 0] = w1[4, 0] = 1
    wr = np.array([[0.5, 0.25], [0, 0]], F32)          # wr[r, j]
    return RR.pack(w1, wr, np.zeros(2, F32), np.array([[1, 0], [0, 1]], F32), np.zeros(2, F32))


# -- what memory MEANS: body 1 crosses eye 0's slit and leaves it -----------------------------------------------------------------------------
MEANING_SHAPE = (64, 8, 1)             # W, F, H
MEANING_STEPS = 12
MEANING_POS = np.array([[0, 0, 0], [6, -8.5, 0]], F32)
MEANING_VEL = np.array([[1, 0, 0], [1, 2, 0]], F32)     # p = v + p: body 1 stays 6 ahead of body 0 and drifts across its slit, 2 a step


def meaning_policy():
    """w2 = b2 = 0: both bodies move in straight lines.  Unit 0: b1 = 0, a large positive row of w1, wr[0, 0] = 1; S = 1: m_0 is 1.0 from
    the first step with anybody in the slit on, whatever the row shows afterwards"""
    w1 = np.full((8, 1), 64, F32)
    return RR.pack(w1, np.ones((1, 1), F32), np.zeros(1, F32), np.zeros((2, 1), F32), np.zeros(2, F32))
