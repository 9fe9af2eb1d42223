"""CPU tests of the scene batches' evolution-strategies generation: the premises of
tests/test_gpu_scenes_es.py.  The restatement (tests/es_restatement.py) is held to Philox's known answers, to the draw's stated
distribution, to the structure E2-E7 promise and to a hand case in exact integers and rationals; every control arm is shown to change
a word on every case it can bear on; and the update is shown to mean what it says: the restatement's loop walks towards a target, the
reversed arm does not.  Nothing here needs a device.

Which cases an arm can bear on:
  swap_sm, odd_x01, nine_rounds, no_bump, uncentred   every population case with sigma above the subnormals, and every update case of B >= 2 (through A)
  (uncentred                                          an update only where the utilities of the odd scenes do not sum to 0)
  no_mirror                                           those with a scene of odd index in them; an update only where such a scene has u != 0
  fma                                                 the population cases of 64 words and more (E3) and the update cases of B >= 64 and M >= 79 (E7)
  near_f64                                            the update cases that weigh a `near` above 2^53 which binary64 cannot hold: kind "near", B >= 2
  no_skip                                             the update cases with a non-finite value in a field of coefficient 0: "special", "near"
  nan_best                                            the update cases with a NaN fitness and B >= 2: "special"
  ties_desc                                           the update cases in which two scenes share a key32, read from the rule's own keys: "ties" from
                                                      B = 64, "equal" from B = 2, "special" from B = 10 (its two zeros, its two NaNs) among them
  u_is_r, reversed                                    the update cases of B >= 2 that are not all ties with A = 0: every kind but none at B = 1
  a32                                                 the update cases at B = 4 096"""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import es_cases as K
import es_restatement as E
import score_restatement as Q
from nenbody_amd import _lib
from nenbody_amd._lib import ES_PROTOTYPES   # (the parent commit has no such table: the file fails here)

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAW_ARMS = ("swap_sm", "odd_x01", "nine_rounds", "no_bump", "uncentred")


def words(x):
    return " ".join("%08x" % int(v) for v in x)


# -- E1 -------------------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    ones = 0xFFFFFFFF
    assert words(E.philox((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert words(E.philox((ones,) * 4, (ones,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert words(E.philox((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    assert words(E.philox((0, 0, 0, 0), (0, 0), rounds=9)) != words(E.philox((0, 0, 0, 0), (0, 0)))
    vec = E.philox((np.array([0, ones]), np.array([0, ones]), np.array([0, ones]), np.array([0, ones])), (np.array([0, ones]), np.array([0, ones])))
    assert words(v[0] for v in vec) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8" and words(v[1] for v in vec) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


# -- E2 -------------------------------------------------------------------------------------------------------------------------------------
def test_the_draw():
    assert E.C.view(np.uint32) == 0x37DDB3D7 and E.C == F32(np.sqrt(3.0) * 2.0 ** -16)
    k = E.draws(1234, 0, np.arange(0, 1024, 2), np.arange(1024))                         # 524 288 draws of even scenes: none mirrored
    assert k.shape == (512, 1024) and np.abs(k).max() <= E.K_MAX
    e = E.noise(k)
    assert (np.abs(e) <= F32(E.K_MAX) * E.C).all()                                       # |e| <= 131 070 C
    assert (E.noise(np.array([E.K_MAX, -E.K_MAX])) == np.array([1, -1], F32) * (F32(E.K_MAX) * E.C)).all()
    e = e.astype(np.float64)
    print("mean", e.mean(), "deviation", e.std(), "fourth moment", (e ** 4).mean())
    assert abs(e.mean()) < 0.01 and abs(e.std() - 1.0) < 0.01 and 2.6 < (e ** 4).mean() < 2.8   # Irwin-Hall of four: 2.7
    whole = E.noise(E.draws(1234, 0, np.arange(256), np.arange(2048))).astype(np.float64)   # 524 288 draws, mirrored
    assert whole.mean() == 0.0 and abs(whole.std() - 1.0) < 0.01 and 2.6 < (whole ** 4).mean() < 2.8


def test_mirroring_and_independence_of_b():
    for seed, g in ((K.SEED, 0), (K.SEED_HIGH, 0xFFFFFFFF)):
        k = E.draws(seed, g, np.arange(65), np.arange(79))
        assert (k[0:64:2] == -k[1:64:2]).all() and (k != 0).any()
        assert (k == E.draws(seed, g, np.arange(4096), np.arange(79))[:65]).all()        # E8: a scene's draw does not know B
        part = E.draws(seed, g, np.arange(3, 65), np.arange(79))
        assert (part == k[3:]).all()
    mean = K.mean_of(79)
    whole, five = E.population(mean, K.SIGMA, K.SEED, 1, 0, 256), E.population(mean, K.SIGMA, K.SEED, 1, 0, 5)
    assert whole[:5].tobytes() == five.tobytes()
    assert E.population(mean, K.SIGMA, K.SEED, 1, 3, 4).tobytes() == whole[3:7].tobytes()
    assert (E.population(mean, 0.0, K.SEED, 1, 0, 5) == mean[None]).all()                # sigma 0: the mean, five times
    sub = E.population(mean, K.SUBNORMAL, K.SEED, 1, 0, 64)
    assert (sub == mean[None]).all()                                                     # a subnormal term vanishes against these means
    tiny = E.population(np.zeros(79, F32), K.SUBNORMAL, K.SEED, 1, 0, 64)
    assert (tiny != 0).any() and (np.abs(tiny) < np.finfo(F32).tiny).all()               # and is kept against +0


# -- E5, E6, E7 -----------------------------------------------------------------------------------------------------------------------------
def test_ranks_are_a_permutation_and_utilities_sum_to_zero():
    for case in K.update_cases():
        r, phi, rep, mean = K.update(case)
        b = case[2]
        assert sorted(r.tolist()) == list(range(b)), case
        assert int(E.utilities(r).sum()) == 0, case
        assert int(r[int(rep["best_scene"])]) == b - 1 and rep["nan_count"] == int(np.isnan(phi).sum()) and rep["generation"] == K.update_generation(case)
    rec, coef = K.records(65, "special")
    phi = E.fitness(rec, coef)
    r = E.ranks(phi)
    nan = np.isnan(phi)
    assert nan.sum() == 2 and sorted(r[nan].tolist()) == [0, 1] and r[1] < r[11]         # NaNs lowest, by index
    assert phi[3] == -np.inf and r[3] == 2 and phi[5] == np.inf and r[5] == 64           # goal2 = +inf is the worst number, -inf the best
    assert phi[7].view(np.uint32) == 0 and phi[9].view(np.uint32) == 0 and r[9] == r[7] + 1   # -0 and +0 weigh the same: +0, a tie by index
    order = np.argsort(E.fitness(*K.records(256, "random")), kind="stable")
    assert (E.ranks(E.fitness(*K.records(256, "random")))[order] == np.arange(256)).all()
    assert E.keys(F32([-0.0, 0.0]))[0] < E.keys(F32([0.0, 0.0]))[0]                      # the map itself puts -0 below +0
    assert [k >> 32 for k in E.keys(F32([np.nan, -np.inf, -1, -0.0, 0.0, 1, np.inf]))] == sorted(k >> 32 for k in E.keys(F32([np.nan, -np.inf, -1, -0.0, 0.0, 1, np.inf])))


def test_a_population_of_one_leaves_the_mean_alone():
    for f, h in K.SHAPES:
        mean = K.mean_of(K.floats(f, h))
        r, phi, rep, new = E.rank_and_update(mean, K.SIGMA, K.STEP, K.COEF_GOAL, K.SEED, 5, K.records(1, "random")[0])
        assert r.tolist() == [0] and rep["best_scene"] == 0 and new.tobytes() == mean.tobytes()


def test_equal_fitnesses_rank_by_index_and_step_zero():
    for b in (2, 65, 256):
        r, phi, rep, new = K.update((8, 7, b, "equal"))
        assert (r == np.arange(b)).all() and rep["best_scene"] == b - 1 and len(set(phi.tolist())) == 1
    for case in ((8, 7, 65, "random"), (8, 7, 256, "ties")):
        assert K.update(case, step=F32(0))[3].tobytes() == K.mean_of(79).tobytes()


# -- the premises of the GPU cases ------------------------------------------------------------------------------------------------------------
def test_sums_pass_24_bits_at_256_and_31_bits_at_the_limit():
    a = np.abs(np.array(E.sums(K.SEED, 3, K.update((64, 32, 256, "random"))[0], K.floats(64, 32)), dtype=np.float64))
    print("B = 256: max |A|", a.max(), "median", np.median(a))
    assert a.max() > 2 ** 24 and (a > 2 ** 24).mean() > 0.5 and a.max() < 2 ** 42
    for case in ((2, 1, K.LIMIT_B, "random"), (8, 7, K.LIMIT_B, "special")):
        a = np.abs(np.array(E.sums(K.SEED, K.update_generation(case), K.update(case)[0], K.floats(*case[:2])), dtype=np.float64))
        print("B = 4096: max |A|", a.max(), "median", np.median(a))
        assert a.max() > 2 ** 31 and a.max() < 2 ** 42, case
    assert 4096 * 4095 * E.K_MAX < 2 ** 42                                               # E7's bound


def test_float_of_a_64_bit_integer():
    n = (1 << 60) + (1 << 36) + 1
    assert E.f32_of_int(n) == F32(2.0 ** 60 + 2.0 ** 37) and F32(np.float64(n)) == F32(2.0 ** 60)   # once, and through binary64
    assert E.f32_of_int((1 << 24) + 1) == F32(2 ** 24) and E.f32_of_int((1 << 24) + 3) == F32(2 ** 24 + 4) and E.f32_of_int((1 << 64) - 1) == F32(2.0 ** 64)
    rng = np.random.default_rng(3)
    for n in [int(x) for x in rng.integers(0, 1 << 63, 200)] + [int(x) >> int(s) for x, s in zip(rng.integers(0, 1 << 63, 200), rng.integers(0, 60, 200))]:
        assert E.f32_of_int(n) == rn(Fraction(n)), n
    assert E.f32_of_signed(-n) == -E.f32_of_int(n)
    rec, coef = K.records(65, "near")
    assert E.fitness(rec, coef)[63] == F32(2.0 ** 60 + 2.0 ** 37) and E.fitness(rec, coef, "near_f64")[63] == F32(2.0 ** 60)


# -- the control arms -------------------------------------------------------------------------------------------------------------------------
def test_every_arm_changes_a_word_of_every_population_case_it_bears_on():
    for case in K.population_cases():
        f, h, b, g, seed, sigma, first = case
        if not sigma >= K.SIGMA:                                                         # sigma 0 and a subnormal sigma: the mean itself
            assert all(not K.differs(K.population(case), K.population(case, arm)) for arm in DRAW_ARMS + ("no_mirror", "fma"))
            continue
        for arm in DRAW_ARMS:
            assert K.differs(K.population(case), K.population(case, arm)), (case, arm)
        assert K.differs(K.population(case), K.population(case, "no_mirror")) == (b >= 2 or first % 2 == 1), case
        if b * K.floats(f, h) >= 64:
            assert K.differs(K.population(case), K.population(case, "fma")), case
        for arm in ("near_f64", "no_skip", "nan_best", "ties_desc", "u_is_r", "reversed", "a32"):
            assert not K.differs(K.population(case), K.population(case, arm))


def test_every_arm_changes_a_word_of_every_update_case_it_bears_on():
    for case in K.update_cases():
        f, h, b, kind = case
        rule = K.update(case)
        bears = {arm: b >= 2 for arm in DRAW_ARMS + ("no_mirror", "u_is_r", "reversed")}
        bears["no_mirror"] = bool((E.utilities(rule[0])[1::2] != 0).any())                # B = 3 ranked in order gives its odd scene u = 0
        assert bears["no_mirror"] == (b >= 2) or b == 3
        bears["uncentred"] = int(E.utilities(rule[0])[1::2].sum()) != 0                   # A moves by 131 070 (sum of even u - sum of odd u)
        assert bears["uncentred"] == (b >= 2) or b == 3 or kind == "equal"
        bears["fma"] = b >= 64 and K.floats(f, h) >= 79                                   # (smaller sums move the mean by too little to tell: not asserted)
        bears["near_f64"] = kind == "near" and b >= 2
        bears["no_skip"] = kind in ("special", "near")
        bears["nan_best"] = kind == "special" and b >= 2
        bears["ties_desc"] = len({k >> 32 for k in E.keys(rule[1])}) < b
        assert bears["ties_desc"] or not ((kind == "ties" and b >= 64) or (kind == "equal" and b >= 2) or (kind == "special" and b >= 10))
        bears["a32"] = b == K.LIMIT_B
        assert set(bears) == set(E.ARMS)
        for arm in E.ARMS:
            if b == K.LIMIT_B and arm in DRAW_ARMS + ("no_mirror", "fma", "u_is_r"):     # (kept short: the limit is there for a32 and the ranks)
                continue
            if arm == "fma" and not bears[arm] and b >= 2:
                continue
            assert K.differs(rule, K.update(case, arm)) == bears[arm], (case, arm)


# -- the hand case ----------------------------------------------------------------------------------------------------------------------------
def rn(x):
    """the binary32 nearest to the rational x, ties to even, as a float32; |x| below 2^128"""
    x = Fraction(x)
    if x == 0:
        return F32(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    while Fraction(2) ** e > a:
        e -= 1
    while Fraction(2) ** (e + 1) <= a:
        e += 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    q = a / quantum
    n = q.numerator // q.denominator
    rest = q - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2):
        n += 1
    v = n * quantum
    out = F32(float(v))                                                                  # exact: 24 bits
    assert Fraction(float(out)) == v
    return -out if x < 0 else out


def fr(v):
    return Fraction(float(v))


def test_hand_case_in_integers_and_rationals():
    """B = 4, M = 7 (F = 2, H = 1): the Philox words are the restatement's, which the known answers hold; everything behind them is
    worked here in Python integers and Fractions with this file's own rn"""
    b, m, seed, g = 4, 7, 0x0123456789ABCDEF, 9
    sigma, step = F32(0.25), F32(2.0 ** -10)
    cfr = Fraction(float(E.C))
    mean = F32([0.5, -0.25, 1.0, 0.0, -0.0, 3.0, -1.5])
    k = [[0] * m for _ in range(b)]
    for q in range(2):
        for p in range(4):
            x = [int(w) for w in E.philox((p, q, g, 0), (seed & 0xFFFFFFFF, seed >> 32))]
            for half, (a_, b_) in enumerate(((x[0], x[1]), (x[2], x[3]))):
                if 2 * p + half < m:
                    v = (a_ & 0xFFFF) + (a_ >> 16) + (b_ & 0xFFFF) + (b_ >> 16) - 131070
                    k[2 * q][2 * p + half], k[2 * q + 1][2 * p + half] = v, -v
    assert all(-131070 <= v <= 131070 for row in k for v in row) and (np.array(k) == E.draws(seed, g, np.arange(b), np.arange(m))).all()
    theta = np.array([[rn(Fraction(float(mean[j])) + Fraction(float(rn(Fraction(float(sigma)) * Fraction(float(rn(k[s][j] * cfr)))))))
                       for j in range(m)] for s in range(b)], F32)
    assert theta.tobytes() == E.population(mean, sigma, seed, g, 0, b).tobytes()
    rec = np.zeros(b, Q.DTYPE)
    rec["near"], rec["goal2"], rec["nonfinite"], rec["speed2"] = [3, 1, 3, 0], F32([2.0, 0.5, 2.0, 8.0]), [0, 1, 0, 0], F32(np.nan)
    coef = (0.5, 0.0, 0.0, 0.0, -1.0, -0.25)                                             # speed2 is a NaN and is not weighed
    phi = []
    for rec_s in rec:                                                                    # E4, the zero coefficients skipped
        t = rn(Fraction(0) + fr(rn(Fraction(1, 2) * int(rec_s["near"]))))
        t = rn(fr(t) + fr(rn(Fraction(-1) * fr(rec_s["goal2"]))))
        phi.append(rn(fr(t) + fr(rn(Fraction(-1, 4) * int(rec_s["nonfinite"])))))
    assert [float(p) for p in phi] == [-0.5, -0.25, -0.5, -8.0]
    r = [sum(1 for t in range(b) if (phi[t], t) < (phi[s], s)) for s in range(b)]
    assert r == [1, 3, 2, 0]                                                             # the tie of scenes 0 and 2 goes by index
    u = [2 * x - (b - 1) for x in r]
    assert u == [-1, 3, 1, -3] and sum(u) == 0
    a = [sum(u[s] * k[s][j] for s in range(b)) for j in range(m)]
    new = np.array([rn(Fraction(float(mean[j])) + Fraction(float(rn(Fraction(float(step)) * Fraction(float(rn(a[j] * cfr))))))) for j in range(m)], F32)
    got = E.rank_and_update(mean, sigma, step, coef, seed, g, rec)
    assert got[0].tolist() == r and E.same_floats(got[1], F32(phi)) and E.sums(seed, g, r, m) == a and got[3].tobytes() == new.tobytes()
    assert got[2]["best_scene"] == 1 and got[2]["best_fitness"] == F32(-0.25) and got[2]["nan_count"] == 0 and got[2]["generation"] == g
    assert (new != mean).sum() >= 6


# -- what the update means --------------------------------------------------------------------------------------------------------------------
GENERATIONS = 60


def search(variant=None):
    """the restatement's loop on crafted records: goal2 = |theta_s - target|^2, nothing else weighed; the distances of the mean to the
    target before and after GENERATIONS generations"""
    b, m = 64, 7
    target = np.random.default_rng(21).uniform(-1, 1, m).astype(F32)
    mean = np.zeros(m, F32)
    sigma = F32(0.1)
    step = F32(float(sigma) / (2.0 * b * (b - 1)))                                       # utilities scaled to [-1/2, 1/2], 1/(B sigma), rate sigma^2
    first = float(np.linalg.norm(mean.astype(np.float64) - target))
    for g in range(GENERATIONS):
        theta = E.population(mean, sigma, 77, g, 0, b)
        rec = np.zeros(b, Q.DTYPE)
        rec["goal2"] = ((theta - target[None]).astype(np.float64) ** 2).sum(1).astype(F32)
        mean = E.rank_and_update(mean, sigma, step, K.COEF_GOAL, 77, g, rec, variant)[3]
    return first, float(np.linalg.norm(mean.astype(np.float64) - target))


def test_the_loop_walks_to_the_target_and_the_reversed_arm_does_not():
    first, last = search()
    back = search("reversed")[1]
    print("distance", first, "->", last, "; reversed ->", back)
    assert last <= 0.5 * first
    assert back > 0.5 * first and back > first


# -- the library's side -----------------------------------------------------------------------------------------------------------------------
NAMES = {"nb_scenes_es_perturb_launch": 9, "nb_scenes_es_update_launch": 12, "nb_scenes_es_set": 6, "nb_scenes_es_perturb": 1, "nb_scenes_es_update": 1,
         "nb_scenes_es_mean": 2, "nb_scenes_es_result": 4, "nb_scenes_es_generation": 1, "nb_scenes_keep": 1, "nb_scenes_rewind": 1}


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nenbody_scenes_es.h")).read(), flags=re.S)


def test_the_header_the_table_and_the_library_agree(nb):
    text = header()
    assert sorted(re.findall(r"\b(nb_[a-z_0-9]+)\s*\(", text)) == sorted(NAMES) == sorted(ES_PROTOTYPES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, c_args in NAMES.items():
        declared = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert declared.count(",") + 1 == c_args == len(ES_PROTOTYPES[name][1]) and hasattr(lib, name) and hasattr(_lib.load(), name), name
    main = open(os.path.join(ROOT, "include", "nenbody.h")).read()
    assert '#include "nenbody_scenes_es.h"' in main and int(re.search(r"#define NB_ABI_VERSION (\d+)", main).group(1)) == 2
    rule = [main.index(" *   E%d:" % i) for i in range(1, 9)]
    assert rule == sorted(rule) and main.index('#include "nenbody_scenes_score.h"') < rule[0] and rule[-1] < main.index('#include "nenbody_scenes_es.h"')
    assert main.index("} nb_es_report;") < main.index('#include "nenbody_scenes_es.h"')
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "0x37DDB3D7", "131070", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"):
        assert word in main, word                                                        # the rule stands alone
    assert _lib.NB_ES_MAX_POPULATION == E.MAX_POPULATION == int(re.search(r"#define NB_ES_MAX_POPULATION (\d+)u", main).group(1))
    assert nb.ES_REPORT_DTYPE == E.REPORT_DTYPE and nb.ES_REPORT_DTYPE.itemsize == ctypes.sizeof(_lib.NbEsReport) == 16
    kernels = open(os.path.join(ROOT, "nenbody_amd", "csrc", "nb_scenes_es.inc")).read()
    assert kernels.count("0xD2511F53u") == 2 and kernels.count("es_philox(") == 2        # the round is written once, and called once
