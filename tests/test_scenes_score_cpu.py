"""CPU tests of the scene batches' score: the premises the GPU tests rest on, checked on the very cases of
tests/score_cases.py through the numpy restatement of Q1-Q7, with control arms; a hand case of three bodies derived in exact
rationals; the header, the binding, the library, the C++ host and the Rust shim agree on the six entries."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import score_cases as K
import score_restatement as Q
from conftest import ROOT
from nenbody_amd._lib import SCENES_SCORE_PROTOTYPES   # (the parent commit has no such table: the file fails here)

F = np.float32
NAMES = ["nb_scenes_score_launch", "nb_scenes_set_score", "nb_scenes_score", "nb_scenes_score_reset", "nb_scenes_scores",
         "nb_scenes_step_policy_scored"]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def arm(kind, n, variant):
    pos, vel, radius_sq, goal = K.make(kind, n)
    rule = K.want(kind, n)
    pairs = variant in ("fma", "le", "ordered")               # the arms that bear on Q2; the others take its count from the rule
    return np.stack([Q.accumulate(np.zeros((), Q.DTYPE),
                                  Q.terms(pos[s], vel[s], radius_sq, goal, variant, None if pairs else int(rule[s]["near"])))
                     for s in range(K.SCENES)])


# -- the premises ------------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_what_the_issue_lists():
    assert K.SCENES == 3 and K.SIZES == (1, 2, 5, 64, 65, 100, 128, 129, 256, 300, 512, 513, 1024, 1025, 1537, 2048)
    assert len(K.KINDS) == 7 and len(K.CASES) == 7 * 16
    assert Q.DTYPE.itemsize == 32 and Q.DTYPE.names == ("near", "spread", "speed2", "momentum2", "goal2", "steps", "nonfinite")
    assert [Q.pow2_at_least(n) for n in (1, 2, 3, 5, 64, 65, 1025, 2048)] == [1, 2, 4, 8, 64, 128, 2048, 2048]


@pytest.mark.parametrize("kind", K.KINDS)
def test_premises_of_every_case(kind):
    """the scenes of a batch are distinct; radius_sq is a d2 some pair attains; every scene with three pairs and more has a pair inside
    and a pair outside; what the kind is for holds: a plane, clumps, squares that are subnormal or zero, integers, the outliers where
    the docstring of score_cases.outliers puts them"""
    for n in K.SIZES:
        pos, vel, radius_sq, goal = K.make(kind, n)
        rule = K.want(kind, n)
        assert pos.shape == vel.shape == (3, n, 3) and pos.dtype == vel.dtype == F and radius_sq >= 0 and np.isfinite(goal).all()
        assert all((bits(pos[a]) != bits(pos[b])).any() for a, b in ((0, 1), (0, 2), (1, 2)))
        assert (rule["steps"] == 1).all()
        if n >= 2:
            assert any((bits(Q.pair_d2(pos[s])) == bits(radius_sq)).any() for s in range(3)), (kind, n)
        if n >= 5:
            for s in range(3):
                assert 0 < int(rule[s]["near"]) < n * (n - 1) // 2, (kind, n, s)
        if kind == "planar":
            assert (pos[..., 2] == 0).all() and (vel[..., 2] == 0).all()
        if kind == "tiny":                                     # every square is below the least normal: subnormal or zero
            with np.errstate(all="ignore"):
                assert (pos * pos < np.finfo(F).tiny).all() and (vel * vel < np.finfo(F).tiny).all()
                assert (bits(pos * pos) != 0).any() and (n > 100 or rule["speed2"].max() < np.finfo(F).tiny)
        if kind == "large":
            assert 1e3 < np.abs(pos).max() <= 2e5 and (n < 64 or np.abs(pos).max() > 1.5e5)
        if kind == "lattice":
            assert (pos == np.rint(pos)).all() and (vel == np.rint(vel)).all()
        if kind == "nonfinite":
            first, last, second = K.outliers(n)
            assert set(first) <= {0, 64 * ((n - 1) // 64)} and n - 1 in last and all(i % 64 == 0 for i in first)
            assert (n <= 1024) == (second == []) and all(i >= 1024 for i in second)
            assert rule["nonfinite"].tolist() == [len(set(first) | set(last)), len(set(first) | set(last)), len(set(second) | {0})]
            assert np.isfinite(rule[0]["speed2"]) and np.isfinite(rule[0]["momentum2"]) and np.isnan(rule[0]["spread"])
            assert np.isfinite(rule[1]["spread"]) and np.isfinite(rule[1]["goal2"]) and np.isnan(rule[1]["speed2"])
            assert not any(np.isfinite(rule[2][f]) for f in Q.FLOATS)
        else:
            assert (rule["nonfinite"] == 0).all() and all(np.isfinite(rule[f]).all() for f in Q.FLOATS)


# Which cases an arm can bear on, from what it changes:
#   an order of summation ("serial", "adjacent", "float64") needs three leaves and sums that round: n >= 5 here; not the lattice, whose
#     sums are exact in any order; not the tiny kind, whose squares are multiples of 2^-149 and add exactly until a sum passes 2^-125,
#     which a small scene's does not; not the nonfinite kind, which leaves a scene two finite float fields -- a NaN meets a NaN
#   "fma" needs a product that rounds and a d2 at the radius that a fused d2 falls below: score_cases.attained_radius sees to the
#     second wherever it is asked to: n >= 64; not the lattice, whose products are exact; not the tiny kind, where rounding is to
#     multiples of 2^-149 whatever the magnitude, and adding such a multiple before or after the rounding is the same but for ties.  It is `near` that tells: a sum of
#     thousands of squares absorbs the last bit of its leaves more often than not
#   "le" needs a pair at the radius: n >= 2 (radius_sq is attained)
#   "ordered" needs a pair inside: n >= 2; not the nonfinite kind at n = 2, where only scene 1's pair is finite and it lies AT the radius
#   "recip" needs a centroid that T * (1/n) rounds to another word than T / n -- the test looks, with the restatement's tree alone --
#     and whose last bit moves the sum of the squares: the clustered kind, whose bodies lie within 2^-13 of a point of size 1
#     (elsewhere a sum of squares of size 1 absorbs it more often than not)
def reciprocal_moves_a_centroid(kind, n):
    pos = K.make(kind, n)[0]
    t = np.stack([Q.tree(p) for p in pos])
    return bool((bits(t / F(n)) != bits(t * (F(1) / F(n)))).any())


ROUNDS = [k for k in K.KINDS if k not in ("lattice", "tiny", "nonfinite")]
BEARS = {
    "serial": lambda kind, n: kind in ROUNDS and n >= 5,
    "adjacent": lambda kind, n: kind in ROUNDS and n >= 5,
    "float64": lambda kind, n: kind in ROUNDS and n >= 5,
    "fma": lambda kind, n: kind not in ("lattice", "tiny") and n >= 64,
    "le": lambda kind, n: n >= 2,
    "ordered": lambda kind, n: n >= 2 and (kind, n) != ("nonfinite", 2),
    "recip": lambda kind, n: kind == "clustered" and n >= 5 and reciprocal_moves_a_centroid(kind, n),
}


@pytest.mark.parametrize("variant", sorted(BEARS))
def test_control_arms_change_a_word(variant):
    """every case the arm can bear on (the table above): the departure from the rule changes a word of some scene's record"""
    cases = [c for c in K.CASES if BEARS[variant](*c)]
    assert len(cases) >= 4
    for kind, n in cases:
        assert not Q.same(arm(kind, n, variant), K.want(kind, n)), (variant, kind, n)


@pytest.mark.parametrize("variant", ["skip_padding", "workgroup"])
def test_padding_changes_no_word(variant):
    """Q1's licence, proven by running both ways on every case: leaving out the adds whose right operand is padding, and running the
    tree over the 64 leaves of the smallest workgroup, give every word of every record"""
    for kind, n in K.CASES:
        assert Q.same(arm(kind, n, variant), K.want(kind, n)), (variant, kind, n)


def test_padding_can_change_the_sign_of_a_zero_sum_only():
    """what the licence costs: T of negative zeros is -0 by the rule with padding skipped and +0 with it added -- and the fields square
    it, subtract it from a coordinate that is squared, or sum squares, so none can tell"""
    u = F([-0.0, -0.0, -0.0])
    assert bits(Q.tree(u, "skip_padding")) == 0x80000000 and bits(Q.tree(u)) == 0 and bits(Q.tree(u, "workgroup")) == 0
    pos = np.zeros((3, 3), F)
    pos[:, 0] = -0.0
    vel = -np.zeros((3, 3), F)
    records = [Q.terms(pos, vel, F(1), F([0, 0, 0]), v) for v in (None, "skip_padding", "workgroup")]
    assert Q.same(records[1], records[0]) and Q.same(records[2], records[0])
    assert all(bits(records[0][f]) == 0 for f in Q.FLOATS)


def test_one_body():
    for kind in K.KINDS:
        rule = K.want(kind, 1)
        assert (rule["near"] == 0).all()
        if kind != "nonfinite":
            assert (bits(rule["spread"]) == 0).all(), kind    # c = p / 1 = p: e = +0


def test_accumulation_is_a_chain_in_call_order():
    pos, vel, radius_sq, goal = K.make("random", 100)
    t = [Q.terms(pos[s], vel[s], radius_sq, goal) for s in range(3)]
    acc = np.zeros((), Q.DTYPE)
    for term in t:
        acc = Q.accumulate(acc, term)
    assert int(acc["near"]) == sum(int(x["near"]) for x in t) and acc["steps"] == 3
    assert bits(acc["spread"]) == bits((t[0]["spread"] + t[1]["spread"]) + t[2]["spread"])
    wrap = np.zeros((), Q.DTYPE)
    wrap["steps"] = 0xFFFFFFFF
    assert Q.accumulate(wrap, t[0])["steps"] == 0


# -- the hand case in exact rationals ------------------------------------------------------------------------------------------------------
def rn(q):
    """the binary32 nearest to the rational q, ties to even (no overflow: the hand case stays near 1)"""
    q = Fraction(q)
    if q == 0:
        return q
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    k = q / ulp
    lo = k.numerator // k.denominator
    rest = k - lo
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    return sign * lo * ulp


def word(q):
    f = F(float(q))
    assert Fraction(float(f)) == q                             # q is a binary32
    return int(bits(f).reshape(-1)[0])


def test_the_hand_case_in_exact_rationals():
    """three bodies, P = 4: T(u) = (u_0 + u_2) + (u_1 + 0), every operation rounded by this file's rn"""
    p = [[Fraction(float(c)) for c in row] for row in K.HAND_POS]
    v = [[Fraction(float(c)) for c in row] for row in K.HAND_VEL]
    g = [Fraction(float(c)) for c in K.HAND_GOAL]

    def tree3(u):
        return rn(rn(u[0] + u[2]) + rn(u[1] + 0))

    def sq3(a, b, c):
        return rn(rn(rn(a * a) + rn(b * b)) + rn(c * c))

    def d2(a, b):
        return sq3(*[rn(a[c] - b[c]) for c in range(3)])

    near = sum(d2(p[i], p[j]) < Fraction(float(K.HAND_RADIUS_SQ)) for i in range(3) for j in range(i + 1, 3))
    assert near == 2 and d2(p[0], p[2]) < 3 < d2(p[0], p[1]) < Fraction(7, 2) < d2(p[1], p[2]) and d2(p[0], p[1]) == d2(p[1], p[0])
    centre = [rn(tree3([p[i][c] for i in range(3)]) / 3) for c in range(3)]
    spread = tree3([d2(p[i], centre) for i in range(3)])
    speed2 = tree3([sq3(*v[i]) for i in range(3)])
    momentum2 = sq3(*[tree3([v[i][c] for i in range(3)]) for c in range(3)])
    goal2 = tree3([d2(p[i], g) for i in range(3)])
    got = Q.terms(K.HAND_POS, K.HAND_VEL, K.HAND_RADIUS_SQ, K.HAND_GOAL)
    assert int(got["near"]) == near and got["steps"] == 1 and got["nonfinite"] == 0
    assert [int(bits(got[f]).reshape(-1)[0]) for f in Q.FLOATS] == [word(spread), word(speed2), word(momentum2), word(goal2)]
    assert rn(Fraction(1, 3)) != Fraction(1, 3) and spread > 0 and momentum2 > 0


# -- the entries -------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nenbody_scenes_score.h")).read(), flags=re.S)


def test_header_binding_and_library_agree(nb):
    from nenbody_amd import _lib

    header = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert sorted(re.findall(r"\b(nb_[a-z_0-9]+)\s*\(", header)) == sorted(NAMES) == sorted(SCENES_SCORE_PROTOTYPES)
    for name in NAMES:
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        assert len(SCENES_SCORE_PROTOTYPES[name][1]) == c_args and hasattr(lib, name) and hasattr(_lib.load(), name), name
        assert not name.startswith("nb_launch_") and name not in _lib.PROTOTYPES
    main = open(os.path.join(ROOT, "include", "nenbody.h")).read()
    assert '#include "nenbody_scenes_score.h"' in main and int(re.search(r"#define NB_ABI_VERSION (\d+)", main).group(1)) == 2
    assert _lib.load().nb_abi_version() == 2
    rule = [main.index(" %s:  " % q) for q in ("Q1", "Q2", "Q3", "Q4", "Q5", "Q6", "Q7")]
    assert rule == sorted(rule) and main.index('#include "nenbody_scenes_policy.h"') < rule[0]
    assert rule[-1] < main.index('#include "nenbody_scenes_score.h"')
    assert main.index("} nb_scene_score;") < main.index('#include "nenbody_scenes_score.h"')
    assert ctypes.sizeof(_lib.NbScoreParams) == 16
    for method in ("set_score", "score", "score_reset", "scores", "step_policy_scored"):
        assert callable(getattr(nb.SceneBatch, method)), method


def test_score_dtype(nb):
    assert nb.SCORE_DTYPE.itemsize == 32 and nb.SCORE_DTYPE == Q.DTYPE
    assert nb.SCORE_DTYPE.names == ("near", "spread", "speed2", "momentum2", "goal2", "steps", "nonfinite")
    assert [nb.SCORE_DTYPE.fields[f][1] for f in nb.SCORE_DTYPE.names] == [0, 8, 12, 16, 20, 24, 28]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nenbody.h")).read(), flags=re.S)
    body = re.search(r"typedef struct nb_scene_score \{(.*?)\} nb_scene_score;", header, re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == list(nb.SCORE_DTYPE.names)


def test_the_rust_shim_and_the_cpp_host_declare_the_entry_points():
    text = open(os.path.join(ROOT, "integration", "rust", "scene.rs")).read()
    header = _header()
    for name in NAMES:
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        m = re.search(r"fn %s\s*\(([^)]*)\)" % name, text)
        assert m, name
        assert m.group(1).strip().rstrip(",").count(",") + 1 == c_args, name
    for item in ("pub fn set_score(&mut self, radius_sq: f32, goal: [f32; 3])", "pub fn score(&mut self)", "pub fn score_reset(&mut self)",
                 "pub fn scores(&mut self, first_scene: u32, scene_count: u32)", "pub fn step_policy_scored(&mut self, k: u32",
                 "pub struct NbSceneScore"):
        assert item in text, item
    hpp = open(os.path.join(ROOT, "include", "nenbody_scene.hpp")).read()
    for item in ("void set_score(float radius_sq", "void score()", "void score_reset()", "std::vector<nb_scene_score> scores(",
                 "void step_policy_scored(uint32_t k, const Mat4 &cp"):
        assert item in hpp, item


def test_the_cpp_host_compiles(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "nenbody_scene.hpp"\n'
                   "static_assert(sizeof(nb_scene_score) == 32 && sizeof(nb_score_params) == 16, \"Q7\");\n"
                   "uint64_t use(nenbody::SceneBatch &b, const nenbody::Mat4 &cp) {\n"
                   "    b.set_score(0.25f, nenbody::Vec3{1.0f, 2.0f, 3.0f});\n"
                   "    b.score();\n"
                   "    b.score_reset();\n"
                   "    b.step_policy_scored(2, cp, 64);\n"
                   "    return b.scores().at(0).near + b.scores(1, 1).size();\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
