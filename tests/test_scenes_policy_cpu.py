"""CPU tests of the scene batches' neural policy: the premises the GPU tests rest on, checked on the very
cases of tests/policy_cases.py through the numpy restatements of the eye rule and of the policy, with control arms; the hand case
derived in exact rationals; the header, the binding, the library, the C++ host and the Rust shim agree on the six entries."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import eyes_restatement as R
import policy_cases as K
import policy_restatement as P
from conftest import ROOT

F = np.float32
NAMES = ["nb_policy_floats", "nb_scenes_policy_step_launch", "nb_scenes_policy_observe_launch", "nb_scenes_set_policy",
         "nb_scenes_step_policy", "nb_scenes_eyes_policy"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_rows = {}


def rows_of(oracle, pos, vel, width, key=None):
    """(ids, depth) rows of every body of one scene by the numpy eye rule; cameras and matrices by the oracle"""
    if key is None or key not in _rows:
        cams = oracle.cameras(pos, vel, K.UP, R.eye_constant(oracle, width))
        got = R.eyes(cams, oracle.instances(pos, vel), 0, width, chunk=64)
        if key is None:
            return got
        _rows[key] = got
    return _rows[key]


def restated(oracle, n, width, features, hidden, own, variant=None):
    """one step of a case's batch by the restatement: (x, o, positions, velocities)"""
    pos, vel = K.batch(oracle, K.row(n, width))
    pol = K.policies(features, hidden, K.SCENES if own else 1)
    return P.batch(lambda s, p, v: rows_of(oracle, p, v, width, (n, width, s)), pos, vel, pol, features, hidden, K.limit(n, width),
                   K.UP, variant=variant)


def differs(a, b):
    return any((bits(g) != bits(w)).any() for g, w in zip(a, b))


# -- the premises ------------------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_what_the_issue_lists():
    assert sorted({c[0] for c in K.CASES}) == [5, 128, 129, 300] and sorted({c[1] for c in K.CASES}) == [8, 64, 1024]
    assert sorted({c[3] for c in K.CASES}) == [1, 7, 64] and K.SCENES == 3
    for w in K.WIDTHS:
        assert {c[2] for c in K.CASES if c[1] == w} == {f for f in (1, 8, w) if f <= 256}
    assert len(K.CASES) == 84 and all(w % f == 0 for _, w, f, _ in K.CASES)


@pytest.mark.parametrize("n,width", [(n, w) for n in K.SIZES for w in K.WIDTHS])
def test_both_relu_branches_and_the_limit_occur(oracle, n, width):
    """every case, with a policy per scene and with one for all: some eye sees nothing and some eye sees somebody; some hidden unit is
    off and some is on; some output passes the limit and some does not; the step is not coasting"""
    pos, vel = K.batch(oracle, K.row(n, width))
    for _, _, features, hidden in [c for c in K.CASES if c[:2] == (n, width)]:
        for own in (True, False):
            pol = K.policies(features, hidden, K.SCENES if own else 1)
            t, raw, x = [], [], []
            for s in range(K.SCENES):
                ids, depth = rows_of(oracle, pos[s], vel[s], width, (n, width, s))
                w1, b1, w2, b2 = P.unpack(pol[s if own else 0], features, hidden)
                xs = P.features_of_rows(ids, depth, features)
                x.append(xs)
                t.append(P.hidden_of(xs, w1, b1, "no_relu"))
                raw.append(P.outputs_of(P.hidden_of(xs, w1, b1), w2, b2, K.limit(n, width), "no_limit"))
            x, t, raw = np.stack(x), np.stack(t), np.stack(raw)
            what = (n, width, features, hidden, own)
            assert (x == 0).all(2).any() and (x > 0).any(2).any(), what
            assert (t > 0).any() and (t <= 0).any(), what
            assert (np.abs(raw) > K.limit(n, width)).any() and (np.abs(raw) <= K.limit(n, width)).any(), what
            _, _, p1, v1 = restated(oracle, n, width, features, hidden, own)
            assert (bits(v1) != bits(vel)).any() and (bits(p1) != bits((vel + pos).astype(F))).any(), what


ARMS = {"fma": lambda n, w, f, h: True, "reverse_f": lambda n, w, f, h: f > 1, "reverse_j": lambda n, w, f, h: h > 1,
        "max": lambda n, w, f, h: w // f > 1, "no_relu": lambda n, w, f, h: True, "no_limit": lambda n, w, f, h: True}


@pytest.mark.parametrize("arm", sorted(ARMS))
def test_control_arms_change_a_word(oracle, arm):
    """every case of 128 bodies and more that the arm can bear on (a reversed order needs two terms, a maximum two columns a bin):
    the departure from the rule changes a word of x, o or the state, with a policy per scene and with one for all.  (A scene of five
    bodies has too few seeing eyes to promise it; those cases are held to equality alone.)"""
    cases = [c for c in K.CASES if c[0] >= 128 and ARMS[arm](*c)]
    assert cases
    for n, width, features, hidden in cases:
        for own in (True, False):
            rule = restated(oracle, n, width, features, hidden, own)
            assert differs(restated(oracle, n, width, features, hidden, own, arm), rule), (arm, n, width, features, hidden, own)


def special_rows(oracle, width=64):
    pos, vel = K.special_scene()
    with np.errstate(all="ignore"):
        return pos, vel, rows_of(oracle, pos[0], vel[0], width)


def test_the_special_scene_tells_the_guard(oracle):
    """the zero-velocity body, the body moving along up and the body with a non-finite velocity coast under the rule and do not with
    P5's guard dropped (their accelerations are NaN); the other bodies see somebody and are pushed"""
    pos, vel, (ids, depth) = special_rows(oracle)
    pol = K.policies(8, 7, 1)
    rule = P.batch(lambda s, p, v: (ids, depth), pos, vel, pol, 8, 7, K.LIMIT, K.UP)
    arm = P.batch(lambda s, p, v: (ids, depth), pos, vel, pol, 8, 7, K.LIMIT, K.UP, variant="no_guard")
    with np.errstate(all="ignore"):
        coast = (vel + pos).astype(F)
    for body in (1, 2, 3):
        assert (bits(rule[3][0, body]) == bits(vel[0, body])).all()
        assert P.same(rule[2][0, body], coast[0, body])
        assert not P.same(arm[3][0, body], rule[3][0, body]), body
    for body in (0, 4, 5):
        assert (rule[0][0, body] > 0).any() and (bits(rule[3][0, body]) != bits(vel[0, body])).any(), body
    nan = pol.copy()
    nan[0, 3] = np.nan                                                 # a NaN weight of hidden unit 3: its h is +0 for every eye (P3)
    poisoned = P.batch(lambda s, p, v: (ids, depth), pos, vel, nan, 8, 7, K.LIMIT, K.UP)
    assert np.isfinite(poisoned[1]).all() and differs(poisoned[1:2], rule[1:2])
    nan = pol.copy()
    nan[0, 8 * 7 + 7 + 2] = np.nan                                     # a NaN in w2[0]: o_0 is NaN wherever h_2 is not skipped -- everywhere
    poisoned = P.batch(lambda s, p, v: (ids, depth), pos, vel, nan, 8, 7, K.LIMIT, K.UP)
    assert np.isnan(poisoned[1][0, :, 0]).all() and np.isfinite(poisoned[1][0, :, 1]).all()
    assert np.isnan(poisoned[3][0, 0]).any() and (bits(poisoned[3][0, 1]) == bits(vel[0, 1])).all()   # it passes the limit; a guarded body still coasts


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
    assert Fraction(float(f)) == q                                     # q is a binary32
    return int(bits(f).reshape(-1)[0])


def test_the_hand_case_in_exact_rationals(oracle):
    """DESIGN.md sections 12 and 13's two bodies under policy_cases.hand_policy(): eye 0 sees depth 0x3F63940C over columns 440 .. 583,
    inside bins 3 and 4 of 8 (columns 384 .. 639); x_3 = x_4 = 1 - d exactly, h = 2x, o = (2x, x), f = (1, 0, 0), s = (0, -1, 0);
    eye 1 sees nothing, its o is b2 = 0 and it coasts"""
    width, features, hidden = K.HAND_SHAPE
    ids, depth = rows_of(oracle, K.HAND_POS, K.HAND_VEL, width)
    seen = np.nonzero(ids[0] != R.NONE)[0]
    assert seen[0] == 440 and seen[-1] == 583 and len(seen) == 144 and (ids[0, seen] == 1).all() and (ids[1] == R.NONE).all()
    assert bits(depth[0, seen]).min() == K.HAND_DEPTH_BITS
    d = Fraction(float(np.uint32(K.HAND_DEPTH_BITS).view(F)))
    x = rn(1 - d)
    assert x == 1 - d                                                  # exact
    t = rn(rn(0 + rn(1 * x)) + rn(1 * x))                              # f = 3, 4; the other bins add w1 x = +0
    assert t == 2 * x
    o0, o1 = rn(0 + rn(1 * t)), rn(0 + rn(Fraction(1, 2) * t))
    assert (o0, o1) == (2 * x, x)
    dt = Fraction(float(F(0.1)))
    a = (rn(rn(o0 * 1) + rn(o1 * 0)), rn(rn(o0 * 0) + rn(o1 * -1)), rn(rn(o0 * 0) + rn(o1 * 0)))
    v = [rn(v0 + rn(ac * dt)) for v0, ac in zip((1, 0, 0), a)]
    p = [rn(vc + p0) for vc, p0 in zip(v, (0, 0, 0))]
    got_x, got_o, got_p, got_v = P.batch(lambda s, ps, vs: (ids, depth), K.HAND_POS[None], K.HAND_VEL[None], K.hand_policy()[None],
                                         features, hidden, np.inf, K.UP)
    assert [int(b) for b in bits(got_x[0, 0])] == [0, 0, 0, word(x), word(x), 0, 0, 0] and (bits(got_x[0, 1]) == 0).all()
    assert [int(b) for b in bits(got_o[0, 0])] == [word(o0), word(o1)] and (bits(got_o[0, 1]) == 0).all()
    assert [int(b) for b in bits(got_v[0, 0])] == [word(c) for c in v] and [int(b) for b in bits(got_p[0, 0])] == [word(c) for c in p]
    assert v[0] > 1 and v[1] < 0 and v[2] == 0                         # thrust ahead, a turn to -y
    assert (bits(got_v[0, 1]) == bits(K.HAND_VEL[1])).all() and (bits(got_p[0, 1]) == bits(F([11, 0, 0]))).all()
    limited = P.batch(lambda s, ps, vs: (ids, depth), K.HAND_POS[None], K.HAND_VEL[None], K.hand_policy()[None], features, hidden,
                      F(0.125), K.UP)
    assert 2 * x > Fraction(1, 8) > x and [int(b) for b in bits(limited[1][0, 0])] == [word(Fraction(1, 8)), word(o1)]


# -- the entries -------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nenbody_scenes_policy.h")).read(), flags=re.S)


def test_header_binding_and_library_agree(nb):
    from nenbody_amd import _lib

    header = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert sorted(re.findall(r"\b(nb_[a-z_0-9]+)\s*\(", header)) == sorted(NAMES) == sorted(_lib.SCENES_POLICY_PROTOTYPES)
    for name in NAMES:
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        assert len(_lib.SCENES_POLICY_PROTOTYPES[name][1]) == c_args and hasattr(lib, name) and hasattr(_lib.load(), name), name
        assert not name.startswith("nb_launch_")
    main = open(os.path.join(ROOT, "include", "nenbody.h")).read()
    assert '#include "nenbody_scenes_policy.h"' in main and int(re.search(r"#define NB_ABI_VERSION (\d+)", main).group(1)) == 2
    assert _lib.load().nb_abi_version() == 2
    rule = [main.index(" %s  " % p) for p in ("P1", "P2", "P3", "P4", "P5", "P6", "P7", "P8")]
    assert rule == sorted(rule) and main.index("SL5") < rule[0] and rule[-1] < main.index('#include "nenbody_scenes_policy.h"')
    assert main.index("#define NB_POLICY_MAX_FEATURES 256u") < main.index('#include "nenbody_scenes_policy.h"')
    assert main.index("#define NB_POLICY_MAX_HIDDEN 64u") < main.index('#include "nenbody_scenes_policy.h"')
    assert (_lib.NB_POLICY_MAX_FEATURES, _lib.NB_POLICY_MAX_HIDDEN) == (256, 64) == (P.MAX_FEATURES, P.MAX_HIDDEN)
    for method in ("set_policy", "step_policy", "policy_observe"):
        assert callable(getattr(nb.SceneBatch, method)), method


def test_policy_floats(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    for f, h in [(1, 1), (8, 1), (64, 32), (256, 64), (255, 63), (3, 7)]:
        assert lib.nb_policy_floats(f, h) == f * h + h + 2 * h + 2 == P.policy_floats(f, h) == nb.policy_floats(f, h)
    assert lib.nb_policy_floats(1, 1) == 6 and lib.nb_policy_floats(64, 32) == 2146 and lib.nb_policy_floats(256, 64) == 16578
    for f, h in [(0, 1), (1, 0), (257, 1), (1, 65), (0, 0), (0xFFFFFFFF, 0xFFFFFFFF)]:
        assert lib.nb_policy_floats(f, h) == 0 == P.policy_floats(f, h), (f, h)
    w1, b1, w2, b2 = np.arange(6, dtype=F).reshape(3, 2), F([10, 11]), F([[20, 21], [30, 31]]), F([40, 41])
    packed = nb.pack_policy(w1, b1, w2, b2)
    assert packed.dtype == F and packed.tolist() == [0, 1, 2, 3, 4, 5, 10, 11, 20, 21, 30, 31, 40, 41] == P.pack(w1, b1, w2, b2).tolist()
    assert packed[2 * 2 + 1] == w1[2, 1] and packed[6 + 1] == b1[1] and packed[8 + 1 * 2 + 0] == w2[1, 0]   # w1[f H + j], w2[k H + j]
    with pytest.raises(ValueError):
        nb.pack_policy(w1, b1, w2[:, :1], b2)


def test_the_rust_shim_and_the_cpp_host_declare_the_entry_points():
    text = open(os.path.join(ROOT, "integration", "rust", "scene.rs")).read()
    header = _header()
    for name in NAMES:
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        m = re.search(r"fn %s\s*\(([^)]*)\)" % name, text)
        assert m, name
        assert m.group(1).strip().rstrip(",").count(",") + 1 == c_args, name
    for item in ("pub fn set_policy(&mut self, weights: &[f32], features: u32, hidden: u32, accel_limit: f32)",
                 "pub fn step_policy(&mut self, k: u32, cp: &[[f32; 4]; 4], width: u32)", "pub fn policy_observe(&mut self, first_scene: u32"):
        assert item in text, item
    hpp = open(os.path.join(ROOT, "include", "nenbody_scene.hpp")).read()
    for item in ("void set_policy(const std::vector<float> &weights, uint32_t features, uint32_t hidden", "void step_policy(uint32_t k, const Mat4 &cp",
                 "PolicyObservation policy_observe(const Mat4 &cp"):
        assert item in hpp, item


def test_the_cpp_host_compiles(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "nenbody_scene.hpp"\n'
                   "void use(nenbody::SceneBatch &b, const nenbody::Mat4 &cp) {\n"
                   "    b.set_policy(std::vector<float>(nb_policy_floats(8, 4)), 8, 4, 0.5f);\n"
                   "    b.step_policy(2, cp, 64);\n"
                   "    (void)b.policy_observe(cp, 64).act.size();\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
