"""CPU tests of the scene batches' recurrent policy: the premises the GPU tests rest on, checked on the very
cases of tests/policy_recurrent_cases.py through the numpy restatements of the eye rule and of the rule R1-R8, with control arms; a
hand case in exact rationals; what memory means; the header, the binding, the library, the C++ host and the Rust shim agree on
the eleven entries.

A case runs with a policy per scene under S = MEMORY_LIMIT and with one policy for all under no memory limit
(policy_recurrent_cases.memory_limit).  Which runs a control arm must change a word on (of x, o, m', the positions or the velocities
of two steps):
  no_mem_limit, o_from_m          every case, under S: each has a unit above S after step 1
  stale                           every case, both runs: wr is not zero and m' is not m
  wr_hidden_major                 every case with H > 1, both runs (one word is its own transpose)
  mem_first, reverse_r, fma_mem   departures in rounding alone: every case of 128 bodies and more without a memory limit, which
                                  would hide the rounding of every unit above it; reverse_r with H > 1; mem_first with F > 1 or H > 1:
                                  with F = H = 1 the chain has three terms, and b1[0] = -2^-7 adds to either of the others exactly, so
                                  both orders round the exact sum once.  A scene of five bodies has too few seeing eyes to promise a
                                  changed rounding and is held to equality alone
  coast_keeps                     the special scene of policy_cases.py, the only one with coasting bodies"""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import es_restatement as E
import eyes_restatement as R
import located_restatement as L
import policy_recurrent_cases as C
import policy_recurrent_restatement as RR
import policy_restatement as P
from conftest import ROOT
from nenbody_amd._lib import SCENES_POLICY_RECURRENT_PROTOTYPES   # (the parent commit has no such table: the file fails here)

F = np.float32
NAMES = ["nb_policy_recurrent_floats", "nb_scenes_policy_recurrent_step_launch", "nb_scenes_policy_recurrent_observe_launch",
         "nb_scenes_es_perturb_floats_launch", "nb_scenes_es_update_floats_launch", "nb_scenes_set_policy_recurrent",
         "nb_scenes_eyes_policy_memory", "nb_scenes_memory_reset", "nb_scenes_memory", "nb_scenes_set_memory", "nb_scenes_es_set_recurrent"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rows_by(oracle, width):
    """rows_of for the restatements: the numpy eye rule on the oracle's cameras and matrices"""
    def rows_of(s, pos, vel):
        with np.errstate(all="ignore"):
            cams = oracle.cameras(pos, vel, C.UP, R.eye_constant(oracle, width))
            return R.eyes(cams, oracle.instances(pos, vel), 0, width, chunk=64)
    return rows_of


def rollout(oracle, case, own, steps=2, variant=None, zero_wr=False):
    n, width, features, hidden = case
    pos, vel = C.batch(oracle, C.row(n, width))
    pol = C.policies(features, hidden, C.SCENES if own else 1, zero_wr=zero_wr)
    mem = np.zeros((C.SCENES, n, hidden), F)
    return RR.rollout(rows_by(oracle, width), pos, vel, mem, pol, features, hidden, C.limit(n, width), C.memory_limit(own), C.UP, steps,
                      variant=variant)


def differs(a, b):
    return any((bits(g) != bits(w)).any() for sa, sb in zip(a, b) for g, w in zip(sa, sb))


# -- the premises ------------------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_what_the_issue_lists():
    assert sorted({c[0] for c in C.CASES}) == [5, 128, 129] and sorted({c[1] for c in C.CASES}) == [8, 64]
    assert sorted({c[2] for c in C.CASES}) == [1, 8] and sorted({c[3] for c in C.CASES}) == [1, 7, 64]
    assert C.SCENES == 3 and C.STEPS == 3 and len(C.CASES) == 36 and all(w % f == 0 for _, w, f, _ in C.CASES)
    assert 0 < C.MEMORY_LIMIT < np.inf


@pytest.mark.parametrize("n,width", [(n, w) for n in C.SIZES for w in C.WIDTHS])
def test_memory_is_written_read_and_limited_on_every_case(oracle, n, width):
    """every case, with a policy per scene and with one for all: after step 1 some memory word is non-zero; some word of step 2's o
    differs from the feedforward o of the same (w1, b1, w2, b2) on the same state; under the finite S one unit is clipped and one is
    not"""
    for case in [c for c in C.CASES if c[:2] == (n, width)]:
        _, _, features, hidden = case
        for own in (True, False):
            what = case + (own,)
            one, two = rollout(oracle, case, own)
            assert (bits(one[2]) != 0).any(), what
            pol = C.feedforward(C.policies(features, hidden, C.SCENES if own else 1), features, hidden)
            forward = P.batch(rows_by(oracle, width), one[3], one[4], pol, features, hidden, C.limit(n, width), C.UP)
            assert (bits(forward[0]) == bits(two[0])).all() and (bits(forward[1]) != bits(two[1])).any(), what
            if own:
                h = rollout(oracle, case, own, steps=1, variant="no_mem_limit")[0][2]
                assert (h > C.MEMORY_LIMIT).any() and (h <= C.MEMORY_LIMIT).any(), what
                assert ((one[2] == C.MEMORY_LIMIT) == (h >= C.MEMORY_LIMIT)).all() and one[2].max() == C.MEMORY_LIMIT and one[2].min() == 0, what
            else:
                assert one[2].max() > C.MEMORY_LIMIT, what


ARMS = {"no_mem_limit": lambda n, w, f, h, own: own, "o_from_m": lambda n, w, f, h, own: own, "stale": lambda n, w, f, h, own: True,
        "wr_hidden_major": lambda n, w, f, h, own: h > 1, "mem_first": lambda n, w, f, h, own: n >= 128 and not own and (f > 1 or h > 1),
        "reverse_r": lambda n, w, f, h, own: n >= 128 and not own and h > 1, "fma_mem": lambda n, w, f, h, own: n >= 128 and not own}


@pytest.mark.parametrize("arm", sorted(ARMS))
def test_control_arms_change_a_word(oracle, arm):
    """every run the arm can bear on (the docstring of this file)"""
    runs = [(c, own) for c in C.CASES for own in (True, False) if ARMS[arm](*c, own)]
    assert runs
    for case, own in runs:
        assert differs(rollout(oracle, case, own, variant=arm), rollout(oracle, case, own)), (arm, case, own)


def test_every_arm_is_exercised():
    assert sorted(list(ARMS) + ["coast_keeps"]) == sorted(RR.VARIANTS)


def test_the_special_scene_has_a_coasting_body_whose_memory_changes(oracle):
    """the zero-velocity body, the body moving along up and the body with a non-finite velocity coast under P5 and still take their
    new memory (R5); the arm that leaves a coasting body's memory alone is told from the rule"""
    pos, vel = C.special_scene()
    pol = C.policies(8, 7, 1)
    mem = np.zeros((1, 6, 7), F)
    args = (rows_by(oracle, 64), pos, vel, mem, pol, 8, 7, C.LIMIT, C.MEMORY_LIMIT, C.UP)
    rule, arm = RR.batch(*args), RR.batch(*args, variant="coast_keeps")
    for body in (1, 2, 3):
        assert (bits(rule[4][0, body]) == bits(vel[0, body])).all(), body                 # it coasts
        assert (bits(rule[2][0, body]) != 0).any() and (bits(arm[2][0, body]) == 0).all(), body
    for body in (0, 4, 5):
        assert (bits(rule[4][0, body]) != bits(vel[0, body])).any() and (bits(rule[2][0, body]) == bits(arm[2][0, body])).all(), body


# -- R6 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,width", [(n, w) for n in C.SIZES for w in C.WIDTHS])
def test_a_zero_wr_is_the_feedforward_policy(oracle, n, width):
    """every case: with every word of wr +0 the positions, the velocities, x and o of three steps are policy_restatement's for
    (w1, b1, w2, b2), bit for bit, while the memory is written all the same"""
    for case in [c for c in C.CASES if c[:2] == (n, width)]:
        _, _, features, hidden = case
        for own in (True, False):
            steps = rollout(oracle, case, own, steps=C.STEPS, zero_wr=True)
            pol = C.feedforward(C.policies(features, hidden, C.SCENES if own else 1, zero_wr=True), features, hidden)
            pos, vel = C.batch(oracle, C.row(n, width))
            for got in steps:
                want = P.batch(rows_by(oracle, width), pos, vel, pol, features, hidden, C.limit(n, width), C.UP)
                for g, w in zip((got[0], got[1], got[3], got[4]), want):
                    assert (bits(g) == bits(w)).all(), case + (own,)
                pos, vel = want[2], want[3]
            assert (bits(steps[-1][2]) != 0).any()
    t = F([-0.0, 1.5, -2.0])                                           # why: t + (+0 * m) leaves every t but -0 alone, and -0 gives +0 as +0 does
    for m in F([3.0, -3.0, 0.0]):
        u = t + F(0) * m
        assert (bits(u[1:]) == bits(t[1:])).all() and bits(np.where(u > 0, u, F(0)))[0] == bits(np.where(t > 0, t, F(0)))[0] == 0


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
    """DESIGN.md section 12's two bodies under policy_recurrent_cases.hand_policy(), F = 8, H = 2, S = 1/8, two steps.  Eye 0 sees body
    1 inside bins 3 and 4; eye 1 sees nothing.  Step 1: t_0 = x_3 + x_4 > S, so m'_0 = S while o_0 = h_0 (R5: o from h); t_1 = 0.
    Step 2: t_0 = (x_3 + x_4) + S/2, t_1 = S/4: unit 1 is on from memory alone"""
    width, features, hidden = C.HAND_SHAPE
    s_lim = Fraction(float(C.HAND_MEMORY_LIMIT))
    dt = Fraction(float(F(0.1)))
    pos, vel, mem = [[Fraction(0)] * 3, [Fraction(10), Fraction(0), Fraction(0)]], [Fraction(1), Fraction(0), Fraction(0)], [Fraction(0)] * 2
    state_p, state_v = P.F32([[0, 0, 0], [10, 0, 0]]), P.F32([[1, 0, 0], [1, 0, 0]])
    got = RR.rollout(rows_by(oracle, width), state_p[None], state_v[None], np.zeros((1, 2, 2), F), C.hand_policy()[None], features, hidden,
                     np.inf, C.HAND_MEMORY_LIMIT, C.UP, 2)
    for step in range(2):
        ids, depth = rows_by(oracle, width)(0, state_p, state_v)
        seen = np.nonzero(ids[0] != R.NONE)[0]
        assert 384 <= seen[0] and seen[-1] < 640 and (seen < 512).any() and (seen >= 512).any() and (ids[1] == R.NONE).all()
        x = []
        for lo in (384, 512):                                          # bins 3 and 4
            cols = seen[(seen >= lo) & (seen < lo + 128)]
            d = Fraction(float(bits(depth[0, cols]).min().view(F)))
            x.append(rn(1 - d))
            assert x[-1] == 1 - d                                      # exact
        f_axis, s_axis = L.axes(state_v, C.UP)
        assert f_axis.tolist() == [[1, 0, 0]] * 2 and s_axis.tolist() == [[0, -1, 0]] * 2
        t0 = rn(rn(rn(0 + rn(1 * x[0])) + rn(1 * x[1])) + rn(Fraction(1, 2) * mem[0]))   # the other bins add +0, and wr[1, 0] m_1 is +0
        t1 = rn(0 + rn(Fraction(1, 4) * mem[0]))
        h = [t0 if t0 > 0 else Fraction(0), t1 if t1 > 0 else Fraction(0)]
        assert h[0] > s_lim and h[1] < s_lim and (h[1] > 0) == (step == 1)
        mem = [min(c, s_lim) for c in h]
        o = [rn(0 + rn(1 * h[0])), rn(0 + rn(1 * h[1]))]                                 # b2 = 0; w2 is the identity; the other term is +0
        a = (rn(rn(o[0] * 1) + rn(o[1] * 0)), rn(rn(o[0] * 0) + rn(o[1] * -1)), Fraction(0))
        vel = [rn(v0 + rn(ac * dt)) for v0, ac in zip(vel, a)]
        pos[0] = [rn(vc + p0) for vc, p0 in zip(vel, pos[0])]
        pos[1] = [rn(pos[1][0] + 1), Fraction(0), Fraction(0)]
        gx, go, gm, gp, gv = got[step]
        assert [int(b) for b in bits(gx[0, 0])] == [0, 0, 0, word(x[0]), word(x[1]), 0, 0, 0] and (bits(gx[0, 1]) == 0).all()
        assert [int(b) for b in bits(go[0, 0])] == [word(c) for c in o] and (bits(go[0, 1]) == 0).all()
        assert [int(b) for b in bits(gm[0, 0])] == [word(c) for c in mem] and (bits(gm[0, 1]) == 0).all()
        assert [int(b) for b in bits(gv[0, 0])] == [word(c) for c in vel] and [int(b) for b in bits(gp[0, 0])] == [word(c) for c in pos[0]]
        assert [int(b) for b in bits(gp[0, 1])] == [word(c) for c in pos[1]] and (bits(gv[0, 1]) == bits(F([1, 0, 0]))).all()
        if step == 1:
            assert word(mem[1]) == word(Fraction(1, 32)) and vel[1] < 0       # the turn of step 2 comes from memory alone
        else:
            assert word(mem[0]) == word(Fraction(1, 8)) and vel[1] == 0 and vel[0] > 1
        state_p, state_v = gp[0], gv[0]


# -- what memory MEANS -----------------------------------------------------------------------------------------------------------------------
def meaning_rollout(oracle):
    width, features, hidden = C.MEANING_SHAPE
    rows_of = rows_by(oracle, width)
    steps = RR.rollout(rows_of, C.MEANING_POS[None], C.MEANING_VEL[None], np.zeros((1, 2, 1), F), C.meaning_policy()[None], features, hidden,
                       np.inf, F(1), C.UP, C.MEANING_STEPS)
    forward = RR.feedforward(C.meaning_policy(), features, hidden)
    w1, b1, _, _ = P.unpack(forward, features, hidden)
    h_forward = [P.hidden_of(s[0][0], w1, b1)[0, 0] for s in steps]    # eye 0's feedforward h_0 on the same snapshots
    return steps, h_forward


def meaning_phases(steps):
    """per step whether eye 0's row shows anybody; the steps before, during and after the crossing"""
    seen = [bool((s[0][0, 0] > 0).any()) for s in steps]
    first, last = seen.index(True), len(seen) - 1 - seen[::-1].index(True)
    assert 0 < first <= last < len(seen) - 2 and all(seen[first:last + 1]), seen     # one crossing, with steps before and at least two after
    return seen, first, last


def test_memory_means_that_a_body_remembers_whom_it_saw(oracle):
    """Two bodies in straight lines (w2 = b2 = 0); body 1 crosses eye 0's slit and leaves it.  m_0 of body 0 is +0 before the crossing,
    1.0 during it and still 1.0 on every step after the row is empty again, where the feedforward h_0 is back at +0"""
    steps, h_forward = meaning_rollout(oracle)
    seen, first, last = meaning_phases(steps)
    for t, s in enumerate(steps):
        m0 = s[2][0, 0, 0]
        want_p = (C.MEANING_POS + F(t + 1) * C.MEANING_VEL).astype(F)                                    # p = v + p, exact here
        assert (bits(s[3][0]) == bits(want_p)).all() and (bits(s[4][0]) == bits(C.MEANING_VEL)).all()     # straight lines
        assert bits(m0) == (0 if t < first else bits(F(1))), (t, seen)
        assert (h_forward[t] > 1) == seen[t] and (seen[t] or bits(h_forward[t]) == 0), (t, seen)
    assert (bits(steps[-1][2][0, 1]) == 0).all()                       # eye 1 never sees body 0


# -- the search ------------------------------------------------------------------------------------------------------------------------------
def test_a_longer_mean_draws_the_same_leading_words():
    """E8 over M: es_restatement at M = policy_recurrent_floats(8, 7) gives the words below policy_floats(8, 7) that it gives at that
    smaller M, for the population and for the update"""
    small, large = P.policy_floats(8, 7), RR.policy_recurrent_floats(8, 7)
    assert (small, large) == (79, 128)
    mean = np.random.default_rng(3).uniform(-1, 1, large).astype(F)
    for g in (0, 5):
        a = E.population(mean[:small], F(0.05), 1234, g, 0, 5)
        b = E.population(mean, F(0.05), 1234, g, 0, 5)
        assert (bits(a) == bits(b[:, :small])).all() and len({tuple(r) for r in bits(b).tolist()}) == 5
        r = np.array([3, 0, 4, 1, 2], np.uint32)
        assert (bits(E.update(mean[:small], F(3e-5), 1234, g, r)) == bits(E.update(mean, F(3e-5), 1234, g, r)[:small])).all()


# -- the entries -------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nenbody_scenes_policy_recurrent.h")).read(), flags=re.S)


def test_header_binding_and_library_agree(nb):
    from nenbody_amd import _lib

    header = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert sorted(re.findall(r"\b(nb_[a-z_0-9]+)\s*\(", header)) == sorted(NAMES) == sorted(SCENES_POLICY_RECURRENT_PROTOTYPES)
    for name in NAMES:
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        assert len(SCENES_POLICY_RECURRENT_PROTOTYPES[name][1]) == c_args and hasattr(lib, name) and hasattr(_lib.load(), name), name
        assert not name.startswith("nb_launch_")
    main = open(os.path.join(ROOT, "include", "nenbody.h")).read()
    include = main.index('#include "nenbody_scenes_policy_recurrent.h"')
    assert int(re.search(r"#define NB_ABI_VERSION (\d+)", main).group(1)) == 2 and _lib.load().nb_abi_version() == 2
    rule = [main.index(" %s  " % r) for r in ("R1", "R2", "R3", "R4", "R5", "R6", "R7", "R8")]
    assert rule == sorted(rule) and main.index(" P8  ") < rule[0] and rule[-1] < include
    assert main.index("#define NB_ES_MAX_FLOATS 20674u") < include and _lib.NB_ES_MAX_FLOATS == 20674 == RR.policy_recurrent_floats(256, 64)
    for phrase in ("do NOT touch the memory", "nb_scenes_upload does not", "leave the memory alone"):
        assert phrase in main[rule[-1]:include], phrase                # the decisions
    for method in ("set_policy_recurrent", "memory", "set_memory", "memory_reset", "policy_observe_memory", "es_set_recurrent"):
        assert callable(getattr(nb.SceneBatch, method)), method


def test_policy_recurrent_floats(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    for f, h in [(1, 1), (8, 1), (8, 7), (64, 32), (256, 64), (255, 63), (3, 7)]:
        want = f * h + h * h + h + 2 * h + 2
        assert lib.nb_policy_recurrent_floats(f, h) == want == RR.policy_recurrent_floats(f, h) == nb.policy_recurrent_floats(f, h)
        assert want == lib.nb_policy_floats(f, h) + h * h
    assert lib.nb_policy_recurrent_floats(256, 64) == 20674 and lib.nb_policy_recurrent_floats(64, 32) == 3170
    for f, h in [(0, 1), (1, 0), (257, 1), (1, 65), (0, 0), (0xFFFFFFFF, 0xFFFFFFFF)]:
        assert lib.nb_policy_recurrent_floats(f, h) == 0 == RR.policy_recurrent_floats(f, h), (f, h)
    w1, wr, b1 = np.arange(6, dtype=F).reshape(3, 2), F([[50, 51], [52, 53]]), F([10, 11])
    w2, b2 = F([[20, 21], [30, 31]]), F([40, 41])
    packed = nb.pack_policy_recurrent(w1, wr, b1, w2, b2)
    assert packed.dtype == F and packed.tolist() == [0, 1, 2, 3, 4, 5, 50, 51, 52, 53, 10, 11, 20, 21, 30, 31, 40, 41]
    assert packed.tolist() == RR.pack(w1, wr, b1, w2, b2).tolist()
    assert packed[6 + 1 * 2 + 0] == wr[1, 0]                           # wr[r H + j]: source-major
    assert RR.feedforward(packed, 3, 2).tolist() == nb.pack_policy(w1, b1, w2, b2).tolist()
    with pytest.raises(ValueError):
        nb.pack_policy_recurrent(w1, wr[:1], b1, w2, b2)


def test_the_rust_shim_and_the_cpp_host_declare_the_entry_points():
    text = open(os.path.join(ROOT, "integration", "rust", "scene.rs")).read()
    header = _header()
    for name in NAMES:
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        m = re.search(r"fn %s\s*\(([^)]*)\)" % name, text)
        assert m, name
        assert m.group(1).strip().rstrip(",").count(",") + 1 == c_args, name
    for item in ("pub fn set_policy_recurrent(&mut self, weights: &[f32], features: u32, hidden: u32, accel_limit: f32, memory_limit: f32)",
                 "pub fn memory(&mut self", "pub fn set_memory(&mut self, memory: &[f32])", "pub fn memory_reset(&mut self)",
                 "pub fn policy_observe_memory(&mut self, first_scene: u32", "pub fn es_set_recurrent(&mut self"):
        assert item in text, item
    hpp = open(os.path.join(ROOT, "include", "nenbody_scene.hpp")).read()
    for item in ("void set_policy_recurrent(const std::vector<float> &weights, uint32_t features, uint32_t hidden", "std::vector<float> memory(",
                 "void set_memory(const std::vector<float> &memory)", "void memory_reset()", "PolicyMemoryObservation policy_observe_memory(const Mat4 &cp",
                 "void es_set_recurrent(const std::vector<float> &mean"):
        assert item in hpp, item


def test_the_cpp_host_compiles(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "nenbody_scene.hpp"\n'
                   "void use(nenbody::SceneBatch &b, const nenbody::Mat4 &cp, const nb_es_params &ep) {\n"
                   "    b.set_policy_recurrent(std::vector<float>(nb_policy_recurrent_floats(8, 4)), 8, 4, 0.5f, 1.0f);\n"
                   "    b.step_policy(2, cp, 64);\n"
                   "    b.set_memory(b.memory());\n"
                   "    b.memory_reset();\n"
                   "    (void)b.policy_observe_memory(cp, 64).mem.size();\n"
                   "    b.es_set_recurrent(std::vector<float>(nb_policy_recurrent_floats(8, 4)), 8, 4, ep, 0.5f, 1.0f);\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
