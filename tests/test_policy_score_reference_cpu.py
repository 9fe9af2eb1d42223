"""Premises of the binary64 references of the scene batches' policy and score (tests/policy_reference.py, tests/score_reference.py),
no device: the cases of tests/policy_reference_cases.py meet their caps on the references alone; the numpy restatements of DESIGN.md
sections 14.4 and 14.5 lie within the references on every case; the bounds are tight enough to matter -- every control arm, a
mutated copy of a restatement that changes what the rule MEANS, is rejected on every fixed case where it can bear, and for the
reason it is about -- and loose enough to be bounds: the arms that only move roundings are accepted; two hand cases in exact rationals.

Largest error / bound of the restatements (test_the_ratios_over_all_cases prints them; run with -s): the figures of the two
reference modules' docstrings."""
import math
from fractions import Fraction

import numpy as np
import pytest

import policy_reference as PR
import policy_reference_cases as C
import policy_restatement as P
import score_cases as SK
import score_reference as QR
import score_restatement as Q
from test_vision_reference_cpu import mutant

F32 = np.float32
INF = float("inf")


# -- 1. the caps, on the references alone -----------------------------------------------------------------------------------------------
def eyes_of(ref, name):
    return np.concatenate([getattr(r, name) for r in ref])


def test_the_case_list_holds_the_shapes_it_promises():
    cs = list(C.FIXED.values())
    assert 14 <= len(cs) <= 18 and all(c["n"] <= 129 and c["batch"] <= 4 or (c["n"], c["eyes"], c["batch"]) == (257, 48, 1) for c in cs)
    assert {c["kind"] for c in cs} == {"planar", "3-D", "lifted", "clustered"}
    assert {c["scale"] for c in cs if c["kind"] == "3-D"} == {3.0, 10.0}
    assert any(c["zeros"] for c in cs) and any(c["along"] for c in cs)
    assert {c["up"] for c in cs} == {C.UP, C.TILTED} and {c["lens"] for c in cs} == set(C.LENSES)
    assert {c["width"] for c in cs} == {7, 63, 64, 65, 200, 256, 1024} and {c["hidden"] for c in cs} == set(C.HIDDEN)
    shapes = {(c["width"], c["features"]) for c in cs}
    assert {(63, 9), (200, 25), (65, 5)} <= shapes and {w for w, f in shapes if f == 1} and {w for w, f in shapes if w == f} >= {7, 64, 256}
    assert {c["own"] for c in cs} == {True, False} and {c["limit"] for c in cs} == set(C.LIMITS)
    assert sum(c["weights"] == (2.0 ** -130,) * 3 for c in cs) == 1 and [n for n, c in C.FIXED.items() if c["exempt"]] == ["lifted3_n100_w65_f5_h2_weights_2p10"]
    assert C.FIXED["lifted3_n100_w65_f5_h2_weights_2p10"]["weights"] == (2.0 ** 10,) * 3
    assert {c["n"] for c in cs} >= {127, 128, 129} and any(c["n"] > 128 for c in cs) and any(c["n"] <= 128 for c in cs)
    assert not any(c["along"] and c["up"] != C.UP for c in cs)        # (policy_reference's docstring: along (0, 0, 1) no heading is undecided)


@pytest.mark.parametrize("name", list(C.FIXED))
def test_the_policy_caps_hold_on_the_reference_alone(name):
    c = C.fixed(name)
    ref = C.reference(c)
    seeing, compared, blind = eyes_of(ref, "seeing"), eyes_of(ref, "compared"), eyes_of(ref, "blind")
    on, off, free, held = (eyes_of(ref, a) & compared for a in ("on", "off", "free", "held"))
    o = np.concatenate([r.o for r in ref])
    print(f"\n{name}: {len(seeing)} eyes, {int(seeing.sum())} see somebody, {int((seeing & ~compared).sum())} of them not compared "
          f"({100.0 * (seeing & ~compared).sum() / max(seeing.sum(), 1):.2f} %), {int(blind.sum())} blind; compared eyes with a unit surely on "
          f"{int(on.sum())}, off {int(off.sum())}, an output inside the limit {int(free.sum())}, at it {int(held.sum())}; largest |o| {np.abs(o).max():.3g}; "
          f"headings none / undecided {int((eyes_of(ref, 'heading') == 0).sum())} / {int((eyes_of(ref, 'heading') < 0).sum())}")
    assert (seeing & ~compared).sum() <= C.CAPS["uncompared_share"] * seeing.sum(), name
    assert (seeing & compared).sum() >= C.CAPS["compared_seeing"], name
    assert np.abs(o).max() <= 1.0 and not (eyes_of(ref, "heading") < 0).any(), name
    assert (blind & ~compared).sum() == 0                                      # an eye that sees nothing has nothing undecided
    if c["n"] >= 64 and not c["exempt"]:
        assert blind.any() and on.any() and off.any() and free.any() and held.any(), name
    if c["zeros"] or c["along"]:
        assert (eyes_of(ref, "heading") == 0).sum() >= c["batch"] * ((c["n"] // 8 if c["zeros"] else 0) + (1 if c["along"] else 0)) - c["batch"] * (c["n"] - c["eyes"])
    if c["exempt"]:
        assert (held | ~seeing).all(), name                                    # weights x 2^10: every seeing eye is clipped
    if c["weights"][0] < 1:
        t = [PR.network(r.x, r.dx, c["policies"][s if c["own"] else 0], c["features"], c["hidden"], c["limit"])[2] for s, r in enumerate(ref)]
        assert max(np.abs(a).max() for a in t) < 2.0 ** -126, name            # every hidden sum is subnormal


@pytest.mark.parametrize("kind", SK.KINDS)
def test_the_score_caps_hold_on_the_reference_alone(kind):
    for n in C.SCORE_SIZES:
        ref = C.score_reference(kind, n)
        print(f"\n{kind} n={n}: maybe pairs per scene {[r.maybe for r in ref]} of {ref[0].pairs}, nonfinite {[r.nonfinite for r in ref]}")
        for r in ref:
            assert r.maybe <= max(C.CAPS["maybe_pairs"], C.CAPS["maybe_share"] * r.pairs), (kind, n, r.maybe)
            if kind == "lattice":
                assert r.maybe == 0, (kind, n, r.maybe)                        # every step of every d2 is exact
    if kind == "lattice":                                                      # and pairs do tie with the radius there
        pos, _, radius_sq, _ = SK.make(kind, 129)
        d2 = np.concatenate([Q.pair_d2(p)[np.triu_indices(129, 1)] for p in pos])
        assert (d2 == radius_sq).sum() >= 100


# -- 2. the restatements lie within the references ---------------------------------------------------------------------------------------
_ratios = {}


def policy_ratios(oracle, c):
    if c["name"] not in _ratios:
        x, o, states = C.restated(oracle, c)
        _ratios[c["name"]] = PR.compare(c["name"], C.reference(c), x, o, *states[0])
    return _ratios[c["name"]]


@pytest.mark.parametrize("name", list(C.FIXED))
def test_the_policy_restatement_lies_within_the_reference(oracle, name):
    r = policy_ratios(oracle, C.fixed(name))
    print(f"\n{name}: error / bound " + " ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values())


@pytest.mark.parametrize("i", range(C.RANDOM_CASES))
def test_the_policy_restatement_lies_within_the_reference_on_random_problems(oracle, i):
    c = C.case(i)
    print("\n" + c["line"])
    r = policy_ratios(oracle, c)
    print("error / bound " + " ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), c["line"]


def score_ratios(kind, n):
    if ("score", kind, n) not in _ratios:
        pos, vel, radius_sq, goal = SK.make(kind, n)
        one = QR.compare(f"{kind} n={n}", C.score_reference(kind, n), SK.want(kind, n))
        two = QR.compare(f"{kind} n={n}, two snapshots", QR.batch(pos, vel, radius_sq, goal, acc=C.score_reference(kind, n)),
                         Q.batch(pos, vel, radius_sq, goal, acc=SK.want(kind, n)))
        _ratios["score", kind, n] = dict(one, **{"two " + k: v for k, v in two.items()})
    return _ratios["score", kind, n]


@pytest.mark.parametrize("kind", SK.KINDS)
def test_the_score_restatement_lies_within_the_reference(kind):
    for n in C.SCORE_SIZES:
        r = score_ratios(kind, n)
        print(f"\n{kind} n={n}: error / bound " + " ".join(f"{k} {v:.4f}" for k, v in r.items()))
        assert all(v <= 1.0 for v in r.values())


def test_the_ratios_over_all_cases(oracle):
    """the largest error / bound per output: the figures of the two reference modules' docstrings and of DESIGN.md sections 14.4, 14.5"""
    worst = {}
    for c in [C.fixed(name) for name in C.FIXED] + [C.case(i) for i in range(C.RANDOM_CASES)]:
        for k, v in policy_ratios(oracle, c).items():
            worst["policy", k] = max(worst.get(("policy", k), 0.0), v)
    for kind, n in C.SCORE_CASES:
        for k, v in score_ratios(kind, n).items():
            worst["score", k] = max(worst.get(("score", k), 0.0), v)
    print("\nlargest error / bound: " + "; ".join(f"{a} {k} {v:.4f}" for (a, k), v in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values())
    assert sum(PR.ROUNDINGS.values()) == 19


# -- 3. control arms ---------------------------------------------------------------------------------------------------------------------------
def policy_rejected(oracle, c, word, **how):
    """PR.compare refuses the arm's result, and names the word the arm is about"""
    x, o, states = C.restated(oracle, c, **how)
    with pytest.raises(AssertionError) as failure:
        PR.compare(c["name"], C.reference(c), x, o, *states[0])
    message = str(failure.value)
    print(f"\nrejected: {message}")
    assert f", {word}[" in message and "shape" not in message, message


def acts(c):
    """the outputs move a body: not where the limit is 0, nor where every weight is scaled by 2^-130 (o below 2^-130 leaves v alone)"""
    return c["limit"] > 0 and c["weights"][1] >= 1


def has_held(c):
    return any((r.held & r.compared).any() for r in C.reference(c))


X_IS_D = [("return (F32(1) - d.astype(np.uint32).view(F32)).astype(F32)", "return d.astype(np.uint32).view(F32)")]
MIRRORED = [("return (F32(1) - d.astype(np.uint32).view(F32)).astype(F32)", "return (F32(1) - d.astype(np.uint32).view(F32)).astype(F32)[:, ::-1]")]
HIDDEN_MAJOR = [("return w1.reshape(features, hidden), b1, w2.reshape(2, hidden), b2", "return w1.reshape(hidden, features).T, b1, w2.reshape(2, hidden), b2")]
W2_SWAPPED = [("return w1.reshape(features, hidden), b1, w2.reshape(2, hidden), b2", "return w1.reshape(features, hidden), b1, w2.reshape(2, hidden)[::-1], b2")]
O_SWAPPED = [("a = (o[:, 0, None] * f) + (o[:, 1, None] * s)", "a = (o[:, 1, None] * f) + (o[:, 0, None] * s)")]
S_NEGATED = [("a = (o[:, 0, None] * f) + (o[:, 1, None] * s)", "a = (o[:, 0, None] * f) + (o[:, 1, None] * -s)")]
NO_DT = [("v = vel + a * F32(dt)", "v = vel + a")]
OLD_VELOCITY = [("p = v + pos", "p = vel + pos")]
# arm: (the word that tells it, how the restatement is run, the fixed cases it can bear on).  Where the limit is 0 every output is 0
# whatever the network says, and under weights x 2^-130 the second layer's products vanish: the network's arms bear on neither; under
# weights x 2^10 every output is +-limit and only its sign is left, which an arm need not move.
POLICY_ARMS = {
    "bins mirrored": ("x", dict(module=MIRRORED), lambda c: c["features"] > 1),
    "farthest instead of nearest": ("x", dict(variant="max"), lambda c: c["width"] // c["features"] > 1),
    "x = d": ("x", dict(module=X_IS_D), lambda c: True),
    "see_self": ("x", dict(see_self=True), lambda c: c["lens"][0] < 1.0),
    "w1 read hidden-major": ("o", dict(module=HIDDEN_MAJOR), lambda c: c["features"] > 1 and c["hidden"] > 1 and acts(c) and not c["exempt"]),
    "rows of w2 swapped": ("o", dict(module=W2_SWAPPED), lambda c: acts(c) and not c["exempt"]),
    "no ReLU": ("o", dict(variant="no_relu"), lambda c: acts(c) and not c["exempt"]),
    "no limit": ("o", dict(variant="no_limit"), lambda c: c["limit"] < INF and (has_held(c) or c["limit"] == 0)),
    "o_0 and o_1 swapped": ("vel", dict(module=O_SWAPPED), lambda c: acts(c) and not c["exempt"]),
    "s negated": ("vel", dict(module=S_NEGATED), acts),
    "dt left out": ("vel", dict(module=NO_DT), acts),
    "p' = p + v": ("pos", dict(module=OLD_VELOCITY), acts),
}


@pytest.mark.parametrize("arm", list(POLICY_ARMS))
def test_policy_arm_is_rejected_on_every_fixed_case_it_can_bear_on(oracle, arm):
    word, how, bears = POLICY_ARMS[arm]
    how = dict(how, module=mutant(P, how["module"])) if "module" in how else how
    names = [name for name in C.FIXED if bears(C.fixed(name))]
    print(f"\n{arm}: {len(names)} of {len(C.FIXED)} cases")
    assert len(names) >= 2
    for name in names:
        policy_rejected(oracle, C.fixed(name), word, **how)


@pytest.mark.parametrize("variant", ["fma", "reverse_f", "reverse_j"])
def test_policy_arms_that_only_move_roundings_are_accepted(oracle, variant):
    """a bound tuned down to the restatement would refuse these"""
    moved = 0
    for name in C.FIXED:
        c = C.fixed(name)
        x, o, states = C.restated(oracle, c, variant=variant)
        PR.compare(f"{name} ({variant})", C.reference(c), x, o, *states[0])
        moved += not P.same(o, C.restated(oracle, c)[1])
    assert moved >= len(C.FIXED) // 2, moved                                   # and they do move words


def score_rejected(kind, n, field, got, ref=None):
    with pytest.raises(AssertionError) as failure:
        QR.compare(f"{kind} n={n}", C.score_reference(kind, n) if ref is None else ref, got)
    message = str(failure.value)
    print(f"\nrejected: {message}")
    assert f", {field}: " in message, message


SPREAD_ORIGIN = [('out["spread"] = tree(dist2(p, c.astype(F32), form), order)', 'out["spread"] = tree(dist2(p, np.zeros(3, F32), form), order)')]
SPREAD_GOAL = [('out["spread"] = tree(dist2(p, c.astype(F32), form), order)', 'out["spread"] = tree(dist2(p, goal, form), order)')]
MOMENTUM_SPEED = [('out["momentum2"] = ((t[4] * t[4]) + (t[5] * t[5])) + (t[6] * t[6])', 'out["momentum2"] = t[3]')]
GOAL_PLUS = [("v, dist2(p, goal, form)[:, None]], 1)", "v, dist2(p, -goal, form)[:, None]], 1)")]
REPLACED = [("out[f] = F32(acc[f]) + F32(term[f])", "out[f] = F32(term[f])")]
SCORE_ARMS = {"spread about the origin": ("spread", SPREAD_ORIGIN), "spread about the goal": ("spread", SPREAD_GOAL),
              "momentum2 as the sum of |v|^2": ("momentum2", MOMENTUM_SPEED), "goal2 with p + goal": ("goal2", GOAL_PLUS)}


@pytest.mark.parametrize("arm", list(SCORE_ARMS))
def test_score_arm_is_rejected_on_every_case(arm):
    """n >= 2, every kind: the nonfinite kind through the scene whose outliers leave the arm's field finite"""
    field, edits = SCORE_ARMS[arm]
    m = mutant(Q, edits)
    for kind, n in C.SCORE_CASES:
        pos, vel, radius_sq, goal = SK.make(kind, n)
        score_rejected(kind, n, field, m.batch(pos, vel, radius_sq, goal))


def test_score_arm_le_is_rejected_where_pairs_tie_exactly_and_ordered_pairs_wherever_a_pair_is_near():
    told = 0
    for kind, n in C.SCORE_CASES:
        pos, vel, radius_sq, goal = SK.make(kind, n)
        ref = C.score_reference(kind, n)
        exact_tie = False                       # a pair whose binary64 d2 IS the radius: only exact steps give that
        for p in pos:
            i, j = np.nonzero(np.triu(Q.pair_d2(p) == radius_sq, 1))
            with np.errstate(all="ignore"):
                exact_tie |= bool((((p[i].astype(np.float64) - p[j].astype(np.float64)) ** 2).sum(1) == float(radius_sq)).any())
        assert exact_tie or kind != "lattice"
        if exact_tie:
            score_rejected(kind, n, "near", Q.batch(pos, vel, radius_sq, goal, variant="le"))
        else:                                                                  # elsewhere the tying pair is within its bound of the radius: maybe
            QR.compare(f"{kind} n={n} (le)", ref, Q.batch(pos, vel, radius_sq, goal, variant="le"))
        if any(2 * r.near_lo > r.near_hi for r in ref):
            score_rejected(kind, n, "near", Q.batch(pos, vel, radius_sq, goal, variant="ordered"))
            told += 1
    assert told >= len(C.SCORE_CASES) - len(SK.KINDS)                          # all but, at most, the three pairs of n = 2


def test_score_arm_a_snapshot_replacing_the_record_is_rejected():
    m = mutant(Q, REPLACED)
    for kind, n in C.SCORE_CASES:
        pos, vel, radius_sq, goal = SK.make(kind, n)
        ref = QR.batch(pos, vel, radius_sq, goal, acc=C.score_reference(kind, n))
        got = m.batch(pos, vel, radius_sq, goal, acc=SK.want(kind, n))
        score_rejected(kind, n, "speed2" if kind == "nonfinite" else "spread", got, ref)      # (the first float field that is held)


@pytest.mark.parametrize("variant", ["adjacent", "float64", "fma", "recip", "skip_padding", "workgroup"])
def test_score_arms_that_only_move_roundings_are_accepted(variant):
    moved = 0
    for kind, n in C.SCORE_CASES:
        pos, vel, radius_sq, goal = SK.make(kind, n)
        got = Q.batch(pos, vel, radius_sq, goal, variant=variant)
        QR.compare(f"{kind} n={n} ({variant})", C.score_reference(kind, n), got)
        moved += not Q.same(got, SK.want(kind, n))
    print(f"\n{variant}: moves a word on {moved} of {len(C.SCORE_CASES)} cases")
    assert moved >= 1 or variant in ("skip_padding", "workgroup")              # (those two move at most the sign of a zero)


# -- 4. two hand cases in exact rationals ------------------------------------------------------------------------------------------------------
def rational_policy(features, hidden, w1, b1, w2, b2):
    dense = np.zeros((features, hidden))
    for (f, j), w in w1.items():
        dense[f, j] = float(w)
    return C.pack(dense, [float(b) for b in b1], [[float(w) for w in row] for row in w2], [float(b) for b in b2])


def close(got, want, tol=1e-13):
    return abs(float(got) - float(want)) <= tol


def test_hand_case_a_bin_boundary_at_63_columns_in_9_bins(oracle):
    """Eye 0 at the origin heading +x, body 1 ten units ahead heading +x: its rear edge, at view distance 9, spans |lateral| <= 1, which
    is |ndc| <= kx / 9 with kx = 1 / (63 tan(45 / 63 degrees)): the centres of columns 27 .. 35, and no others.  Seven columns a bin:
    bin 3 holds column 27 alone, bin 4 columns 28 .. 34, bin 5 column 35 alone; depth = A (1 - 1/9), A = 10000/9999, so x = 1 - 8 A / 9 =
    9991/89991 there and 0 elsewhere."""
    width, features, hidden = 63, 9, 2
    kx = 1.0 / (63.0 * math.tan(math.radians(45.0 / 63.0)))
    inside = [c for c in range(63) if abs((c + 0.5 - 31.5) / 31.5) <= kx / 9.0]
    assert inside == list(range(27, 36)) and {c // 7 for c in inside} == {3, 4, 5} and {c // 9 for c in inside} == {3}
    x_near = 1 - Fraction(10000, 9999) * Fraction(8, 9)
    assert x_near == Fraction(9991, 89991)
    want_x = [x_near if f in (3, 4, 5) else Fraction(0) for f in range(9)]
    w1 = {(3, 0): Fraction(1), (4, 0): Fraction(2), (5, 0): Fraction(4), (2, 0): Fraction(64), (6, 0): Fraction(64), (4, 1): Fraction(-1)}
    b1, w2, b2 = [Fraction(-1, 128), Fraction(1, 64)], [[Fraction(1), Fraction(8)], [Fraction(-1, 4), Fraction(1)]], [Fraction(1, 256), Fraction(0)]
    t = [b1[j] + sum(w * want_x[f] for (f, jj), w in w1.items() if jj == j) for j in range(2)]
    assert t[0] == 7 * x_near - Fraction(1, 128) > 0 and t[1] < 0
    h = [max(v, Fraction(0)) for v in t]
    o = [b2[k] + sum(w2[k][j] * h[j] for j in range(2)) for k in range(2)]
    limit = Fraction(1, 2)
    assert o[0] > limit and -limit < o[1] < 0                                   # thrust is clipped, turn is not
    o = [min(max(v, -limit), limit) for v in o]
    dt = Fraction(float(C.DT))
    want_v = [Fraction(1) + o[0] * dt, -o[1] * dt, Fraction(0)]                 # f = (1, 0, 0); s = f x up = (0, -1, 0): a = (o_0, -o_1, 0)
    want_p = [want_v[0], want_v[1], Fraction(0)]
    pos, vel = np.array([[[0, 0, 0], [10, 0, 0]]], F32), np.array([[[1, 0, 0], [1, 0, 0]]], F32)
    pol = rational_policy(features, hidden, w1, b1, w2, b2)[None]
    ref = PR.batch(pos, vel, [0, 1], width, C.UP, 1.0, 10000.0, pol, features, hidden, 0.5, C.DT)[0]
    assert all(close(ref.x[0, f], want_x[f]) for f in range(9)) and (ref.x[1] == 0).all() and (ref.dx[1] == 0).all()
    assert all(close(ref.o[0, k], o[k]) for k in range(2)) and ref.do[0, 0] == 0 and 0 < ref.do[0, 1] < 1e-4
    assert all(close(ref.vel[0, k], want_v[k]) and close(ref.pos[0, k], want_p[k]) for k in range(3)) and ref.vel[0, 1] > 0
    blind = b2[0] + w2[0][1] * b1[1]                                            # eye 1 looks away: the biases alone, unit 1 on
    assert close(ref.o[1, 0], blind) and close(ref.vel[1, 0], 1 + blind * dt) and close(ref.pos[1, 0], 11 + blind * dt)
    c = dict(name="hand: 63 columns", pos=pos, vel=vel, up=np.array(C.UP, F32), width=width, lens=C.LENSES[0], policies=pol, features=features,
             hidden=hidden, limit=0.5)
    x, got_o, states = C.restated(oracle, c)
    print("\nhand case, 63 columns: error / bound", PR.compare(c["name"], [ref], x, got_o, *states[0]))
    assert (x[0, 0] > 0).tolist() == [f in (3, 4, 5) for f in range(9)]


def test_hand_case_an_eye_off_the_plane_under_the_tilted_up(oracle):
    """Eye 0 at (1, 2, 3) heading +y under up = (0.6, 0, 0.8): f = (0, 1, 0), s = f x up = (0.8, 0, -0.6), u = s x f = (0.6, 0, 0.8).  Body 1
    ten units ahead at the same height heading +y has its rear edge from (0, 11, 3) to (2, 11, 3): view distance 9, lateral 0.8 (x - 1),
    height 0.6 (x - 1).  A row is a slit: |ky height| <= 9 with ky = 1 / tan(45 / 64 degrees) leaves |x - 1| <= 9 / (0.6 ky), lateral
    |ndc| <= (ky / 64) 0.8 (9 / (0.6 ky)) / 9 = 1 / 48: the centres of columns 31 and 32 of 64 (ndc -+1/64) and no others (+-3/64).
    Under up = (0, 0, 1) the edge lies in the slit whole and fills ten columns: the tilt is what the two columns tell."""
    width, features, hidden = 64, 64, 1
    pos, vel = np.array([[[1, 2, 3], [1, 12, 3]]], F32), np.array([[[0, 2, 0], [0, 1, 0]]], F32)
    x_near = Fraction(9991, 89991)
    w1 = {(31, 0): Fraction(1), (32, 0): Fraction(2), (30, 0): Fraction(64), (33, 0): Fraction(64)}
    b1, w2, b2 = [Fraction(-1, 128)], [[Fraction(1)], [Fraction(-1, 2)]], [Fraction(0), Fraction(1, 64)]
    h = 3 * x_near - Fraction(1, 128)
    o = [h, Fraction(1, 64) - h / 2]
    assert h > 0 and abs(o[0]) < 1 and abs(o[1]) < 1
    dt = Fraction(float(C.DT))
    s = [Fraction(4, 5), Fraction(0), Fraction(-3, 5)]
    want_v = [o[1] * s[0] * dt, 2 + o[0] * dt, o[1] * s[2] * dt]
    want_p = [1 + want_v[0], 2 + want_v[1], 3 + want_v[2]]
    pol = rational_policy(features, hidden, w1, b1, w2, b2)[None]
    ref = PR.batch(pos, vel, [0, 1], width, (0.6, 0.0, 0.8), 1.0, 10000.0, pol, features, hidden, INF, C.DT)[0]
    assert [f for f in range(64) if ref.x[0, f] > 0] == [31, 32] and all(close(ref.x[0, f], x_near) for f in (31, 32))
    assert all(close(ref.o[0, k], o[k]) for k in range(2))
    assert all(close(ref.vel[0, k], want_v[k], 1e-12) and close(ref.pos[0, k], want_p[k], 1e-12) for k in range(3))
    flat = PR.batch(pos, vel, [0], width, C.UP, 1.0, 10000.0, pol, features, hidden, INF, C.DT)[0]
    kx = 1.0 / (64.0 * math.tan(math.radians(45.0 / 64.0)))
    whole = [c for c in range(64) if abs((c + 0.5 - 32.0) / 32.0) <= kx / 9.0]
    assert len(whole) == 10 and [f for f in range(64) if flat.x[0, f] > 0] == whole
    c = dict(name="hand: tilted", pos=pos, vel=vel, up=np.array((0.6, 0.0, 0.8), F32), width=width, lens=C.LENSES[0], policies=pol, features=features,
             hidden=hidden, limit=INF)
    x, got_o, states = C.restated(oracle, c)
    print("\nhand case, tilted: error / bound", PR.compare(c["name"], [ref], x, got_o, *states[0]))
