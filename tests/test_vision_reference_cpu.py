"""Premises of the geometric reference (tests/vision_reference.py), no device: it reproduces the suite's hand-derived results on its
own; the numpy restatements of DESIGN.md sections 10-12 lie within its bounds on every decided cell of every case
(tests/vision_reference_cases.py); the cases meet their caps and coverage conditions; and the bounds are tight enough to matter:
eight mutations of the restatements' output path, applied to copies inside this file, are each rejected on decided cells.

Largest observed error / bound of the restatements over the cases (test_the_ratios_over_all_cases prints them; run with -s):
    eyes / eyes_colour   depth 0.026   rgba 0.078
    eyes_msaa            depth8 0.021  rgba 0.19       (16 eyes a case; 0.19 on a centre clamped to an edge's end, bound 6 * 2^-24)
    frame                depth 0.014   rgba 0.062
    seen                 nearest depth 0.026 where one edge decides it, 0.975 over all (see next line)
and where another edge of the winning body may be the nearer one (the bound then spans both edges' depths): below 1.0 by
construction, 0.9999 observed.  The bounds count 60 roundings on magnitude sums where a handful act, hence the small ratios; the
control arms below show that they still reject every mistake of the kinds the rule could hide."""
import inspect
import math
import types

import numpy as np
import pytest

import eyes_colour_restatement as K
import eyes_msaa_restatement as M
import eyes_restatement as R
import frame_restatement as FR
import seen_restatement as S
import vision_reference as V
import vision_reference_cases as C

F = np.float32
UP = np.array([0, 0, 1], F)
EYE_FOVY, EYE_ASPECT = float(F(90.0) / F(1024.0)), 1024.0


# -- 1. the hand-derived results, from geometry alone --------------------------------------------------------------------------------------
def straight_ahead(**kw):
    pos = np.array([[0, 0, 0], [10, 0, 0]], F)
    vel = np.array([[1, 0, 0], [1, 0, 0]], F)
    return V.eye_rows(pos, vel, [0, 1], 1024, UP, EYE_FOVY, EYE_ASPECT, **kw)


def test_one_body_straight_ahead_fills_columns_440_to_583():
    r = straight_ahead()
    assert not r.und.any() and not r.und_rgba.any()
    assert (np.nonzero(r.ids[0] != V.NONE)[0] == np.arange(440, 584)).all() and (r.ids[0, 440:584] == 1).all()
    assert np.allclose(r.depth[0, 440:584], 10000 / 9999 * 8 / 9, rtol=0, atol=1e-15) and (r.edge[0, 440:584] == 2).all()
    assert (r.ids[1] == V.NONE).all() and (r.depth[1] == 1).all()            # eye 1 looks away: a body behind the eye is unseen
    assert (r.rgba[0, :440] == V.CLEAR).all() and (r.rgba[1] == V.CLEAR).all()


def test_the_centre_pair_of_that_span_shades_the_hand_value():
    r = straight_ahead()
    want = 1.0 - 40.5 * math.tan(math.radians(90.0 / 2048.0)) ** 2
    assert np.allclose(r.rgba[0, [511, 512], :3], want, rtol=0, atol=1e-14) and (r.rgba[0, 440:584, 3] == 1).all()
    assert (np.diff(r.rgba[0, 440:512, 0]) > 0).all() and (np.diff(r.rgba[0, 512:584, 0]) < 0).all()
    assert float(r.drgba[0, 511, 0]) < 1e-5 and float(r.ddepth[0, 511]) < 1e-4       # the bounds are far below what they guard


def test_a_row_spans_less_than_90_degrees():
    """the column planes at the row's two ends are 2 atan(W tan(45 / W degrees)) apart: a body at that bearing's inside is seen,
    one between it and 45 degrees is not"""
    for width in (64, 1024):
        half = math.atan(width * math.tan(math.radians(45.0 / width)))
        assert abs(2 * math.degrees(half) - 76.3) < 0.1
        fovy, aspect = float(F(90.0) / F(width)), float(width)
        L = V.lens(fovy, aspect)
        assert abs(math.atan(1.0 / L.kx) - half) < 1e-12
        for bearing, seen in ((half - 0.05, True), (half + 0.05, False), (math.radians(44.0), False)):
            pos = np.array([[0, 0, 0], [30 * math.cos(bearing), 30 * math.sin(bearing), 0]], F)
            vel = np.array([[1, 0, 0], [1, 0, 0]], F)
            r = V.eye_rows(pos, vel, [0], width, UP, fovy, aspect)
            assert ((r.ids[0] == 1).any()) == seen and not r.und.any(), (width, bearing)
            if seen:
                assert np.nonzero(r.ids[0] == 1)[0].max() < width / 8      # +y is to the left: among the row's first columns


def test_bodies_behind_the_eye_or_beyond_far_are_unseen():
    pos = np.array([[0, 0, 0], [-10, 0, 0], [60, 10, 0], [20, 0, 0]], F)
    vel = np.tile(F([1, 0, 0]), (4, 1))
    r = V.eye_rows(pos, vel, [0], 1024, UP, EYE_FOVY, EYE_ASPECT, far=50.0)
    assert set(np.unique(r.ids[0])) == {3, V.NONE} and not r.und.any()
    r = V.eye_rows(pos, vel, [0], 1024, UP, EYE_FOVY, EYE_ASPECT)
    assert set(np.unique(r.ids[0])) == {2, 3, V.NONE}      # with the reference's far plane body 2 shows beside body 3's span
    assert (r.ids[0, 511] == 3) and r.depth[0, 511] < r.depth[0, np.nonzero(r.ids[0] == 2)[0][0]]


# -- 2. the restatements lie within the reference's bounds ----------------------------------------------------------------------------------
_results = {}


def restated_eyes(oracle, name, see_self=None, cp=None, colour=K.colour):
    c = C.EYE_CASES[name]
    pos, vel = C.eye_state(oracle, name)
    cams = oracle.cameras(pos[:c["eyes"]], vel[:c["eyes"]], np.array(c["up"], F), C.eye_constant(oracle, name) if cp is None else cp)
    skin = K.skin_from_srgb8(C.golden_skin()) if c["skin"] else None
    return colour(cams, oracle.instances(pos, vel), 0, c["width"], c["see_self"] if see_self is None else see_self, skin)


def restated_msaa(oracle, name):
    c = C.EYE_CASES[name]
    pos, vel = C.eye_state(oracle, name)
    e = C.eyes_of(name, True)
    cams = oracle.cameras(pos[:e], vel[:e], np.array(c["up"], F), C.eye_constant(oracle, name))
    skin = K.skin_from_srgb8(C.golden_skin()) if c["skin"] else None
    return M.msaa(cams, oracle.instances(pos, vel), 0, c["width"], c["see_self"], skin)


def restated_frame(oracle, name, frame=FR.frame):
    c = C.FRAME_CASES[name]
    pos, vel = C.frame_state(oracle)
    cam = FR.camera(oracle, c["eye"], c["direction"], c["up"], C.frame_constant(oracle, name))
    skin = K.skin_from_srgb8(C.golden_skin()) if c["skin"] else None
    return frame(cam, oracle.instances(pos, vel), *c["extent"], skin=skin)


def eye_case_result(oracle, name):
    if name not in _results:
        c = C.EYE_CASES[name]
        ref = C.eye_reference(oracle, name)
        ids, depth, rgba, _ = restated_eyes(oracle, name)
        plain = R.eyes(oracle.cameras(*[a[:c["eyes"]] for a in C.eye_state(oracle, name)], np.array(c["up"], F), C.eye_constant(oracle, name)),
                       oracle.instances(*C.eye_state(oracle, name)), 0, c["width"], c["see_self"])
        out = {"eyes": V.compare(name + " eyes", ref, *plain), "eyes_colour": V.compare(name + " eyes_colour", ref, ids, depth, rgba)}
        count, sids, sdepth, _ = S.seen_rows(ids, depth)
        out["seen"] = {"depth": V.compare_seen(name + " seen", ref, count, sids, sdepth)}
        if c["width"] <= C.MSAA_MAX_WIDTH:
            ids8, depth8, rgba8, _ = restated_msaa(oracle, name)
            out["eyes_msaa"] = V.compare(name + " eyes_msaa", C.eye_reference(oracle, name, True), ids8, depth8, rgba8)
        _results[name] = out
    return _results[name]


def frame_case_result(oracle, name):
    if name not in _results:
        ids, depth, rgba, _ = restated_frame(oracle, name)
        _results[name] = {"frame": V.compare(name + " frame", C.frame_reference(oracle, name), ids, depth, rgba, axes=("row", "column"))}
    return _results[name]


def report(name, ref, result):
    touched, und, covered = C.shares(ref)
    print(f"\n{name}: {touched} cells touched, {und} undecided ({100.0 * und / max(touched, 1):.2f} %), {covered} decided covered; "
          + "; ".join(f"{k} " + " ".join(f"{o} {v:.4f}" for o, v in r.items()) for k, r in result.items()))


@pytest.mark.parametrize("name", list(C.EYE_CASES))
def test_the_eye_restatements_lie_within_the_bounds(oracle, name):
    result = eye_case_result(oracle, name)
    report(name, C.eye_reference(oracle, name), result)
    assert all(v <= 1.0 for r in result.values() for v in r.values()), result


@pytest.mark.parametrize("name", list(C.FRAME_CASES))
def test_the_frame_restatement_lies_within_the_bounds(oracle, name):
    result = frame_case_result(oracle, name)
    report(name, C.frame_reference(oracle, name), result)
    assert all(v <= 1.0 for r in result.values() for v in r.values()), result


def test_the_ratios_over_all_cases(oracle):
    """the largest error / bound per output; the figures of this module's docstring and of DESIGN.md sections 10 and 11"""
    worst = {}
    for name in C.EYE_CASES:
        for entry, r in eye_case_result(oracle, name).items():
            for o, v in r.items():
                worst[(entry, o)] = max(worst.get((entry, o), 0.0), v)
    for name in C.FRAME_CASES:
        for entry, r in frame_case_result(oracle, name).items():
            for o, v in r.items():
                worst[(entry, o)] = max(worst.get((entry, o), 0.0), v)
    print("\nlargest error / bound: " + "; ".join(f"{e} {o} {v:.5f}" for (e, o), v in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values())
    # what the docstring records, with room (the seen sets' least depth may come from a two-edge column)
    assert all(v < 0.25 for (e, o), v in worst.items() if o != "depth_two_edges" and e != "seen"), worst
    assert V.R == 60 and V.ROUNDINGS == dict(camera=29, instance=11, step1=4, rule=16)


# -- 3. the caps and the coverage conditions ---------------------------------------------------------------------------------------------------
def test_the_case_list_holds_the_shapes_it_promises():
    cs = C.EYE_CASES.values()
    assert {c["n"] for c in cs} == {2, 3, 100, 257} and {c["width"] for c in cs} == {1, 3, 64, 65, 256, 1024, 4096}
    assert [c["eyes"] for c in cs if c["width"] == 4096] == [8] and max(c["eyes"] for c in cs) == 48
    assert {c["scale"] for c in cs} == {0.1, 1.0, 30.0} and all(c["width"] == 256 for c in cs if c["scale"] == 30.0)
    assert any(c["near"] == 0.5 and c["see_self"] for c in cs) and any(c["far"] == 50.0 for c in cs)
    assert any(c["lift"] and c["up"] != C.UP for c in cs) and any(c["skin"] for c in cs) and any(not c["skin"] for c in cs)
    assert {c["extent"] for c in C.FRAME_CASES.values()} == {(64, 48), (96, 64), (1, 1), (3, 2)} and C.FRAME_N == 40


@pytest.mark.parametrize("name", list(C.EYE_CASES) + list(C.FRAME_CASES))
def test_the_caps_hold_on_the_reference_alone(oracle, name):
    eye = name in C.EYE_CASES
    case = C.EYE_CASES[name] if eye else C.FRAME_CASES[name]
    refs = [C.eye_reference(oracle, name)] if eye else [C.frame_reference(oracle, name)]
    if eye and case["width"] <= C.MSAA_MAX_WIDTH:
        refs.append(C.eye_reference(oracle, name, True))
    for ref in refs:
        touched, und, covered = C.shares(ref)
        no_colour, columns, compared = C.colour_shares(ref)
        print(f"\n{name}: undecided {und} of {touched} touched ({100.0 * und / max(touched, 1):.2f} %), decided covered {covered}; colour not "
              f"compared on {no_colour} ({100.0 * no_colour / max(touched, 1):.2f} %); {compared} of {columns} touched columns or pixels compared "
              f"in colour, largest bound {ref.drgba[~ref.und_rgba].max():.2g}")
        assert und <= C.CAPS["undecided_share"] * touched, (name, und, touched)
        assert covered >= (1 if case["exempt"] else C.CAPS["decided_covered"]), (name, covered)
        if not case["colour_exempt"]:
            assert no_colour <= C.CAPS["undecided_share"] * touched, (name, no_colour, touched)
        least = 1 if case["exempt"] else C.CAPS["colour_compared_exempt" if case["colour_exempt"] else "colour_compared"]
        assert compared >= least, (name, compared)
        assert ref.drgba[~ref.und_rgba].max() <= V.MAX_COLOUR_BOUND         # no compared colour has a vacuous bound


def test_only_the_far_away_case_is_exempt_from_the_colour_cap():
    assert [n for n, c in C.EYE_CASES.items() if c["colour_exempt"]] == ["n100_w256_far_away"]
    assert not any(c["colour_exempt"] for c in C.FRAME_CASES.values())


def test_the_coverage_conditions_hold_over_the_list(oracle):
    eye, frame = V.new_stats(), V.new_stats()
    for name in C.EYE_CASES:
        for k, v in C.eye_reference(oracle, name).stats.items():
            eye[k] = eye[k] + v
    for name in C.FRAME_CASES:
        for k, v in C.frame_reference(oracle, name).stats.items():
            frame[k] = frame[k] + v
    print(f"\neye rows: {eye}\nframes: {frame}")
    assert (eye["edge"] > 1000).all() and (frame["edge"] > 100).all()                  # every edge index wins
    assert (eye["cut"] > 100).all()                                                     # near, far, y = -w, y = +w cut winning edges
    assert frame["cut"][0] > 0 and frame["cut"][2] > 0                                  # the low camera's near plane; the frames' lower edge
    assert eye["unequal_w"] > 1000 and frame["unequal_w"] > 100 and eye["hidden"] > 1000 and frame["hidden"] > 10
    assert frame["xmajor"] > 100 and frame["ymajor"] > 100


# -- 4. control arms: mistakes the rule could hide, each rejected on decided cells -----------------------------------------------------------
def mutant(module, edits, **deps):
    """a copy of a restatement module with `edits` (old text, new text) applied to its source and `deps` (its imported restatement
    modules, as other mutants) replaced: the shipped module stays untouched"""
    src = inspect.getsource(module)
    for old, new in edits:
        assert old in src, f"{module.__name__} no longer reads {old!r}"
        src = src.replace(old, new)
    ns = {"__name__": module.__name__ + "_mutant"}
    exec(compile(src, module.__file__, "exec"), ns)
    ns.update(deps)
    return types.SimpleNamespace(**ns)


KINDS = {"body": "against the reference's", "depth": ": depth ", "colour": ": colour "}


def rejected(case, ref, got, kind, **kw):
    """`compare` refuses `got`, and for the reason the arm is about: a wrong body, depth or colour on a decided cell"""
    with pytest.raises(AssertionError) as failure:
        V.compare(case, ref, *got, **kw)
    print(f"\nrejected: {failure.value}")
    message = str(failure.value)
    assert KINDS[kind] in message and ("body " in message) and "shapes" not in message, message
    return message


def test_arm_the_eye_constant_of_a_true_90_degree_row(oracle):
    name = "n100_w1024_skin"
    cp = oracle.camera_constant(math.degrees(2 * math.atan(1.0 / 1024.0)), 1024.0, 1.0, 10000.0)
    rejected(name, C.eye_reference(oracle, name), restated_eyes(oracle, name, cp=cp)[:3], "body")


def test_arm_the_edge_parameter_interpolated_in_screen_space(oracle):
    name = "n257_w1024_close"
    mk = mutant(K, [("sk = num / den", "sk = s0 + t * (s1 - s0)")])
    ids, depth, rgba, _ = restated_eyes(oracle, name, colour=mk.colour)
    rejected(name, C.eye_reference(oracle, name), (ids, depth, rgba), "colour")
    V.compare(name, C.eye_reference(oracle, name), ids, depth)            # ids and depth are untouched: the colour alone tells


def test_arm_edge_2_textured_s_s(oracle):
    name = "n100_w1024_skin"
    mk = mutant(K, [("one_minus = F(1) - s ", "one_minus = s ")])
    rejected(name, C.eye_reference(oracle, name), restated_eyes(oracle, name, colour=mk.colour)[:3], "colour")


def test_arm_a_model_vertex_moved(oracle):
    name = "n100_w1024_skin"
    mr = mutant(R, [("[1, 0, 0, 1]", "[1, 0.05, 0, 1]")])
    mk = mutant(K, [], R=mr)
    rejected(name, C.eye_reference(oracle, name), restated_eyes(oracle, name, colour=mk.colour)[:3], "body")
    name = "oblique_96x64_skin"
    mf = mutant(FR, [], R=mr, K=mk)
    rejected(name, C.frame_reference(oracle, name), restated_frame(oracle, name, frame=mf.frame)[:3], "body", axes=("row", "column"))


def coincident():
    pos = np.array([[0, 0, 0], [10, 0, 0], [10, 0, 0]], F)
    vel = np.tile(F([1, 0, 0]), (3, 1))
    return pos, vel, V.eye_rows(pos, vel, [0], 1024, UP, EYE_FOVY, EYE_ASPECT)


def test_arm_equal_keys_resolved_to_the_higher_index(oracle):
    """two coincident bodies give equal keys but for the index: the lower one shows, and nothing is undecided"""
    pos, vel, ref = coincident()
    assert not ref.und.any() and (ref.ids[0, 440:584] == 1).all()
    cams = oracle.cameras(pos[:1], vel[:1], UP, R.eye_constant(oracle))
    V.compare("coincident", ref, *R.eyes(cams, oracle.instances(pos, vel), 0, 1024))
    top = "np.uint64(0xFFFFFFFE)"
    mr = mutant(R, [("| j_idx[seg].astype(np.uint64)", f"| ({top} - j_idx[seg].astype(np.uint64))"),
                    ("(keys & np.uint64(0xFFFFFFFF)).astype(np.uint32))", f"({top} - (keys & np.uint64(0xFFFFFFFF))).astype(np.uint32))")])
    ids, depth = mr.eyes(cams, oracle.instances(pos, vel), 0, 1024)
    assert (ids[0, 440:584] == 2).all()
    assert "body 2 " in rejected("coincident", ref, (ids, depth), "body")


def test_arm_the_own_body_not_skipped(oracle):
    """the restatement's skip of the eye's own body taken out: with the near plane at 0.5 every eye then sees its own side edges"""
    name = "n3_w1024_close_near_self"
    c = C.EYE_CASES[name]
    pos, vel = C.eye_state(oracle, name)
    ref = V.eye_rows(pos, vel, np.arange(3), 1024, c["up"], *C.eye_lens(name), c["near"], c["far"], see_self=False)
    V.compare(name, ref, *restated_eyes(oracle, name, see_self=False)[:3])
    mr = mutant(R, [("    if not see_self:\n        own = first", "    if False:\n        own = first")])
    mk = mutant(K, [], R=mr)
    message = rejected(name, ref, restated_eyes(oracle, name, see_self=False, colour=mk.colour)[:3], "body")
    assert f"the reference's {V.NONE}" in message           # an eye's own body where the reference sees nothing


def test_arm_closed_span_ends(oracle):
    """a span that covers every column one of its ends falls in: caught through decided EMPTY cells next to spans"""
    name = "n100_w1024_skin"
    mr = mutant(R, [("covered = (xa[seg] <= xc) & (xc < xb[seg])", "covered = (np.floor(xa[seg]) <= xc) & (xc < np.floor(xb[seg]) + 1)")])
    c = C.EYE_CASES[name]
    pos, vel = C.eye_state(oracle, name)
    cams = oracle.cameras(pos[:c["eyes"]], vel[:c["eyes"]], UP, C.eye_constant(oracle, name))
    ids, depth = mr.eyes(cams, oracle.instances(pos, vel), 0, c["width"])
    ref = C.eye_reference(oracle, name)
    empty = ~ref.und & ~ref.touched
    assert (empty & (ids != V.NONE)).sum() > 100             # decided empty cells that the closed ends cover
    rejected(name, ref, (ids, depth), "body")
    # and through the empty cells alone: every other cell given the reference's own value
    assert f"the reference's {V.NONE}" in rejected(name, ref, (np.where(empty, ids, ref.ids), np.where(empty, depth, ref.depth)), "body")


def test_arm_the_frames_rows_flipped(oracle):
    name = "oblique_96x64_skin"
    mf = mutant(FR, [("g - (Q0[:, 1] / Q0[:, 3]) * g", "g + (Q0[:, 1] / Q0[:, 3]) * g"), ("g - (Q1[:, 1] / Q1[:, 3]) * g", "g + (Q1[:, 1] / Q1[:, 3]) * g")])
    rejected(name, C.frame_reference(oracle, name), restated_frame(oracle, name, frame=mf.frame)[:3], "body", axes=("row", "column"))
