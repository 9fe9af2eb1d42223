"""GPU tests of the scene batches' policy and score against their binary64 references (tests/policy_reference.py,
tests/score_reference.py) on the cases of tests/policy_reference_cases.py.  Every result is compared twice -- (a) with the
reference: every feature and output of every eye within its interval, the stepped records within their bounds, `near` within its
interval and every float of a record within its bound; (b) bit for bit with the numpy restatements (tests/policy_restatement.py on
the rows of tests/eyes_restatement.py and the oracle's cameras, tests/score_restatement.py), chained step by step: the first bitwise
check of the policy on 3-D data, a tilted `up`, other lenses and W / F that is no power of two.  What the cases cover, that the
restatements lie within the references and that the references reject mistakes of meaning is checked on the CPU
(tests/test_policy_score_reference_cpu.py)."""
import numpy as np
import pytest

import policy_reference as PR
import policy_reference_cases as C
import score_cases as SK
import score_reference as QR
import score_restatement as Q
import test_gpu_scenes_policy as TP
import test_gpu_scenes_score as TS

pytestmark = pytest.mark.gpu

F = np.float32
STATELESS = ("3d3_n129_w63_f9_h33_tilted", "lifted3_n65_w65_f5_h63_tilted_far50", "3d10_n100_w200_f25_h2_near05")


def setup(nb, c):
    return dict(width=c["width"], up=c["up"], cp=C.camera_constant(nb, c))


def run_case(nb, oracle, c):
    """observe, one step, then k steps in one call through the context: the reference on the first step, the restatement's chain on
    every word"""
    eye, k = setup(nb, c), c["k"]
    with nb.SceneBatch(c["pos"], c["vel"]) as sb:
        sb.set_policy(c["policies"], c["features"], c["hidden"], c["limit"])
        x, o = sb.policy_observe(**eye)
        sb.step_policy(1, **eye)
        p1, v1 = sb.positions(), sb.velocities()
        sb.step_policy(k, **eye)
        pk, vk = sb.positions(), sb.velocities()
        assert sb.steps_done == 1 + k
    ratios = PR.compare(c["name"], C.reference(c), x, o, p1, v1)
    print(f"\n{c['name']}: error / bound " + " ".join(f"{w} {v:.4f}" for w, v in ratios.items()))
    want_x, want_o, states = C.restated(oracle, c, steps=1 + k)
    for got, want, what in ((x, want_x, "features"), (o, want_o, "outputs"), (p1, states[0][0], "positions after one step"),
                            (v1, states[0][1], "velocities after one step"), (pk, states[k][0], f"positions after 1 + {k} steps"),
                            (vk, states[k][1], f"velocities after 1 + {k} steps")):
        TP.assert_words(got, want, f"{c.get('line', c['name'])}: {what}")
    return ratios


@pytest.mark.parametrize("name", list(C.FIXED))
def test_fixed_cases(nb, oracle, name):
    c = C.fixed(name)
    assert all(v <= 1.0 for v in run_case(nb, oracle, c).values())


@pytest.mark.parametrize("i", range(C.RANDOM_CASES))
def test_random_problems(nb, oracle, i):
    c = C.case(i)
    print("\n" + c["line"])
    assert all(v <= 1.0 for v in run_case(nb, oracle, c).values()), c["line"]


def test_both_launch_shapes_are_among_the_cases():
    sizes = [C.fixed(name)["n"] for name in C.FIXED] + [C.case(i)["n"] for i in range(C.RANDOM_CASES)]
    assert min(sizes) <= 128 < max(sizes) and {127, 128, 129} <= set(sizes)
    assert {C.fixed(name)["n"] > 128 for name in STATELESS} == {True, False}


@pytest.mark.parametrize("name", STATELESS)
def test_stateless_launches(nb, oracle, name):
    """nb_scenes_policy_observe_launch and nb_scenes_policy_step_launch on caller-owned memory, cameras and model matrices from the
    device under the case's lens and `up`: the reference and the restatement's words"""
    import torch

    from nenbody_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    c = C.fixed(name)
    b, n, width, features, hidden = c["batch"], c["n"], c["width"], c["features"], c["hidden"]
    pol, records = c["policies"], c["batch"] * c["n"]
    t_pos, t_vel = torch.from_numpy(TP.records_of(c["pos"])).to(dev), torch.from_numpy(TP.records_of(c["vel"])).to(dev)
    t_pol = torch.from_numpy(np.array(pol, F)).to(dev)
    o_pos, o_vel = torch.zeros((records, 4), dtype=torch.float32, device=dev), torch.zeros((records, 4), dtype=torch.float32, device=dev)
    cpm = np.ascontiguousarray(C.camera_constant(nb, c), F).reshape(16)
    up = np.ascontiguousarray(c["up"], F)
    cams = torch.empty((records, 16), dtype=torch.float32, device=dev)
    inst = torch.empty((records, 16), dtype=torch.float32, device=dev)
    feat = torch.full((records + 1, features), TP.FILL, dtype=torch.int32, device=dev)
    act = torch.full((records + 1, 2), TP.FILL, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        _lib.check(lib.nb_launch_instances(records, t_pos.data_ptr(), t_vel.data_ptr(), inst.data_ptr(), s.cuda_stream))
        _lib.check(lib.nb_launch_cameras(records, t_pos.data_ptr(), t_vel.data_ptr(), up.ctypes.data, cpm.ctypes.data, cams.data_ptr(), s.cuda_stream))
        _lib.check(lib.nb_scenes_policy_observe_launch(b, n, 0, records, cams.data_ptr(), inst.data_ptr(), width, features, hidden, len(pol),
                                                       t_pol.data_ptr(), float(c["limit"]), feat.data_ptr(), act.data_ptr(), s.cuda_stream))
        _lib.check(lib.nb_scenes_policy_step_launch(None, b, n, cams.data_ptr(), inst.data_ptr(), width, up.ctypes.data, features, hidden,
                                                    len(pol), t_pol.data_ptr(), float(c["limit"]), t_pos.data_ptr(), t_vel.data_ptr(),
                                                    o_pos.data_ptr(), o_vel.data_ptr(), s.cuda_stream))
    s.synchronize()
    g_feat, g_act = feat.cpu().numpy().view(np.uint32), act.cpu().numpy().view(np.uint32)
    assert (g_feat[records] == TP.FILL).all() and (g_act[records] == TP.FILL).all()
    x, o = g_feat[:records].view(F).reshape(b, n, features), g_act[:records].view(F).reshape(b, n, 2)
    p1, v1 = o_pos.cpu().numpy()[:, :3].reshape(b, n, 3), o_vel.cpu().numpy()[:, :3].reshape(b, n, 3)
    print(f"\n{name}, stateless: error / bound", PR.compare(name + " (stateless)", C.reference(c), x, o, p1, v1))
    want_x, want_o, states = C.restated(oracle, c)
    for got, want, what in ((x, want_x, "features"), (o, want_o, "outputs"), (p1, states[0][0], "positions"), (v1, states[0][1], "velocities")):
        TP.assert_words(got, want, f"{name}, stateless: {what}")


# -- scored rollouts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.ROLLOUTS)
def test_scored_rollouts(nb, oracle, name):
    """step_policy_scored(3): the records are score_restatement's on the restated states between the steps, word for word, and lie
    within the score reference accumulated over the same three snapshots"""
    c = C.fixed(name)
    score = C.ROLLOUT_SCORE
    with nb.SceneBatch(c["pos"], c["vel"]) as sb:
        sb.set_policy(c["policies"], c["features"], c["hidden"], c["limit"])
        sb.set_score(float(score["radius_sq"]), score["goal"])
        sb.step_policy_scored(3, **setup(nb, c))
        got, p3, v3 = sb.scores(), sb.positions(), sb.velocities()
    _, _, states = C.restated(oracle, c, steps=3)
    TP.assert_words(p3, states[2][0], f"{name}: positions after the rollout")
    TP.assert_words(v3, states[2][1], f"{name}: velocities after the rollout")
    want = ref = None
    for p, v in states:
        want = Q.batch(p, v, score["radius_sq"], score["goal"], acc=want)
        ref = QR.batch(p, v, score["radius_sq"], score["goal"], acc=ref)
    TS.assert_records(got, want, f"{name}: the rollout's records")
    assert (got["steps"] == 3).all() and (got["near"] > 0).any()
    print(f"\n{name}, scored rollout: near {got['near'].tolist()} of {[(r.near_lo, r.near_hi) for r in ref]}; error / bound",
          QR.compare(f"{name}: the rollout's records", ref, got))


# -- the score alone -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SK.KINDS)
def test_score_launch_against_the_reference(nb, kind):
    """nb_scenes_score_launch from cleared records, and a second snapshot accumulated: `near` within its interval, every held float
    within its bound, `steps` and `nonfinite` exactly"""
    worst = {}
    for n in C.SCORE_SIZES:
        pos, vel, radius_sq, goal = SK.make(kind, n)
        one = TS.launch(pos, vel, radius_sq, goal)
        r = QR.compare(f"{kind} n={n}", C.score_reference(kind, n), one)
        two = TS.launch(pos, vel, radius_sq, goal, snapshots=2)
        r2 = QR.compare(f"{kind} n={n}, two snapshots", QR.batch(pos, vel, radius_sq, goal, acc=C.score_reference(kind, n)), two)
        assert (two["steps"] == 2).all() and (two["near"] == 2 * one["near"]).all()
        TS.assert_records(one, SK.want(kind, n), f"{kind} n={n}")
        for key, v in list(r.items()) + [("two " + k, v) for k, v in r2.items()]:
            worst[key] = max(worst.get(key, 0.0), v)
    print(f"\n{kind}: error / bound " + " ".join(f"{k} {v:.4f}" for k, v in worst.items()))


# -- P7 ---------------------------------------------------------------------------------------------------------------------------------------
def test_scenes_of_four_kinds_in_one_launch_are_what_they_are_alone_and_permuted(nb, oracle):
    """a planar, a 3-D, a zero-velocity and a clustered scene in one launch, each with its own policy: each equals its result alone
    and its result in a permuted batch, and the reference holds all four"""
    n, width, features, hidden, limit = 65, 63, 9, 33, 0.5
    rng = np.random.default_rng(1790)
    states = [C.state(rng, n, kind, 3.0, 0.1, C.TILTED, zeros=zeros) for kind, zeros in (("planar", False), ("3-D", False), ("3-D", True), ("clustered", False))]
    c = dict(name="four kinds", n=n, batch=4, width=width, features=features, hidden=hidden, limit=limit, lens=C.LENSES[2], up=np.array(C.TILTED, F),
             pos=np.stack([s[0] for s in states]), vel=np.stack([s[1] for s in states]), policies=C.policies(features, hidden, 4, 1790, 4.0), k=2,
             eyes=n)
    eye = setup(nb, c)

    def run(order):
        with nb.SceneBatch(c["pos"][order], c["vel"][order]) as sb:
            sb.set_policy(c["policies"][order], features, hidden, limit)
            x, o = sb.policy_observe(**eye)
            sb.step_policy(2, **eye)
            return x, o, sb.positions(), sb.velocities()

    whole = run([0, 1, 2, 3])
    assert len({TP.bits(whole[3][s]).tobytes() for s in range(4)}) == 4
    order = [2, 0, 3, 1]
    moved = run(order)
    for a, b in zip(whole, moved):
        assert (TP.bits(b) == TP.bits(a[order])).all()
    for s in range(4):
        alone = run([s])
        for a, b in zip(whole, alone):
            assert (TP.bits(b[0]) == TP.bits(a[s])).all(), s
    run_case(nb, oracle, c)
