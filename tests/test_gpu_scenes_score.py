"""GPU tests of the scene batches' score: the kernel of nb_scenes_score.inc against the numpy restatement
(tests/score_restatement.py), every word of every record (Q1-Q7).  A float field that the restatement gives as a NaN is met by a NaN:
the rule leaves a NaN's sign and payload open (include/nenbody.h); every other comparison is of bit patterns, and two runs of the
device are compared byte for byte, NaNs included.

The cases, their batches, radii and goals are tests/score_cases.py's, and the expected records are computed once there;
tests/test_scenes_score_cpu.py holds their premises."""
import ctypes

import numpy as np
import pytest

import policy_cases as PK
import score_cases as K
import score_restatement as Q
from nenbody_amd._lib import SCENES_SCORE_PROTOTYPES   # (the parent commit has no such table: the file fails here)

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 0x07


def assert_records(got, want, what):
    got, want = np.ascontiguousarray(got, Q.DTYPE).reshape(-1), np.ascontiguousarray(want, Q.DTYPE).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not Q.same(got, want):
        bad = [s for s in range(len(got)) if not Q.same(got[s], want[s])]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ, first scene {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}")


def records_of(a, w):
    """(B, n, 3) -> (B * n, 4) records with `w` in the fourth word, which no rule reads"""
    out = np.full((a.shape[0] * a.shape[1], 4), w, F)
    out[:, :3] = a.reshape(-1, 3)
    return out


def launch(pos, vel, radius_sq, goal, snapshots=1, start=None, others=()):
    """nb_scenes_score_launch on `snapshots` copies of the batch's snapshot -- then on every (pos, vel) of `others` -- from the records
    `start` (cleared ones by default): the records; guard bytes in front of and behind the records and around pos and vel come back
    as they were, and pos and vel are unmodified"""
    import torch

    from nenbody_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    b, n = pos.shape[:2]
    sp = _lib.NbScoreParams(float(radius_sq), (ctypes.c_float * 3)(*[float(c) for c in goal]))
    rec = np.full((b + 2) * 32, GUARD, np.uint8)
    rec[32:-32] = 0 if start is None else np.ascontiguousarray(start, Q.DTYPE).view(np.uint8).reshape(-1)
    t_rec = torch.from_numpy(rec).to(dev)
    stream = torch.cuda.Stream(dev)
    for p, v in [(pos, vel)] * snapshots + list(others):
        hp = np.concatenate([np.full((1, 4), np.uint32(0x7FC0BEEF).view(F), F), records_of(p, np.nan), np.full((1, 4), np.uint32(0x7FC0BEEF).view(F), F)])
        hv = np.concatenate([np.full((1, 4), np.uint32(0x7FC0BEEF).view(F), F), records_of(v, np.inf), np.full((1, 4), np.uint32(0x7FC0BEEF).view(F), F)])
        t_pos, t_vel = torch.from_numpy(hp).to(dev), torch.from_numpy(hv).to(dev)
        with torch.cuda.stream(stream):
            _lib.check(lib.nb_scenes_score_launch(ctypes.byref(sp), b, n, t_pos.data_ptr() + 16, t_vel.data_ptr() + 16, t_rec.data_ptr() + 32,
                                                  stream.cuda_stream))
        stream.synchronize()
        assert (t_pos.cpu().numpy().view(np.uint32) == hp.view(np.uint32)).all() and (t_vel.cpu().numpy().view(np.uint32) == hv.view(np.uint32)).all()
    out = t_rec.cpu().numpy()
    assert (out[:32] == GUARD).all() and (out[-32:] == GUARD).all()
    return out[32:-32].view(Q.DTYPE).copy()


# -- every word of every record ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.KINDS)
def test_every_word_of_every_record(nb, kind):
    """B = 3 through the stateless launch from cleared records, every size of the case list: every workgroup of the ladder, both sides
    of each of its steps, a lane's second body"""
    for n in K.SIZES:
        pos, vel, radius_sq, goal = K.make(kind, n)
        assert_records(launch(pos, vel, radius_sq, goal), K.want(kind, n), f"{kind} n={n}")


def test_the_hand_case(nb):
    got = launch(K.HAND_POS[None], K.HAND_VEL[None], K.HAND_RADIUS_SQ, K.HAND_GOAL)
    assert_records(got, Q.batch(K.HAND_POS[None], K.HAND_VEL[None], K.HAND_RADIUS_SQ, K.HAND_GOAL), "hand case")
    assert int(got[0]["near"]) == 2 and got[0]["steps"] == 1 and got[0]["nonfinite"] == 0


def test_radius_zero_and_infinite(nb):
    """radius_sq = 0 counts nothing, not even coincident bodies; +inf counts every pair whose d2 is finite"""
    pos, vel, _, goal = K.make("lattice", 129)
    zero, every = launch(pos, vel, 0.0, goal), launch(pos, vel, np.inf, goal)
    assert (zero["near"] == 0).all() and (every["near"] == 129 * 128 // 2).all()
    assert_records(zero, Q.batch(pos, vel, 0.0, goal), "radius 0")
    npos, nvel, _, ngoal = K.make("nonfinite", 129)
    got = launch(npos, nvel, np.inf, ngoal)
    assert_records(got, Q.batch(npos, nvel, np.inf, ngoal), "radius inf, outliers")
    assert int(got[0]["near"]) == 126 * 125 // 2 and int(got[1]["near"]) == 129 * 128 // 2      # scene 0 has three outliers in its positions


# -- Q7 ----------------------------------------------------------------------------------------------------------------------------------
def test_three_snapshots_in_one_sequence_and_split(nb):
    """three different snapshots of (3, 300) scored into the same records: the restatement's chain; one launch then two equals three"""
    n = 300
    snaps = [K.make(kind, n)[:2] for kind in ("random", "clustered", "planar")]
    _, _, radius_sq, goal = K.make("random", n)
    want = None
    for p, v in snaps:
        want = Q.batch(p, v, radius_sq, goal, acc=want)
    assert (want["steps"] == 3).all()
    got = launch(*snaps[0], radius_sq, goal, others=snaps[1:])
    assert_records(got, want, "three snapshots")
    first = launch(*snaps[0], radius_sq, goal)
    assert_records(first, Q.batch(*snaps[0], radius_sq, goal), "the first of three")
    rest = launch(*snaps[1], radius_sq, goal, start=first, others=snaps[2:])
    assert got.tobytes() == rest.tobytes()
    wrap = np.zeros(3, Q.DTYPE)
    wrap["steps"], wrap["nonfinite"], wrap["near"] = 0xFFFFFFFF, 0xFFFFFFFF, (1 << 40)
    npos, nvel, nr, ng = K.make("nonfinite", 65)
    assert_records(launch(npos, nvel, nr, ng, start=wrap), Q.batch(npos, nvel, nr, ng, acc=wrap), "steps and nonfinite wrap, near is 64 bits")


def test_two_runs_permuted_scenes_and_a_batch_of_one(nb):
    for kind, n in (("large", 2048), ("nonfinite", 1537), ("tiny", 100)):
        pos, vel, radius_sq, goal = K.make(kind, n)
        a, b = launch(pos, vel, radius_sq, goal, snapshots=2), launch(pos, vel, radius_sq, goal, snapshots=2)
        assert a.tobytes() == b.tobytes(), (kind, n)                                     # the same bytes from run to run, NaNs included
        order = [2, 0, 1]
        c = launch(pos[order], vel[order], radius_sq, goal, snapshots=2)
        assert c.tobytes() == a[order].tobytes(), (kind, n)
        for s in range(3):
            one = launch(pos[s:s + 1], vel[s:s + 1], radius_sq, goal, snapshots=2)
            assert one.tobytes() == a[s:s + 1].tobytes(), (kind, n, s)


def test_more_scenes_than_workgroups(nb):
    """2 100 scenes of 5 bodies, more than the grid holds: fifteen distinct scenes cycling, so that a workgroup's second scene differs
    from its first"""
    kinds = ("planar", "random", "clustered", "large", "lattice")
    scenes = [(K.make(kind, 5)[0][s], K.make(kind, 5)[1][s]) for kind in kinds for s in range(3)]
    radius_sq, goal = F(1.5), F([0.5, 0.25, -1.0])
    each = np.stack([Q.accumulate(np.zeros((), Q.DTYPE), Q.terms(p, v, radius_sq, goal)) for p, v in scenes])
    assert len({e.tobytes() for e in each}) == 15 and len(set(each["near"].tolist())) >= 5
    pick = np.arange(2100) % 15
    pos, vel = np.stack([scenes[i][0] for i in pick]), np.stack([scenes[i][1] for i in pick])
    assert_records(launch(pos, vel, radius_sq, goal), each[pick], "2100 scenes")


# -- the context -------------------------------------------------------------------------------------------------------------------------
def test_context_scores_between_mixed_steps(nb):
    """step(1); score(); step_boids(1); score() against the restatement on the downloaded states; then score_reset, a second
    set_score, a sub-range, and an upload that leaves the records as they were"""
    from nenbody_amd import _lib

    n = 129
    pos, vel, radius_sq, goal = K.make("random", n)
    with nb.SceneBatch(pos, vel) as sb:
        sb.set_score(radius_sq, goal)
        assert_records(sb.scores(), np.zeros(3, Q.DTYPE), "cleared")
        sb.score()
        want = Q.batch(pos, vel, radius_sq, goal)
        assert_records(sb.scores(), want, "the uploaded state")
        sb.step(1)
        sb.score()
        p1, v1 = sb.positions(), sb.velocities()
        want = Q.batch(p1, v1, radius_sq, goal, acc=want)
        sb.step_boids(1)
        sb.score()
        p2, v2 = sb.positions(), sb.velocities()
        want = Q.batch(p2, v2, radius_sq, goal, acc=want)
        got = sb.scores()
        assert got.dtype == nb.SCORE_DTYPE and got.shape == (3,) and (got["steps"] == 3).all()
        assert_records(got, want, "gravity, then boids")
        assert sb.scores(1, 2).tobytes() == got[1:].tobytes() and sb.scores(3, 0).shape == (0,) and sb.scores(1).tobytes() == got[1:].tobytes()
        _lib.check(sb._lib.nb_scenes_upload(sb._ctx, pos.ctypes.data, vel.ctypes.data))
        assert sb.scores().tobytes() == got.tobytes()                                    # an upload does not clear
        sb.score()
        assert_records(sb.scores(), Q.batch(pos, vel, radius_sq, goal, acc=want), "after an upload")
        sb.score_reset()
        assert sb.scores().tobytes() == np.zeros(3, Q.DTYPE).tobytes()
        sb.score()
        assert_records(sb.scores(), Q.batch(pos, vel, radius_sq, goal), "after a reset")
        other = (F(0.5) * radius_sq, F([1, -1, 0.5]))
        sb.set_score(*other)                                                             # a second set_score: cleared, new parameters
        assert sb.scores().tobytes() == np.zeros(3, Q.DTYPE).tobytes()
        sb.score()
        assert_records(sb.scores(), Q.batch(pos, vel, *other), "a second set_score")
        assert (sb.scores()["near"] < want["near"]).all()


def test_step_policy_scored_is_step_policy_and_score(nb, oracle):
    """step_policy_scored(2) equals step_policy(1); score() twice, in records and in final state; the records are the restatement's on
    the states between"""
    n, width, features, hidden = 129, 64, 8, 7
    pos, vel = PK.batch(oracle, PK.row(n, width))
    pol = PK.policies(features, hidden, PK.SCENES)
    radius_sq, goal = F(np.median(Q.pair_d2(pos[0])[np.triu_indices(n, 1)])), F([0.01, 0.02, 0.0])
    with nb.SceneBatch(pos, vel) as a, nb.SceneBatch(pos, vel) as b:
        for sb in (a, b):
            sb.set_policy(pol, features, hidden, PK.limit(n, width))
            sb.set_score(radius_sq, goal)
        a.step_policy_scored(2, width)
        want = None
        for _ in range(2):
            b.step_policy(1, width)
            b.score()
            want = Q.batch(b.positions(), b.velocities(), radius_sq, goal, acc=want)
        ra, rb = a.scores(), b.scores()
        assert a.steps_done == b.steps_done == 2 and (ra["steps"] == 2).all()
        assert ra.tobytes() == rb.tobytes()
        assert_records(ra, want, "two scored policy steps")
        assert 0 < int(ra["near"].min()) and int(ra["near"].max()) < 2 * (n * (n - 1) // 2)
        assert a.positions().tobytes() == b.positions().tobytes() and a.velocities().tobytes() == b.velocities().tobytes()
        a.step_policy_scored(0, width)                                                   # k = 0: a checked no-op
        assert a.steps_done == 2 and a.scores().tobytes() == ra.tobytes()


def test_context_entries_refuse_with_their_texts(nb, oracle):
    from nenbody_amd import _lib

    lib = _lib.load()
    cp = np.ascontiguousarray(nb.eye_constant(64), F).reshape(16)
    up, cpp = PK.UP.ctypes.data, cp.ctypes.data
    out = np.zeros(4, Q.DTYPE)
    good = _lib.NbScoreParams(0.25, (ctypes.c_float * 3)(0, 0, 0))
    err = lambda ctx: lib.nb_scenes_last_error(ctx).decode()
    Ss, Sc, Sr, Sd, Sp = ("nb_scenes_set_score: ", "nb_scenes_score: ", "nb_scenes_score_reset: ", "nb_scenes_scores: ",
                          "nb_scenes_step_policy_scored: ")
    upload, unset = "no state uploaded (call nb_scenes_upload first)", "no score set (call nb_scenes_set_score first)"
    no_policy = "no policy set (call nb_scenes_set_policy first)"
    ctx = ctypes.c_void_p()
    _lib.check(lib.nb_scenes_create(3, 8, None, ctypes.byref(ctx)))
    try:
        assert lib.nb_scenes_score(ctx) == _lib.NB_ERR_STATE and err(ctx) == Sc + upload
        assert lib.nb_scenes_score_reset(ctx) == _lib.NB_ERR_STATE and err(ctx) == Sr + unset
        assert lib.nb_scenes_scores(ctx, 0, 3, out.ctypes.data) == _lib.NB_ERR_STATE and err(ctx) == Sd + unset
        assert lib.nb_scenes_step_policy_scored(ctx, 1, up, cpp, 64) == _lib.NB_ERR_STATE and err(ctx) == Sp + upload
        assert lib.nb_scenes_set_score(ctx, ctypes.byref(good)) == _lib.NB_OK                # a score before an upload
        assert lib.nb_scenes_score(ctx) == _lib.NB_ERR_STATE and err(ctx) == Sc + upload
        assert lib.nb_scenes_scores(ctx, 0, 3, out.ctypes.data) == _lib.NB_OK and out[:3].tobytes() == bytes(96)
        assert lib.nb_scenes_score_reset(ctx) == _lib.NB_OK
    finally:
        lib.nb_scenes_destroy(ctx)
    pos, vel = PK.batch(oracle, (1100, 8, 64, 0.1, 3))
    with nb.SceneBatch(pos, vel) as sb:
        c = sb._ctx
        assert lib.nb_scenes_score(c) == _lib.NB_ERR_STATE and err(c) == Sc + unset
        assert lib.nb_scenes_step_policy_scored(c, 1, up, cpp, 64) == _lib.NB_ERR_STATE and err(c) == Sp + no_policy   # step_policy's checks first
        assert lib.nb_scenes_step_policy_scored(c, 1, up, cpp, 0) == _lib.NB_ERR_INVALID
        assert err(c) == Sp + "width must be 1 .. NB_EYES_MAX_WIDTH (4096)"
        sb.set_policy(PK.policies(8, 7, 3), 8, 7, 0.5)
        assert lib.nb_scenes_step_policy_scored(c, 1, up, cpp, 64) == _lib.NB_ERR_STATE and err(c) == Sp + unset
        assert lib.nb_scenes_step_policy_scored(c, 0, up, cpp, 64) == _lib.NB_ERR_STATE and err(c) == Sp + unset       # k = 0 is checked too
        assert lib.nb_scenes_step_policy_scored(c, 1, up, cpp, 60) == _lib.NB_ERR_INVALID and err(c) == Sp + "width must be a multiple of features"
        assert lib.nb_scenes_step_policy_scored(c, 1, None, cpp, 64) == _lib.NB_ERR_INVALID and err(c) == Sp + "null argument"
        assert lib.nb_scenes_set_score(c, None) == _lib.NB_ERR_INVALID and err(c) == Ss + "null argument"
        for radius_sq, goal, text in ((-1.0, (0, 0, 0), "radius_sq must be at least 0 (+inf: every pair)"),
                                      (float("nan"), (0, 0, 0), "radius_sq must be at least 0 (+inf: every pair)"),
                                      (1.0, (0, float("inf"), 0), "goal must be finite"), (1.0, (float("nan"), 0, 0), "goal must be finite"),
                                      (-1.0, (float("nan"), 0, 0), "radius_sq must be at least 0 (+inf: every pair)")):
            bad = _lib.NbScoreParams(radius_sq, (ctypes.c_float * 3)(*goal))
            assert lib.nb_scenes_set_score(c, ctypes.byref(bad)) == _lib.NB_ERR_INVALID and err(c) == Ss + text
        assert lib.nb_scenes_score(c) == _lib.NB_ERR_STATE and err(c) == Sc + unset                                   # a refused score is none
        assert sb.steps_done == 0
        sb.set_score(float("inf"))
        for args, text in (((0, 3, None), "null argument"), ((0, 4, out.ctypes.data), "scenes [first_scene, first_scene + scene_count) exceed the batch"),
                           ((4, 0, out.ctypes.data), "scenes [first_scene, first_scene + scene_count) exceed the batch"),
                           ((0xFFFFFFFF, 2, out.ctypes.data), "scenes [first_scene, first_scene + scene_count) exceed the batch")):
            assert lib.nb_scenes_scores(c, *args) == _lib.NB_ERR_INVALID and err(c) == Sd + text
        assert lib.nb_scenes_scores(c, 3, 0, out.ctypes.data) == _lib.NB_OK                                           # scene_count = 0: a checked no-op
        with pytest.raises(nb.NbError, match="goal must be finite"):
            sb.set_score(1.0, (0, 0, np.inf))
        with pytest.raises(ValueError):
            sb.set_score(1.0, (0, 0))
        with pytest.raises(ValueError):
            sb.scores(-1)
        sb.score()
        assert (sb.scores()["near"] == 8 * 7 // 2).all()
