"""GPU tests of the scene batches' neural policy: the fused kernel of nb_scenes_policy.inc against the numpy
restatement (tests/policy_restatement.py), every word of the features, of the outputs and of every body's position and velocity
(P1-P8); a NaN of the restatement is met by a NaN.

Expected values: per scene the eye rows of the state before the step -- a Scene's own rows (nb_eyes with flags = 0, which is how P1
defines the row, and which tests/test_gpu_eyes.py holds to the numpy eye rule), or the numpy eye rule itself for the hand case --,
then P2-P6 by the restatement.  The cases (n, width, F, H), their batches and their policies are tests/policy_cases.py's;
tests/test_scenes_policy_cpu.py holds their premises."""
import ctypes

import numpy as np
import pytest

import eyes_restatement as R
import policy_cases as K
import policy_restatement as P

pytestmark = pytest.mark.gpu

F = np.float32
UP = K.UP
FILL = 0x07070707


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_words(got, want, what):
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    ok = (bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))
    bad = np.argwhere(~ok)
    assert ok.all(), f"{what}: {len(bad)} words differ, first at {bad[:4].tolist()}: got {g[~ok][:4]}, want {w[~ok][:4]}"


def scene_rows(nb, pos, vel, width):
    """per scene the (ids, depth) rows of a Scene of its bodies"""
    out = []
    for s in range(len(pos)):
        with nb.Scene(pos[s], vel[s]) as sc:
            ids, depth = sc.eyes(width=width)
            out.append((ids.copy(), depth.copy()))
    return out


def restate(nb, pos, vel, pol, features, hidden, limit, width, rows=None, dt=F(0.1)):
    rows = scene_rows(nb, pos, vel, width) if rows is None else rows
    return P.batch(lambda s, p, v: rows[s], pos, vel, pol, features, hidden, limit, UP, dt=dt)


def check_observe_and_steps(nb, pos, vel, pol, features, hidden, limit, width, steps, what, rows=None):
    """observe, then `steps` calls of one step, every word against the restatement; returns the final (positions, velocities)"""
    with nb.SceneBatch(pos, vel) as sb:
        sb.set_policy(pol, features, hidden, limit)
        p0, v0 = pos, vel
        for step in range(steps):
            want_x, want_o, want_p, want_v = restate(nb, p0, v0, pol, features, hidden, limit, width, rows if step == 0 else None)
            if step == 0:
                got_x, got_o = sb.policy_observe(width=width)
                assert_words(got_x, want_x, f"{what}: features")
                assert_words(got_o, want_o, f"{what}: outputs")
                assert sb.steps_done == 0
            sb.step_policy(1, width)
            p0, v0 = sb.positions(), sb.velocities()
            assert_words(p0, want_p, f"{what}: positions after step {step + 1}")
            assert_words(v0, want_v, f"{what}: velocities after step {step + 1}")
        assert sb.steps_done == steps
    return p0, v0


# -- the hand case -----------------------------------------------------------------------------------------------------------------------
def test_hand_case_through_observe_and_step(nb, oracle):
    """policy_cases.hand_policy() on DESIGN.md section 13's two bodies, placed in scene 1 of 3 whose scenes share the policy: the words
    tests/test_scenes_policy_cpu.py derives in exact rationals, here by the restatement on the numpy eye rule's rows"""
    width, features, hidden = K.HAND_SHAPE
    pos, vel = K.batch(oracle, (1100, 2, width, 1.0, 3))
    pos[1], vel[1] = K.HAND_POS, K.HAND_VEL
    rows = []
    for s in range(3):
        cams = oracle.cameras(pos[s], vel[s], UP, R.eye_constant(oracle, width))
        rows.append(R.eyes(cams, oracle.instances(pos[s], vel[s]), 0, width))
    pol = K.hand_policy()[None]
    x = F(1) - np.uint32(K.HAND_DEPTH_BITS).view(F)
    with nb.SceneBatch(pos, vel) as sb:
        sb.set_policy(pol, features, hidden)
        got_x, got_o = sb.policy_observe(width=width)
        assert (bits(got_x[1, 0]) == bits(F([0, 0, 0, x, x, 0, 0, 0]))).all() and (bits(got_x[1, 1]) == 0).all()
        assert (bits(got_o[1, 0]) == bits(F([x + x, x]))).all() and (bits(got_o[1, 1]) == 0).all()
        sb.step_policy(1, width)
        p, v = sb.positions(), sb.velocities()
    want = restate(nb, pos, vel, pol, features, hidden, np.inf, width, rows)
    for got, exp, name in zip((got_x, got_o, p, v), want, ("features", "outputs", "positions", "velocities")):
        assert_words(got, exp, "hand case: " + name)
    want_v = K.HAND_VEL[0] + F([x + x, -x, 0]) * F(0.1)
    assert (bits(v[1, 0]) == bits(want_v)).all() and (bits(p[1, 0]) == bits(want_v + K.HAND_POS[0])).all() and v[1, 0, 0] > 1 > 0 > v[1, 0, 1]
    assert (bits(v[1, 1]) == bits(K.HAND_VEL[1])).all() and (bits(p[1, 1]) == bits(F([11, 0, 0]))).all()       # eye 1 sees nothing: it coasts


# -- seeded batches ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,width", [(n, w) for n in K.SIZES for w in K.WIDTHS])
def test_seeded_batches_own_and_shared_policies(nb, oracle, n, width):
    """B = 3; every (F, H) of the case list at this (n, width); a policy per scene, then the same batch with policy 0 for all: observe,
    then two steps"""
    pos, vel = K.batch(oracle, K.row(n, width))
    rows = scene_rows(nb, pos, vel, width)
    cases = [c for c in K.CASES if c[:2] == (n, width)]
    assert cases
    for _, _, features, hidden in cases:
        own = K.policies(features, hidden, K.SCENES)
        ends = []
        for pol in (own, own[:1]):
            what = f"n={n} W={width} F={features} H={hidden} policies={len(pol)}"
            ends.append(check_observe_and_steps(nb, pos, vel, pol, features, hidden, K.limit(n, width), width, 2, what, rows))
        assert (bits(ends[0][1][0]) == bits(ends[1][1][0])).all()          # scene 0 has policy 0 either way
        assert (bits(ends[0][1][1:]) != bits(ends[1][1][1:])).any()        # the others have not


def test_a_zero_velocity_a_body_along_up_a_non_finite_velocity_and_a_nan_weight(nb, oracle):
    pos, vel = K.special_scene()
    pol = K.policies(8, 7, 1)
    p1, v1 = check_observe_and_steps(nb, pos, vel, pol, 8, 7, K.LIMIT, 64, 1, "special scene")
    for body in (1, 2, 3):                                                 # P5's guard: they coast
        assert (bits(v1[0, body]) == bits(vel[0, body])).all(), body
    assert all((bits(v1[0, body]) != bits(vel[0, body])).any() for body in (0, 4, 5))
    for at in (3, 8 * 7 + 7 + 2):                                          # a NaN in w1 (P3 gives +0), a NaN in w2 (it passes the limit)
        nan = pol.copy()
        nan[0, at] = np.nan
        p2, v2 = check_observe_and_steps(nb, pos, vel, nan, 8, 7, K.LIMIT, 64, 1, f"special scene, NaN weight {at}")
        assert np.isnan(v2[0, 0]).any() == (at != 3) and (bits(v2[0, 1]) == bits(vel[0, 1])).all()


# -- P7 ----------------------------------------------------------------------------------------------------------------------------------
def test_k_steps_are_k_calls_two_runs_and_permuted_scenes(nb, oracle):
    n, width, features, hidden = 129, 64, 8, 7
    pos, vel = K.batch(oracle, K.row(n, width))
    pol = K.policies(features, hidden, K.SCENES)
    limit = K.limit(n, width)
    want = check_observe_and_steps(nb, pos, vel, pol, features, hidden, limit, width, 2, "two calls of one step")

    def run(order, k):
        with nb.SceneBatch(pos[order], vel[order]) as sb:
            sb.set_policy(pol[order], features, hidden, limit)
            sb.step_policy(k, width)
            assert sb.steps_done == k
            return sb.positions(), sb.velocities()

    same = [0, 1, 2]
    first, again = run(same, 2), run(same, 2)
    for got, name in zip(first, ("positions", "velocities")):
        assert_words(got, want[name == "velocities"], "k = 2 in one call: " + name)
    assert (bits(first[0]) == bits(again[0])).all() and (bits(first[1]) == bits(again[1])).all()      # the same bits from run to run
    order = [2, 0, 1]
    moved = run(order, 2)
    assert (bits(moved[0]) == bits(first[0][order])).all() and (bits(moved[1]) == bits(first[1][order])).all()
    assert (bits(first[1][0]) != bits(first[1][1])).any()
    alone = run([1], 2)                                                    # a batch of one scene: `scenes` does not enter
    assert (bits(alone[0][0]) == bits(first[0][1])).all() and (bits(alone[1][0]) == bits(first[1][1])).all()


# -- the extremes ------------------------------------------------------------------------------------------------------------------------
def test_the_lds_extreme(nb, oracle):
    """n = 2 048, W = 4 096, F = 256, H = 64, B = 1: 34 048 bytes of LDS a workgroup"""
    n, width, features, hidden = 2048, 4096, 256, 64
    pos, vel = K.batch(oracle, (5, n, width, 1.0, 1))
    pol = K.policies(features, hidden, 1)
    check_observe_and_steps(nb, pos, vel, pol, features, hidden, K.LIMIT, width, 1, "the LDS extreme")


def test_more_eyes_than_the_grid_cap(nb, oracle):
    """524 300 scenes of n = 2, W = 8, F = 1, H = 1: 1 048 600 eyes, more than the 2^20 workgroups a launch has at most, so some
    workgroups take a second eye, which must start from clean LDS.  The batch cycles through four distinct scenes, each with its own
    policy; every copy must get its restated original's words"""
    n, width, distinct, b = 2, 8, 4, 524300
    assert b * n > 1 << 20
    pos4 = np.array([[[0, 0, 0], [d, 0, 0]] for d in (2.5, 4, 6, 10)], F)
    vel4 = np.tile(F([1, 0, 0]), (distinct, n, 1))
    pol4 = K.policies(1, 1, distinct)
    want = restate(nb, pos4, vel4, pol4, 1, 1, K.LIMIT, width)
    assert (want[0][:, 0, 0] > 0).all() and (want[0][:, 1, 0] == 0).all()         # eye 0 of every scene sees body 1, eye 1 nobody
    assert len({tuple(bits(v).reshape(-1)) for v in want[3]}) == distinct
    reps = -(-b // distinct)
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:b]
    with nb.SceneBatch(tile(pos4), tile(vel4)) as sb:
        sb.set_policy(tile(pol4), 1, 1, K.LIMIT)
        sb.step_policy(1, width)
        got_p, got_v = sb.positions(), sb.velocities()
    assert (bits(got_p) == bits(tile(want[2]))).all() and (bits(got_v) == bits(tile(want[3]))).all()


# -- the context, mixed with the other steps -----------------------------------------------------------------------------------------------
def test_round_trip_mixed_with_step(nb, oracle):
    """step(1), step_policy(1), step(1), a second set_policy, step_policy(1): per scene a Scene's own step for the gravity steps and
    the restatement for the policy's"""
    n, width = 100, 1024
    pos, vel = K.batch(oracle, (1100, n, width, 1.0, 3))
    first, second = K.policies(8, 7, 3), K.policies(64, 1, 1, seed=8)

    def gravity(p, v):
        out = []
        for s in range(len(p)):
            with nb.Scene(p[s], v[s]) as sc:
                sc.step_n(1)
                out.append(sc.state())
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    p, v = gravity(pos, vel)
    _, _, p, v = restate(nb, p, v, first, 8, 7, K.LIMIT, width)
    p, v = gravity(p, v)
    want_x, want_o, p, v = restate(nb, p, v, second, 64, 1, np.inf, width)
    with nb.SceneBatch(pos, vel) as sb:
        sb.set_policy(first, 8, 7, K.LIMIT)
        sb.step(1)
        sb.step_policy(1, width)
        sb.step(1)
        sb.set_policy(second, 64, 1)
        got_x, got_o = sb.policy_observe(width=width)
        sub_x, sub_o = sb.policy_observe(first_scene=1, scene_count=2, width=width)
        none_x, none_o = sb.policy_observe(first_scene=3, scene_count=0, width=width)
        sb.step_policy(1, width)
        assert sb.steps_done == 4
        got_p, got_v = sb.positions(), sb.velocities()
    assert_words(got_x, want_x, "mixed: features")
    assert_words(got_o, want_o, "mixed: outputs")
    assert (bits(sub_x) == bits(got_x[1:])).all() and (bits(sub_o) == bits(got_o[1:])).all()
    assert none_x.shape == (0, n, 64) and none_o.shape == (0, n, 2)
    assert_words(got_p, p, "mixed: positions")
    assert_words(got_v, v, "mixed: velocities")


# -- the stateless launches ----------------------------------------------------------------------------------------------------------------
def records_of(a):
    r = np.zeros(a.shape[:-1] + (4,), F)
    r[..., :3] = a
    return r.reshape(-1, 4)


@pytest.mark.parametrize("n,policies", [(100, 3), (129, 1)])
def test_stateless_launches_between_guards(nb, oracle, n, policies):
    """nb_scenes_policy_step_launch: pos_out and vel_out lie inside tensors with one scene of NaN records in front and one behind; the
    guards come back bit for bit, the inputs are unmodified, and what lies between is the step.  nb_scenes_policy_observe_launch over
    a range of eyes that starts and ends inside a scene: every word of the outputs is written and none beyond"""
    import torch

    from nenbody_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    width, features, hidden, b = 1024, 8, 7, 3
    pos, vel = K.batch(oracle, (1100, n, width, 1.0, b))
    pol = K.policies(features, hidden, policies)
    want_x, want_o, want_p, want_v = restate(nb, pos, vel, pol, features, hidden, K.LIMIT, width)
    t_pos, t_vel = torch.from_numpy(records_of(pos)).to(dev), torch.from_numpy(records_of(vel)).to(dev)
    t_pol = torch.from_numpy(pol).to(dev)
    guard = np.full(((b + 2) * n, 4), np.uint32(0x7FC0BEEF).view(F), F)
    o_pos, o_vel = torch.from_numpy(guard.copy()).to(dev), torch.from_numpy(guard.copy()).to(dev)
    cpm = np.ascontiguousarray(nb.eye_constant(width), F).reshape(16)
    records = b * n
    cams = torch.empty((records, 16), dtype=torch.float32, device=dev)
    inst = torch.empty((records, 16), dtype=torch.float32, device=dev)
    first, count = n // 2, records - n // 2 - 7
    feat = torch.full((count + 1, features), FILL, dtype=torch.int32, device=dev)
    act = torch.full((count + 1, 2), FILL, dtype=torch.int32, device=dev)
    only = torch.full((count + 1, 2), FILL, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        _lib.check(lib.nb_launch_instances(records, t_pos.data_ptr(), t_vel.data_ptr(), inst.data_ptr(), s.cuda_stream))
        _lib.check(lib.nb_launch_cameras(records, t_pos.data_ptr(), t_vel.data_ptr(), UP.ctypes.data, cpm.ctypes.data, cams.data_ptr(),
                                         s.cuda_stream))
        _lib.check(lib.nb_scenes_policy_step_launch(None, b, n, cams.data_ptr(), inst.data_ptr(), width, UP.ctypes.data, features, hidden,
                                                    policies, t_pol.data_ptr(), float(K.LIMIT), t_pos.data_ptr(), t_vel.data_ptr(),
                                                    o_pos.data_ptr() + 16 * n, o_vel.data_ptr() + 16 * n, s.cuda_stream))
        _lib.check(lib.nb_scenes_policy_observe_launch(b, n, first, count, cams.data_ptr(), inst.data_ptr(), width, features, hidden, policies,
                                                       t_pol.data_ptr(), float(K.LIMIT), feat.data_ptr(), act.data_ptr(), s.cuda_stream))
        _lib.check(lib.nb_scenes_policy_observe_launch(b, n, first, count, cams.data_ptr(), inst.data_ptr(), width, features, hidden, policies,
                                                       t_pol.data_ptr(), float(K.LIMIT), None, only.data_ptr(), s.cuda_stream))
    s.synchronize()
    gp, gv = o_pos.cpu().numpy(), o_vel.cpu().numpy()
    for got in (gp, gv):
        assert (bits(got[:n]) == 0x7FC0BEEF).all() and (bits(got[-n:]) == 0x7FC0BEEF).all()
        assert (bits(got[n:-n, 3]) == 0).all()
    assert_words(gp[n:-n, :3], want_p.reshape(-1, 3), "stateless: positions")
    assert_words(gv[n:-n, :3], want_v.reshape(-1, 3), "stateless: velocities")
    assert (bits(t_pos.cpu().numpy()) == bits(records_of(pos))).all() and (bits(t_vel.cpu().numpy()) == bits(records_of(vel))).all()
    g_feat, g_act, g_only = (t.cpu().numpy().view(np.uint32) for t in (feat, act, only))
    assert (g_feat[:count] == bits(want_x.reshape(-1, features)[first:first + count])).all() and (g_feat[count] == FILL).all()
    assert (g_act[:count] == bits(want_o.reshape(-1, 2)[first:first + count])).all() and (g_act[count] == FILL).all()
    assert (g_only == g_act).all()


# -- the context's refusals that need a device --------------------------------------------------------------------------------------------
def test_context_entries_refuse_with_their_texts(nb, oracle):
    from nenbody_amd import _lib

    lib = _lib.load()
    cp = np.ascontiguousarray(nb.eye_constant(64), F).reshape(16)
    up, cpp = UP.ctypes.data, cp.ctypes.data
    pol = K.policies(8, 7, 3)
    w = pol.ctypes.data
    feat, act = np.zeros(3 * 8 * 8, F), np.zeros(3 * 8 * 2 + 2, F)
    err = lambda ctx: lib.nb_scenes_last_error(ctx).decode()
    Sp, St, Ey = "nb_scenes_set_policy: ", "nb_scenes_step_policy: ", "nb_scenes_eyes_policy: "
    upload, unset = "no state uploaded (call nb_scenes_upload first)", "no policy set (call nb_scenes_set_policy first)"
    ctx = ctypes.c_void_p()
    _lib.check(lib.nb_scenes_create(3, 8, None, ctypes.byref(ctx)))
    try:
        assert lib.nb_scenes_step_policy(ctx, 1, up, cpp, 64) == _lib.NB_ERR_STATE and err(ctx) == St + upload
        assert lib.nb_scenes_eyes_policy(ctx, 0, 3, up, cpp, 64, feat.ctypes.data, act.ctypes.data) == _lib.NB_ERR_STATE and err(ctx) == Ey + unset
        assert lib.nb_scenes_set_policy(ctx, 8, 7, 3, w, 0.5) == _lib.NB_OK                          # a policy before an upload
        assert lib.nb_scenes_step_policy(ctx, 1, up, cpp, 64) == _lib.NB_ERR_STATE and err(ctx) == St + upload
        assert lib.nb_scenes_eyes_policy(ctx, 0, 3, up, cpp, 64, feat.ctypes.data, act.ctypes.data) == _lib.NB_ERR_STATE and err(ctx) == Ey + upload
        assert lib.nb_scenes_step_policy(ctx, 1, up, cpp, 0) == _lib.NB_ERR_INVALID                  # the eye set-up comes first
        assert err(ctx) == St + "width must be 1 .. NB_EYES_MAX_WIDTH (4096)"
    finally:
        lib.nb_scenes_destroy(ctx)
    pos, vel = K.batch(oracle, (1100, 8, 64, 0.1, 3))
    with nb.SceneBatch(pos, vel) as sb:
        c = sb._ctx
        assert lib.nb_scenes_step_policy(c, 1, up, cpp, 64) == _lib.NB_ERR_STATE and err(c) == St + unset
        assert lib.nb_scenes_step_policy(c, 0, up, cpp, 64) == _lib.NB_ERR_STATE and err(c) == St + unset          # k = 0 is checked too
        for args, text in (((8, 7, 3, None, 0.5), "null argument"), ((0, 7, 3, w, 0.5), "features must be 1 .. NB_POLICY_MAX_FEATURES (256)"),
                           ((257, 7, 3, w, 0.5), "features must be 1 .. NB_POLICY_MAX_FEATURES (256)"),
                           ((8, 0, 3, w, 0.5), "hidden must be 1 .. NB_POLICY_MAX_HIDDEN (64)"), ((8, 65, 3, w, 0.5), "hidden must be 1 .. NB_POLICY_MAX_HIDDEN (64)"),
                           ((8, 7, 2, w, 0.5), "policies must be 1 or scenes"), ((8, 7, 0, w, 0.5), "policies must be 1 or scenes"),
                           ((8, 7, 3, w, -0.5), "accel_limit must be at least 0 (+inf: no limit)"),
                           ((8, 7, 3, w, float("nan")), "accel_limit must be at least 0 (+inf: no limit)"),
                           ((8, 65, 2, w, -1.0), "hidden must be 1 .. NB_POLICY_MAX_HIDDEN (64)")):
            assert lib.nb_scenes_set_policy(c, *args) == _lib.NB_ERR_INVALID, args
            assert err(c) == Sp + text
        assert lib.nb_scenes_step_policy(c, 1, up, cpp, 64) == _lib.NB_ERR_STATE and err(c) == St + unset          # a refused policy is none
        sb.set_policy(pol, 8, 7, 0.5)
        for args, text in (((1, None, cpp, 64), "null argument"), ((1, up, None, 64), "null argument"),
                           ((1, up, cpp, 4097), "width must be 1 .. NB_EYES_MAX_WIDTH (4096)"), ((1, up, cpp, 0), "width must be 1 .. NB_EYES_MAX_WIDTH (4096)"),
                           ((1, up, cpp, 60), "width must be a multiple of features"), ((0, up, cpp, 60), "width must be a multiple of features")):
            assert lib.nb_scenes_step_policy(c, *args) == _lib.NB_ERR_INVALID, args
            assert err(c) == St + text
        assert sb.steps_done == 0
        f, a = feat.ctypes.data, act.ctypes.data
        for args, text in (((0, 3, None, cpp, 64, f, a), "null argument"), ((0, 3, up, cpp, 0, f, a), "width must be 1 .. NB_EYES_MAX_WIDTH (4096)"),
                           ((0, 3, up, cpp, 60, f, a), "width must be a multiple of features"),
                           ((1, 3, up, cpp, 64, f, a), "scenes [first_scene, first_scene + scene_count) exceed the batch"),
                           ((0, 3, up, cpp, 64, None, None), "feat_out and act_out are both NULL"),
                           ((0, 3, up, cpp, 64, f, f + 4), "the outputs must not overlap each other or an input")):
            assert lib.nb_scenes_eyes_policy(c, *args) == _lib.NB_ERR_INVALID, args
            assert err(c) == Ey + text
        assert lib.nb_scenes_step_policy(c, 0, up, cpp, 64) == _lib.NB_OK and sb.steps_done == 0                  # k = 0: a checked no-op
        assert lib.nb_scenes_eyes_policy(c, 0, 3, up, cpp, 64, f, None) == _lib.NB_OK                            # one output is enough
        assert lib.nb_scenes_eyes_policy(c, 0, 3, up, cpp, 64, None, a) == _lib.NB_OK
        with pytest.raises(nb.NbError, match="width must be a multiple of features"):
            sb.step_policy(1, 60)
        with pytest.raises(ValueError):
            sb.set_policy(pol[:, :-1], 8, 7)
