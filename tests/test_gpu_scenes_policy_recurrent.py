"""GPU tests of the scene batches' recurrent policy: the fused kernel of nb_scenes_policy_recurrent.inc
against the numpy restatement (tests/policy_recurrent_restatement.py), every word of the features, of the outputs, of the memory and
of every body's position and velocity (R1-R8); a NaN of the restatement is met by a NaN.

Expected values: per scene the eye rows of the state before the step -- a Scene's own rows (nb_eyes with flags = 0, which is how P1
defines the row, and which tests/test_gpu_eyes.py holds to the numpy eye rule) --, then R2-R5 by the restatement, the memory carried
from step to step.  The cases (n, width, F, H), their batches, their policies and their memory limits are
tests/policy_recurrent_cases.py's; tests/test_scenes_policy_recurrent_cpu.py holds their premises."""
import ctypes

import numpy as np
import pytest

import es_cases as EK
import es_restatement as E
import policy_recurrent_cases as C
import policy_recurrent_restatement as RR
import policy_restatement as P
import score_restatement as Q
from nenbody_amd._lib import SCENES_POLICY_RECURRENT_PROTOTYPES   # noqa: F401  (the parent commit has no such table: the file fails here)

pytestmark = pytest.mark.gpu

F = np.float32
UP = C.UP
FILL = 0x07070707
NAN_GUARD = 0x7FC0BEEF


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_words(got, want, what):
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    ok = (bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))
    bad = np.argwhere(~ok)
    assert ok.all(), f"{what}: {len(bad)} words differ, first at {bad[:4].tolist()}: got {g[~ok][:4]}, want {w[~ok][:4]}"


def rows_by(nb, width):
    """rows_of for the restatement: a Scene's own rows of the scene's bodies"""
    def rows_of(s, pos, vel):
        with nb.Scene(pos, vel) as sc:
            ids, depth = sc.eyes(width=width)
            return ids.copy(), depth.copy()
    return rows_of


def check_steps(nb, pos, vel, pol, features, hidden, limit, memory_limit, width, steps, what, mem=None, observe=True):
    """set_policy_recurrent, an optional set_memory, then observe and `steps` calls of one step, every word against the restatement;
    returns the final (positions, velocities, memory)"""
    m0 = np.zeros(pos.shape[:2] + (hidden,), F) if mem is None else mem
    want = RR.rollout(rows_by(nb, width), pos, vel, m0, pol, features, hidden, limit, memory_limit, UP, steps)
    with nb.SceneBatch(pos, vel) as sb:
        sb.set_policy_recurrent(pol, features, hidden, limit, memory_limit)
        if mem is not None:
            sb.set_memory(mem)
        assert bits(sb.memory()).tobytes() == bits(m0).tobytes()
        for step, (want_x, want_o, want_m, want_p, want_v) in enumerate(want):
            if observe and step in (0, steps - 1):
                before = bits(sb.memory()).tobytes()
                got_x, got_o, got_m = sb.policy_observe_memory(width=width)
                two_x, two_o = sb.policy_observe(width=width)
                assert_words(got_x, want_x, f"{what}: features at step {step + 1}")
                assert_words(got_o, want_o, f"{what}: outputs at step {step + 1}")
                assert_words(got_m, want_m, f"{what}: observed memory at step {step + 1}")
                assert bits(two_x).tobytes() == bits(got_x).tobytes() and bits(two_o).tobytes() == bits(got_o).tobytes()
                assert bits(sb.memory()).tobytes() == before and sb.steps_done == step      # R8: nothing stepped, the memory's bytes unchanged
            sb.step_policy(1, width)
            assert_words(sb.positions(), want_p, f"{what}: positions after step {step + 1}")
            assert_words(sb.velocities(), want_v, f"{what}: velocities after step {step + 1}")
            assert_words(sb.memory(), want_m, f"{what}: memory after step {step + 1}")
        assert sb.steps_done == steps
    return want[-1][3], want[-1][4], want[-1][2]


# -- every case ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,width", [(n, w) for n in C.SIZES for w in C.WIDTHS])
def test_three_steps_of_every_case_own_and_shared_policies(nb, oracle, n, width):
    """B = 3; every (F, H) of the case list at this (n, width); a policy per scene under S, then policy 0 for all without a memory
    limit: observe, then three steps, so that memory written by step 1 is read by step 2 and overwritten in place by step 3"""
    pos, vel = C.batch(oracle, C.row(n, width))
    cases = [c for c in C.CASES if c[:2] == (n, width)]
    assert len(cases) == 6
    for _, _, features, hidden in cases:
        own = C.policies(features, hidden, C.SCENES)
        ends = []
        for pol in (own, own[:1]):
            what = f"n={n} W={width} F={features} H={hidden} policies={len(pol)}"
            ends.append(check_steps(nb, pos, vel, pol, features, hidden, C.limit(n, width), C.memory_limit(len(pol) > 1), width, C.STEPS, what))
        assert (bits(ends[0][2]) != bits(ends[1][2])).any()


@pytest.mark.parametrize("n,width", [(n, w) for n in C.SIZES for w in C.WIDTHS])
def test_a_zero_wr_is_the_feedforward_kernel_bit_for_bit(nb, oracle, n, width):
    """R6 on every case against the EXISTING feedforward kernel on the device: set_policy + step_policy of (w1, b1, w2, b2) and
    set_policy_recurrent + step_policy of the same with every word of wr +0 give the same positions and velocities on each of three
    steps, and the same x and o"""
    pos, vel = C.batch(oracle, C.row(n, width))
    for _, _, features, hidden in [c for c in C.CASES if c[:2] == (n, width)]:
        for count in (C.SCENES, 1):
            pol = C.policies(features, hidden, count, zero_wr=True)
            with nb.SceneBatch(pos, vel) as ff, nb.SceneBatch(pos, vel) as rec:
                ff.set_policy(C.feedforward(pol, features, hidden), features, hidden, C.limit(n, width))
                rec.set_policy_recurrent(pol, features, hidden, C.limit(n, width), C.memory_limit(count > 1))
                for step in range(C.STEPS):
                    for a, b in zip(ff.policy_observe(width=width), rec.policy_observe(width=width)):
                        assert bits(a).tobytes() == bits(b).tobytes(), (n, width, features, hidden, count, step)
                    ff.step_policy(1, width)
                    rec.step_policy(1, width)
                    assert bits(ff.positions()).tobytes() == bits(rec.positions()).tobytes(), (n, width, features, hidden, count, step)
                    assert bits(ff.velocities()).tobytes() == bits(rec.velocities()).tobytes(), (n, width, features, hidden, count, step)
                assert (bits(rec.memory()) != 0).any() and (bits(ff.velocities()) != bits(vel)).any()


def test_the_special_scene_and_special_words_in_the_memory(nb, oracle):
    """a zero velocity, a body along up and a non-finite velocity coast and still take their new memory; then NaN, +inf, -inf and -0 in
    the memory, uploaded through set_memory, through the step and through observe"""
    pos, vel = C.special_scene()
    pol = C.policies(8, 7, 1)
    p1, v1, m1 = check_steps(nb, pos, vel, pol, 8, 7, C.LIMIT, C.MEMORY_LIMIT, 64, 2, "special scene")
    for body in (1, 2, 3):
        assert (bits(v1[0, body]) == bits(vel[0, body])).all() and (bits(m1[0, body]) != 0).any(), body
    mem = np.zeros((1, 6, 7), F)
    mem[0, 0, :4] = [np.nan, np.inf, -np.inf, -0.0]
    mem[0, 4] = [-0.0, 1.5, np.inf, 2.0 ** -140, -2.0, 0.5, 0.25]         # no NaN: +inf and -inf terms meet in some units and not in others
    mem[0, 1, 2] = np.inf                                                  # a coasting body
    mem[0, 5] = -0.0
    for s_lim in (C.MEMORY_LIMIT, np.inf):
        _, _, m2 = check_steps(nb, pos, vel, pol, 8, 7, C.LIMIT, s_lim, 64, 2, f"special words, S={s_lim}", mem=mem)
        assert not np.isnan(m2).any() and m2.min() >= 0 and m2.max() <= s_lim   # R4: m' lies in [+0, S] whatever the old memory held


# -- R7 ------------------------------------------------------------------------------------------------------------------------------------
def test_k_steps_are_k_calls_two_runs_permuted_scenes_and_a_batch_of_one(nb, oracle):
    n, width, features, hidden = 129, 64, 8, 7
    pos, vel = C.batch(oracle, C.row(n, width))
    pol = C.policies(features, hidden, C.SCENES)
    limit = C.limit(n, width)
    want = check_steps(nb, pos, vel, pol, features, hidden, limit, C.MEMORY_LIMIT, width, 3, "three calls of one step", observe=False)

    def run(order, k):
        with nb.SceneBatch(pos[order], vel[order]) as sb:
            sb.set_policy_recurrent(pol[order], features, hidden, limit, C.MEMORY_LIMIT)
            sb.step_policy(k, width)
            assert sb.steps_done == k
            return sb.positions(), sb.velocities(), sb.memory()

    same = [0, 1, 2]
    first, again = run(same, 3), run(same, 3)
    for got, exp, name in zip(first, want, ("positions", "velocities", "memory")):
        assert_words(got, exp, "k = 3 in one call: " + name)
    assert all(bits(a).tobytes() == bits(b).tobytes() for a, b in zip(first, again))                  # the same bytes from run to run
    order = [2, 0, 1]
    moved = run(order, 3)
    assert all(bits(m).tobytes() == bits(f[order]).tobytes() for m, f in zip(moved, first))
    assert (bits(first[2][0]) != bits(first[2][1])).any()
    alone = run([1], 3)                                                    # a batch of one scene: `scenes` does not enter
    assert all(bits(a[0]).tobytes() == bits(f[1]).tobytes() for a, f in zip(alone, first))


# -- what memory means ---------------------------------------------------------------------------------------------------------------------
def test_a_body_remembers_whom_it_saw(nb, oracle):
    """the meaning case of tests/test_scenes_policy_recurrent_cpu.py on the device: m_0 of body 0 is +0 before body 1 crosses its slit,
    1.0 during the crossing and 1.0 on every step after the row is empty again, where the feedforward h_0 is back at +0"""
    width, features, hidden = C.MEANING_SHAPE
    pol = C.meaning_policy()[None]
    w1 = RR.unpack(pol[0], features, hidden)[0]
    seen, memory = [], []
    with nb.SceneBatch(C.MEANING_POS[None], C.MEANING_VEL[None]) as sb:
        sb.set_policy_recurrent(pol, features, hidden, np.inf, 1.0)
        for t in range(C.MEANING_STEPS):
            x, o, _ = sb.policy_observe_memory(width=width)
            seen.append(bool((x[0, 0] > 0).any()))
            h_forward = P.hidden_of(x[0], w1, np.zeros(1, F))[0, 0]
            assert (h_forward > 1) == seen[-1] and (seen[-1] or bits(h_forward) == 0) and (bits(o) == 0).all()
            sb.step_policy(1, width)
            memory.append(sb.memory()[0])
        assert (bits(sb.velocities()[0]) == bits(C.MEANING_VEL)).all()     # straight lines
        assert (bits(sb.positions()[0]) == bits((C.MEANING_POS + F(C.MEANING_STEPS) * C.MEANING_VEL).astype(F))).all()
    first, last = seen.index(True), len(seen) - 1 - seen[::-1].index(True)
    assert 0 < first <= last < len(seen) - 2 and all(seen[first:last + 1]), seen
    for t, m in enumerate(memory):
        assert bits(m[0, 0]) == (0 if t < first else bits(F(1))) and bits(m[1, 0]) == 0, (t, seen)


# -- the context's memory --------------------------------------------------------------------------------------------------------------------
def test_memory_reset_round_trip_and_the_way_back_to_a_feedforward_policy(nb, oracle):
    n, width, features, hidden = 5, 8, 8, 7
    pos, vel = C.batch(oracle, C.row(n, width))
    pol = C.policies(features, hidden, C.SCENES)
    forward = C.feedforward(pol, features, hidden)
    rng = np.random.default_rng(5)
    words = rng.integers(0, 1 << 32, (C.SCENES, n, hidden), dtype=np.uint64).astype(np.uint32)        # any bit patterns
    with nb.SceneBatch(pos, vel) as ff:
        ff.set_policy(forward, features, hidden, C.LIMIT)
        ff.step_policy(1, width)
        ff_p, ff_v = ff.positions(), ff.velocities()
    with nb.SceneBatch(pos, vel) as sb:
        sb.set_policy_recurrent(pol, features, hidden, C.LIMIT, C.MEMORY_LIMIT)
        assert (bits(sb.memory()) == 0).all()                              # all +0 initially
        sb.set_memory(words.view(F))
        assert sb.memory().view(np.uint32).tobytes() == words.tobytes()    # a round trip, NaN payloads included
        assert sb.memory(1, 2).view(np.uint32).tobytes() == words[1:].tobytes() and sb.memory(3, 0).shape == (0, n, hidden)
        sb.memory_reset()
        assert (bits(sb.memory()) == 0).all()
        sb.step_policy(1, width)
        stepped = sb.memory()
        assert (bits(stepped) != 0).any()
        sb.step(1)                                                         # the other laws leave the memory alone
        sb.keep()
        sb.step_policy(1, width)
        after = sb.memory()
        sb.rewind()                                                        # and so do keep and rewind
        assert bits(sb.memory()).tobytes() == bits(after).tobytes() != bits(stepped).tobytes()
        from nenbody_amd import _lib
        _lib.check(sb._lib.nb_scenes_upload(sb._ctx, pos.ctypes.data, vel.ctypes.data))
        assert bits(sb.memory()).tobytes() == bits(after).tobytes()        # an upload does not clear the memory
        sb.set_policy_recurrent(pol, features, hidden, C.LIMIT, C.MEMORY_LIMIT)
        assert (bits(sb.memory()) == 0).all()                              # set_policy_recurrent does
        sb.set_policy(forward, features, hidden, C.LIMIT)                  # back to the feedforward kernel
        sb.step_policy(1, width)
        assert bits(sb.positions()).tobytes() == bits(ff_p).tobytes() and bits(sb.velocities()).tobytes() == bits(ff_v).tobytes()
        with pytest.raises(nb.NbError, match="call nb_scenes_set_policy_recurrent first"):
            sb.memory()


# -- the extremes ----------------------------------------------------------------------------------------------------------------------------
def test_the_lds_extreme(nb, oracle):
    """n = 2 048, W = 4 096, F = 256, H = 64, B = 1, two steps: 34 304 bytes of LDS a workgroup"""
    n, width, features, hidden = 2048, 4096, 256, 64
    pos, vel = C.batch(oracle, (5, n, width, 1.0, 1))
    pol = C.policies(features, hidden, 1)
    check_steps(nb, pos, vel, pol, features, hidden, C.LIMIT, C.MEMORY_LIMIT, width, 2, "the LDS extreme", observe=False)


def test_more_eyes_than_the_grid_cap(nb, oracle):
    """524 300 scenes of n = 2, W = 8, F = 1, H = 2: 1 048 600 eyes, more than the 2^20 workgroups a launch has at most, so some
    workgroups take a second eye, which must start from clean LDS and its own memory.  The batch cycles through four distinct scenes,
    each with its own policy; every copy must get its restated original's words, 8 MB of memory among them, on both of two steps"""
    n, width, distinct, b, hidden = 2, 8, 4, 524300, 2
    assert b * n > 1 << 20
    pos4 = np.array([[[0, 0, 0], [d, 0, 0]] for d in (2.5, 4, 6, 10)], F)
    vel4 = np.tile(F([1, 0, 0]), (distinct, n, 1))
    pol4 = C.policies(1, hidden, distinct)
    want = RR.rollout(rows_by(nb, width), pos4, vel4, np.zeros((distinct, n, hidden), F), pol4, 1, hidden, C.LIMIT, np.inf, UP, 2)
    assert (want[0][0][:, 0, 0] > 0).all() and (want[0][0][:, 1, 0] == 0).all()       # eye 0 of every scene sees body 1, eye 1 nobody
    assert len({tuple(bits(m).reshape(-1)) for m in want[1][2]}) == distinct and (bits(want[0][2]) != bits(want[1][2])).any()
    reps = -(-b // distinct)
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:b]
    with nb.SceneBatch(tile(pos4), tile(vel4)) as sb:
        sb.set_policy_recurrent(tile(pol4), 1, hidden, C.LIMIT, np.inf)
        sb.step_policy(2, width)
        got_p, got_v, got_m = sb.positions(), sb.velocities(), sb.memory()
    assert (bits(got_p) == bits(tile(want[1][3]))).all() and (bits(got_v) == bits(tile(want[1][4]))).all()
    assert (bits(got_m) == bits(tile(want[1][2]))).all()


# -- the stateless launches ----------------------------------------------------------------------------------------------------------------
def records_of(a):
    r = np.zeros(a.shape[:-1] + (4,), F)
    r[..., :3] = a
    return r.reshape(-1, 4)


@pytest.mark.parametrize("n,policies", [(100, 3), (129, 1)])
def test_stateless_launches_between_guards(nb, oracle, n, policies):
    """nb_scenes_policy_recurrent_step_launch with the memory out of place (mem_out between guard words, mem_in unmodified) and in
    place (the memory between guard words), both from a memory that is not zero; nb_scenes_policy_recurrent_observe_launch over a range
    of eyes that starts and ends inside a scene: every word of the outputs is written, none beyond, and the memory's bytes stay"""
    import torch

    from nenbody_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    width, features, hidden, b = 64, 8, 7, 3
    pos, vel = C.batch(oracle, (1100, n, width, 0.1, b))
    pol = C.policies(features, hidden, policies)
    limit, s_lim = C.limit(n, width), C.MEMORY_LIMIT
    records = b * n
    mem = np.random.default_rng(11).uniform(0, 2 * float(s_lim), (b, n, hidden)).astype(F)
    want_x, want_o, want_m, want_p, want_v = RR.batch(rows_by(nb, width), pos, vel, mem, pol, features, hidden, limit, s_lim, UP)
    t_pos, t_vel = torch.from_numpy(records_of(pos)).to(dev), torch.from_numpy(records_of(vel)).to(dev)
    t_pol, t_mem = torch.from_numpy(pol).to(dev), torch.from_numpy(mem).to(dev)
    guard = np.full(((b + 2) * n, 4), np.uint32(NAN_GUARD).view(F), F)
    o_pos, o_vel = torch.from_numpy(guard.copy()).to(dev), torch.from_numpy(guard.copy()).to(dev)
    i_pos, i_vel = torch.from_numpy(guard.copy()).to(dev), torch.from_numpy(guard.copy()).to(dev)
    pad = 64                                                               # guard words on either side of a memory
    mguard = np.full(records * hidden + 2 * pad, np.uint32(NAN_GUARD).view(F), F)
    o_mem = torch.from_numpy(mguard.copy()).to(dev)
    inplace = mguard.copy()
    inplace[pad:-pad] = mem.reshape(-1)
    i_mem = torch.from_numpy(inplace).to(dev)
    cpm = np.ascontiguousarray(nb.eye_constant(width), F).reshape(16)
    cams = torch.empty((records, 16), dtype=torch.float32, device=dev)
    inst = torch.empty((records, 16), dtype=torch.float32, device=dev)
    first, count = n // 2, records - n // 2 - 7
    feat = torch.full((count + 1, features), FILL, dtype=torch.int32, device=dev)
    act = torch.full((count + 1, 2), FILL, dtype=torch.int32, device=dev)
    nxt = torch.full((count + 1, hidden), FILL, dtype=torch.int32, device=dev)
    only = torch.full((count + 1, hidden), FILL, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    shape = (features, hidden, policies, t_pol.data_ptr(), float(limit), float(s_lim))
    with torch.cuda.stream(s):
        _lib.check(lib.nb_launch_instances(records, t_pos.data_ptr(), t_vel.data_ptr(), inst.data_ptr(), s.cuda_stream))
        _lib.check(lib.nb_launch_cameras(records, t_pos.data_ptr(), t_vel.data_ptr(), UP.ctypes.data, cpm.ctypes.data, cams.data_ptr(),
                                         s.cuda_stream))
        _lib.check(lib.nb_scenes_policy_recurrent_observe_launch(b, n, first, count, cams.data_ptr(), inst.data_ptr(), width, *shape,
                                                                 t_mem.data_ptr(), feat.data_ptr(), act.data_ptr(), nxt.data_ptr(),
                                                                 s.cuda_stream))
        _lib.check(lib.nb_scenes_policy_recurrent_observe_launch(b, n, first, count, cams.data_ptr(), inst.data_ptr(), width, *shape,
                                                                 t_mem.data_ptr(), None, None, only.data_ptr(), s.cuda_stream))
        _lib.check(lib.nb_scenes_policy_recurrent_step_launch(None, b, n, cams.data_ptr(), inst.data_ptr(), width, UP.ctypes.data, *shape,
                                                              t_pos.data_ptr(), t_vel.data_ptr(), t_mem.data_ptr(), o_pos.data_ptr() + 16 * n,
                                                              o_vel.data_ptr() + 16 * n, o_mem.data_ptr() + 4 * pad, s.cuda_stream))
        _lib.check(lib.nb_scenes_policy_recurrent_step_launch(None, b, n, cams.data_ptr(), inst.data_ptr(), width, UP.ctypes.data, *shape,
                                                              t_pos.data_ptr(), t_vel.data_ptr(), i_mem.data_ptr() + 4 * pad,
                                                              i_pos.data_ptr() + 16 * n, i_vel.data_ptr() + 16 * n, i_mem.data_ptr() + 4 * pad,
                                                              s.cuda_stream))
    s.synchronize()
    for gp, gv, gm, name in ((o_pos, o_vel, o_mem, "out of place"), (i_pos, i_vel, i_mem, "in place")):
        gp, gv, gm = gp.cpu().numpy(), gv.cpu().numpy(), gm.cpu().numpy()
        for got in (gp, gv):
            assert (bits(got[:n]) == NAN_GUARD).all() and (bits(got[-n:]) == NAN_GUARD).all() and (bits(got[n:-n, 3]) == 0).all(), name
        assert (bits(gm[:pad]) == NAN_GUARD).all() and (bits(gm[-pad:]) == NAN_GUARD).all(), name
        assert_words(gp[n:-n, :3], want_p.reshape(-1, 3), f"stateless, {name}: positions")
        assert_words(gv[n:-n, :3], want_v.reshape(-1, 3), f"stateless, {name}: velocities")
        assert_words(gm[pad:-pad], want_m.reshape(-1), f"stateless, {name}: memory")
    assert (bits(t_pos.cpu().numpy()) == bits(records_of(pos))).all() and (bits(t_vel.cpu().numpy()) == bits(records_of(vel))).all()
    assert bits(t_mem.cpu().numpy()).tobytes() == bits(mem).tobytes()      # the observe launches and the out-of-place step leave the memory's bytes
    g_feat, g_act, g_nxt, g_only = (t.cpu().numpy().view(np.uint32) for t in (feat, act, nxt, only))
    assert (g_feat[:count] == bits(want_x.reshape(-1, features)[first:first + count])).all() and (g_feat[count] == FILL).all()
    assert (g_act[:count] == bits(want_o.reshape(-1, 2)[first:first + count])).all() and (g_act[count] == FILL).all()
    assert (g_nxt[:count] == bits(want_m.reshape(-1, hidden)[first:first + count])).all() and (g_nxt[count] == FILL).all()
    assert (g_only == g_nxt).all()


# -- the search ------------------------------------------------------------------------------------------------------------------------------
def ep_of(sigma, step, coef, seed):
    from nenbody_amd import _lib

    return _lib.NbEsParams(float(sigma), float(step), (ctypes.c_float * 6)(*[float(c) for c in coef]), int(seed))


def es_launches(m, b, g, shape=None, records=None, coef=EK.COEF_MIX):
    """the population of generation g and the update from `records`, through the _floats launches (shape None) or the shape launches:
    (theta (b, m), ranks, fitnesses, report words, mean')"""
    import torch

    from nenbody_amd import _lib

    lib, dev = _lib.load(), torch.device("cuda", 0)
    mean = EK.mean_of(m)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1).copy()).to(dev)
    t_mean, t_theta, t_new = put(mean), put(np.full(b * m + 1, FILL, np.uint32)), put(np.full(m + 1, FILL, np.uint32))
    t_rec, t_rank, t_fit, t_rep = put(records.view(np.uint32)), put(np.zeros(b, np.uint32)), put(np.zeros(b, np.uint32)), put(np.zeros(4, np.uint32))
    ep = ep_of(EK.SIGMA, EK.STEP, coef, EK.SEED_HIGH)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        if shape is None:
            _lib.check(lib.nb_scenes_es_perturb_floats_launch(ctypes.byref(ep), m, g, 0, b, t_mean.data_ptr(), t_theta.data_ptr(), stream.cuda_stream))
            _lib.check(lib.nb_scenes_es_update_floats_launch(ctypes.byref(ep), m, g, b, t_rec.data_ptr(), t_mean.data_ptr(), t_new.data_ptr(),
                                                             t_rank.data_ptr(), t_fit.data_ptr(), t_rep.data_ptr(), stream.cuda_stream))
        else:
            _lib.check(lib.nb_scenes_es_perturb_launch(ctypes.byref(ep), *shape, g, 0, b, t_mean.data_ptr(), t_theta.data_ptr(), stream.cuda_stream))
            _lib.check(lib.nb_scenes_es_update_launch(ctypes.byref(ep), *shape, g, b, t_rec.data_ptr(), t_mean.data_ptr(), t_new.data_ptr(),
                                                      t_rank.data_ptr(), t_fit.data_ptr(), t_rep.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    theta, new = t_theta.cpu().numpy().view(np.uint32), t_new.cpu().numpy().view(np.uint32)
    assert theta[-1] == FILL and new[-1] == FILL                          # nothing behind the M-th word
    return (theta[:-1].view(F).reshape(b, m), t_rank.cpu().numpy().view(np.uint32), t_fit.cpu().numpy().view(F), t_rep.cpu().numpy().view(np.uint32),
            new[:-1].view(F))


def test_the_floats_launches_of_the_search(nb):
    """byte for byte the shape launches at M = nb_policy_floats(8, 7) and (64, 32); against es_restatement at M = 1 and at the longest
    mean, M = 20 674, with B = 3"""
    for shape, b in (((8, 7), 5), ((64, 32), 64)):
        m = P.policy_floats(*shape)
        rec, coef = EK.records(b, "random")
        by_floats, by_shape = es_launches(m, b, 2, None, rec, coef), es_launches(m, b, 2, shape, rec, coef)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(by_floats, by_shape)), shape
    for m in (1, 20674):
        b, g = 3, 1
        rec, coef = EK.records(b, "random")
        theta, r, phi, rep, new = es_launches(m, b, g, None, rec, coef)
        mean = EK.mean_of(m)
        assert theta.tobytes() == E.population(mean, EK.SIGMA, EK.SEED_HIGH, g, 0, b).tobytes(), m
        want = E.rank_and_update(mean, EK.SIGMA, EK.STEP, coef, EK.SEED_HIGH, g, rec)
        assert (r == want[0]).all() and E.same_floats(phi, want[1]) and E.same_report(rep.view(E.REPORT_DTYPE)[0], want[2]), m
        assert new.tobytes() == want[3].tobytes() and (new != mean).any(), m


@pytest.mark.parametrize("b", [4, 5])
def test_three_generations_of_the_six_call_loop(nb, oracle, b):
    """rewind; memory_reset; score_reset; es_perturb; step_policy_scored(k); es_update, three times, against
    policy_recurrent_restatement, score_restatement and es_restatement chained; a set_policy between two generations is overwritten
    and leaves the search its memory"""
    n, width, features, hidden, k = 5, 64, 8, 7, 3
    pos, vel = C.batch(oracle, (1100, n, width, 0.05, b))
    mean = C.policies(features, hidden, 1)[0]
    sigma, step, seed, limit, s_lim = F(0.05), F(1e-3), EK.SEED_HIGH, C.LIMIT, C.MEMORY_LIMIT
    coef = EK.COEF_MIX
    radius_sq, goal = F(np.median(Q.pair_d2(pos[0])[np.triu_indices(n, 1)])), F([0.01, 0.02, 0.0])
    with nb.SceneBatch(pos, vel) as sb:
        sb.set_score(radius_sq, goal)
        sb.es_set_recurrent(mean, features, hidden, sigma, step, coef, seed, limit, s_lim)
        sb.keep()
        assert sb.es_generation == 0 and sb.es_mean().tobytes() == mean.tobytes() and len(mean) == RR.policy_recurrent_floats(features, hidden)
        for g in range(3):
            sb.rewind()
            sb.memory_reset()
            sb.score_reset()
            sb.es_perturb()
            sb.step_policy_scored(k, width)
            sb.es_update()
            theta = E.population(mean, sigma, seed, g, 0, b)
            steps = RR.rollout(rows_by(nb, width), pos, vel, np.zeros((b, n, hidden), F), theta, features, hidden, limit, s_lim, UP, k)
            acc = None
            for st in steps:
                acc = Q.batch(st[3], st[4], radius_sq, goal, acc=acc)
            assert Q.same(sb.scores(), acc), g
            want = E.rank_and_update(mean, sigma, step, coef, seed, g, acc)
            rep, phi, r = sb.es_result()
            assert (r == want[0]).all() and E.same_floats(phi, want[1]) and E.same_report(rep, want[2]), g
            assert sb.es_mean().tobytes() == want[3].tobytes() and (want[3] != mean).any(), g
            assert rep["generation"] == g and sb.es_generation == g + 1 and sb.steps_done == k
            mean = want[3]
            assert P.same(sb.positions(), steps[-1][3]) and P.same(sb.velocities(), steps[-1][4]) and P.same(sb.memory(), steps[-1][2])
            assert (bits(steps[-1][2]) != 0).any()
            if g == 0:
                sb.set_policy(C.feedforward(C.policies(features, hidden, 1, seed=9), features, hidden), features, hidden, 0.25)


# -- the context's refusals that need a device ---------------------------------------------------------------------------------------------
def test_context_entries_refuse_with_their_texts(nb, oracle):
    from nenbody_amd import _lib

    lib = _lib.load()
    cp = np.ascontiguousarray(nb.eye_constant(64), F).reshape(16)
    up, cpp = UP.ctypes.data, cp.ctypes.data
    pol = C.policies(8, 7, 3)
    w = pol.ctypes.data
    feat, act, mem = np.zeros(3 * 8 * 8, F), np.zeros(3 * 8 * 2 + 2, F), np.zeros(3 * 8 * 7, F)
    f, a, m = feat.ctypes.data, act.ctypes.data, mem.ctypes.data
    err = lambda ctx: lib.nb_scenes_last_error(ctx).decode()
    Sp, Ey, Mr, Mg, Ms, Es = ("nb_scenes_set_policy_recurrent: ", "nb_scenes_eyes_policy_memory: ", "nb_scenes_memory_reset: ", "nb_scenes_memory: ",
                              "nb_scenes_set_memory: ", "nb_scenes_es_set_recurrent: ")
    upload, unset = "no state uploaded (call nb_scenes_upload first)", "no recurrent policy set (call nb_scenes_set_policy_recurrent first)"
    e = ep_of(0.05, 1e-3, EK.COEF_GOAL, 1)
    ctx = ctypes.c_void_p()
    _lib.check(lib.nb_scenes_create(3, 8, None, ctypes.byref(ctx)))
    try:
        assert lib.nb_scenes_eyes_policy_memory(ctx, 0, 3, up, cpp, 64, f, a, m) == _lib.NB_ERR_STATE and err(ctx) == Ey + unset
        assert lib.nb_scenes_memory_reset(ctx) == _lib.NB_ERR_STATE and err(ctx) == Mr + unset
        assert lib.nb_scenes_memory(ctx, 0, 3, m) == _lib.NB_ERR_STATE and err(ctx) == Mg + unset
        assert lib.nb_scenes_set_memory(ctx, m) == _lib.NB_ERR_STATE and err(ctx) == Ms + unset
        assert lib.nb_scenes_set_policy_recurrent(ctx, 8, 7, 3, w, 0.5, 1.0) == _lib.NB_OK          # a policy before an upload
        assert lib.nb_scenes_memory_reset(ctx) == _lib.NB_OK and lib.nb_scenes_memory(ctx, 0, 3, m) == _lib.NB_OK and not mem.any()
        assert lib.nb_scenes_eyes_policy_memory(ctx, 0, 3, up, cpp, 64, f, a, m) == _lib.NB_ERR_STATE and err(ctx) == Ey + upload
        assert lib.nb_scenes_step_policy(ctx, 1, up, cpp, 64) == _lib.NB_ERR_STATE and err(ctx) == "nb_scenes_step_policy: " + upload
    finally:
        lib.nb_scenes_destroy(ctx)
    pos, vel = C.batch(oracle, (1100, 8, 64, 0.1, 3))
    with nb.SceneBatch(pos, vel) as sb:
        c = sb._ctx
        sb.set_policy(C.feedforward(pol, 8, 7), 8, 7, 0.5)                 # a feedforward policy is no recurrent one
        assert lib.nb_scenes_eyes_policy_memory(c, 0, 3, up, cpp, 64, f, a, m) == _lib.NB_ERR_STATE and err(c) == Ey + unset
        assert lib.nb_scenes_memory_reset(c) == _lib.NB_ERR_STATE and err(c) == Mr + unset
        for args, text in (((8, 7, 3, None, 0.5, 1.0), "null argument"), ((0, 7, 3, w, 0.5, 1.0), "features must be 1 .. NB_POLICY_MAX_FEATURES (256)"),
                           ((8, 65, 3, w, 0.5, 1.0), "hidden must be 1 .. NB_POLICY_MAX_HIDDEN (64)"), ((8, 7, 2, w, 0.5, 1.0), "policies must be 1 or scenes"),
                           ((8, 7, 3, w, -0.5, 1.0), "accel_limit must be at least 0 (+inf: no limit)"),
                           ((8, 7, 3, w, 0.5, -1.0), "memory_limit must be at least 0 (+inf: no limit)"),
                           ((8, 7, 3, w, 0.5, float("nan")), "memory_limit must be at least 0 (+inf: no limit)"),
                           ((8, 7, 3, w, -0.5, -1.0), "accel_limit must be at least 0 (+inf: no limit)")):
            assert lib.nb_scenes_set_policy_recurrent(c, *args) == _lib.NB_ERR_INVALID, args
            assert err(c) == Sp + text
        assert lib.nb_scenes_memory_reset(c) == _lib.NB_ERR_STATE and err(c) == Mr + unset           # a refused policy is none
        for args, text in (((8, 7, None, 0.5, 1.0, ctypes.byref(e)), "null argument"), ((8, 7, w, 0.5, 1.0, None), "null argument"),
                           ((257, 7, w, 0.5, 1.0, ctypes.byref(e)), "features must be 1 .. NB_POLICY_MAX_FEATURES (256)"),
                           ((8, 7, w, 0.5, -1.0, ctypes.byref(e)), "memory_limit must be at least 0 (+inf: no limit)"),
                           ((8, 7, w, 0.5, 1.0, ctypes.byref(ep_of(-1.0, 1e-3, EK.COEF_GOAL, 1))), "sigma must be at least 0 and finite")):
            assert lib.nb_scenes_es_set_recurrent(c, *args) == _lib.NB_ERR_INVALID, args
            assert err(c) == Es + text
        sb.set_policy_recurrent(pol, 8, 7, 0.5, 1.0)
        for args, text in (((0, 3, None, cpp, 64, f, a, m), "null argument"), ((0, 3, up, cpp, 0, f, a, m), "width must be 1 .. NB_EYES_MAX_WIDTH (4096)"),
                           ((0, 3, up, cpp, 60, f, a, m), "width must be a multiple of features"),
                           ((1, 3, up, cpp, 64, f, a, m), "scenes [first_scene, first_scene + scene_count) exceed the batch"),
                           ((0, 3, up, cpp, 64, None, None, None), "feat_out, act_out and mem_out are all NULL"),
                           ((0, 3, up, cpp, 64, f, a, a + 4), "the outputs must not overlap each other or an input")):
            assert lib.nb_scenes_eyes_policy_memory(c, *args) == _lib.NB_ERR_INVALID, args
            assert err(c) == Ey + text
        assert lib.nb_scenes_eyes_policy_memory(c, 0, 3, up, cpp, 64, None, None, m) == _lib.NB_OK  # one output is enough
        assert lib.nb_scenes_eyes_policy_memory(c, 0, 3, up, cpp, 64, None, a, None) == _lib.NB_OK
        assert lib.nb_scenes_eyes_policy_memory(c, 3, 0, up, cpp, 64, f, a, m) == _lib.NB_OK        # no scenes: a checked no-op
        assert lib.nb_scenes_memory(c, 0, 3, None) == _lib.NB_ERR_INVALID and err(c) == Mg + "null argument"
        assert lib.nb_scenes_memory(c, 2, 2, m) == _lib.NB_ERR_INVALID and err(c) == Mg + "scenes [first_scene, first_scene + scene_count) exceed the batch"
        assert lib.nb_scenes_set_memory(c, None) == _lib.NB_ERR_INVALID and err(c) == Ms + "null argument"
        assert sb.steps_done == 0
        with pytest.raises(ValueError):
            sb.set_policy_recurrent(pol[:, :-1], 8, 7)
        with pytest.raises(ValueError):
            sb.set_memory(np.zeros((3, 8, 6), F))
