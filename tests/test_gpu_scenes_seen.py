"""GPU tests of the scene batches' seen boids step: the fused kernel of nb_scenes_seen.inc against what a
context per scene computes and against the numpy restatement, every word of every body's position and velocity (SV1, SV2, SV4),
and every word of the seen sets it folds over against Scene.seen (SV3).

Expected values are formed as tests/test_gpu_seen.py::assert_step forms them: per scene a Scene, per step the mask from that
Scene's eye rows of the state before the step through seen_restatement.boids_seen_step, and the Scene's own step, which must
agree with it; for k > 1 a second Scene's step_boids_seen_n(k) must give the same words too.  The rows (seed, n, width, scale, scenes) are tests/scenes_seen_cases.py's; tests/test_scenes_seen_cpu.py holds their
premises.  A NaN of the reference is met by a NaN."""
import ctypes
import statistics
import subprocess
import time

import numpy as np
import pytest

import scenes_seen_cases as K
import seen_cases as SK
import seen_restatement as S

pytestmark = pytest.mark.gpu

F = np.float32
NONE = S.NONE
UP = K.UP
FILL = 0x07070707


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_words(got, want, what):
    ok, rows = SK.same_words(got, want)
    assert ok, f"{what}: {len(rows)} bodies differ, first {rows[:8]}"


def per_scene(nb, pos, vel, k, width=1024, cp=None, consts=None):
    """scene after scene k seen steps of a Scene: (positions, velocities) (B, n, 3) by the restatement, which the Scene's own
    steps must give too"""
    consts = consts or {}
    params = SK.device_params(nb, **consts) if consts else None
    out_p, out_v = np.empty_like(pos), np.empty_like(vel)
    for s in range(len(pos)):
        with nb.Scene(pos[s], vel[s]) as sc:
            for step in range(k):
                p0, v0 = sc.state()
                ids, _ = sc.eyes(width=width, cp=cp)
                want = S.boids_seen_step(p0, v0, S.mask_of_rows(ids, sc.n), **{key: F(val) for key, val in consts.items()})
                sc.step_boids_seen(params, width, cp=cp)
                p1, v1 = sc.state()
                assert_words(p1, want[0], f"the context's own step {step} of scene {s}: positions")
                assert_words(v1, want[1], f"the context's own step {step} of scene {s}: velocities")
            out_p[s], out_v[s] = p1, v1
        if k > 1:                                                      # and the k steps as ONE call of the context's entry
            with nb.Scene(pos[s], vel[s]) as sc:
                sc.step_boids_seen_n(k, params, width, cp=cp)
                pk, vk = sc.state()
            assert_words(pk, out_p[s], f"step_boids_seen_n({k}) of scene {s}: positions")
            assert_words(vk, out_v[s], f"step_boids_seen_n({k}) of scene {s}: velocities")
    return out_p, out_v


_expected = {}


def expected(nb, oracle, row, k):
    """per_scene for every scene of a row, computed once"""
    if (row, k) not in _expected:
        pos, vel = K.batch(oracle, row)
        _expected[(row, k)] = (pos, vel) + per_scene(nb, pos, vel, k, width=row[2])
    return _expected[(row, k)]


def batch_step(nb, pos, vel, k, width=1024, cp=None, consts=None):
    params = SK.device_params(nb, **consts) if consts else None
    with nb.SceneBatch(pos, vel) as sb:
        sb.step_boids_seen(k, params, width, cp=cp)
        assert sb.steps_done == k
        return sb.positions(), sb.velocities()


# -- SV1 ---------------------------------------------------------------------------------------------------------------------------------
SIZE_CASES = [(n, b, k) for n in sorted(K.SIZES) if n != 2048 for b in (1, 3) for k in (1, 3)] + [(2048, 2, 1)]


@pytest.mark.parametrize("n,b,k", SIZE_CASES)
def test_every_scene_gets_its_contexts_bits(nb, oracle, n, b, k):
    pos, vel, want_p, want_v = expected(nb, oracle, K.SIZES[n], k)
    got_p, got_v = batch_step(nb, pos[:b], vel[:b], k)
    assert_words(got_p.reshape(-1, 3), want_p[:b].reshape(-1, 3), f"n={n} B={b} k={k}: positions")
    assert_words(got_v.reshape(-1, 3), want_v[:b].reshape(-1, 3), f"n={n} B={b} k={k}: velocities")


@pytest.mark.parametrize("width", sorted(K.WIDTHS))
def test_widths(nb, oracle, width):
    row = K.WIDTHS[width]
    pos, vel, want_p, want_v = expected(nb, oracle, row, 2)
    got_p, got_v = batch_step(nb, pos, vel, 2, width=width)
    assert_words(got_p.reshape(-1, 3), want_p.reshape(-1, 3), f"W={width}: positions")
    assert_words(got_v.reshape(-1, 3), want_v.reshape(-1, 3), f"W={width}: velocities")


def test_three_dimensional_data_under_a_callers_camera(nb, oracle):
    n, b = 300, 3
    pos, vel = K.batch(oracle, (9, n, 1024, 1.0, b))
    rng = np.random.default_rng(9)
    pos[:, :, 2] = rng.uniform(-30, 30, (b, n)).astype(F)
    vel[:, :, 2] = rng.uniform(-0.05, 0.05, (b, n)).astype(F)
    cp = oracle.camera_constant(30.0, 1.0, 1.0, 10000.0)
    want_p, want_v = per_scene(nb, pos, vel, 1, cp=cp)
    got_p, got_v = batch_step(nb, pos, vel, 1, cp=cp)
    assert_words(got_p.reshape(-1, 3), want_p.reshape(-1, 3), "3-D: positions")
    assert_words(got_v.reshape(-1, 3), want_v.reshape(-1, 3), "3-D: velocities")
    assert (got_v[:, :, 2] != 0).any(1).all()


@pytest.mark.parametrize("n", [65, 300])
def test_cut_cloud_under_cut_constants(nb, oracle, n):
    """each rule holds for some seen pairs and fails for others (tests/seen_cases.py)"""
    clouds = [SK.cut_cloud(oracle, n, 40 + s) for s in range(3)]
    pos, vel = np.stack([c[0] for c in clouds]), np.stack([c[1] for c in clouds])
    held = np.zeros(3)
    pairs = 0
    for s in range(3):
        with nb.Scene(pos[s], vel[s]) as sc:
            mask = S.mask_of_rows(sc.eyes()[0], n)
        shares = SK.predicate_shares(pos[s], vel[s], mask, **SK.CUT)
        held += np.round(np.array(shares[:3]) * shares[3])
        pairs += shares[3]
    assert pairs > n // 2 and (held >= 1).all() and (held <= pairs - 1).all(), (held, pairs)   # over the batch, every rule cuts
    want_p, want_v = per_scene(nb, pos, vel, 2, consts=SK.CUT)
    got_p, got_v = batch_step(nb, pos, vel, 2, consts=SK.CUT)
    assert_words(got_p.reshape(-1, 3), want_p.reshape(-1, 3), f"cut cloud n={n}: positions")
    assert_words(got_v.reshape(-1, 3), want_v.reshape(-1, 3), f"cut cloud n={n}: velocities")


def test_hand_case_in_scene_one_of_three(nb, oracle):
    """DESIGN.md section 12's hand case: body 0 sees body 1 and takes v.x = 0.7f, body 1 sees nobody and stops"""
    pos, vel = K.batch(oracle, (1100, 2, 1024, 1.0, 3))
    pos[1], vel[1] = [[0, 0, 0], [10, 0, 0]], [[1, 0, 0], [1, 0, 0]]
    with nb.SceneBatch(pos, vel) as sb:
        count, ids = sb.seen()
        assert (count[1] == [1, 0]).all() and ids[1, 0, 0] == 1 and (ids[1, 0, 1:] == NONE).all() and (ids[1, 1] == NONE).all()
        sb.step_boids_seen()
        p, v = sb.positions()[1], sb.velocities()[1]
    vx = (F(10) * F(0.02) + F(0) * F(0.05)) + F(1) * F(0.5)
    assert (bits(v[0]) == [0x3F333333, 0, 0]).all() and bits(p[0])[0] == bits(vx * F(0.04) + F(0))[0] and (bits(p[0])[1:] == 0).all()
    assert (bits(v[1]) == 0).all() and (bits(p[1]) == bits(F([10, 0, 0]))).all()


def test_more_eyes_than_the_grid_cap(nb, oracle):
    """n = 5 and 209 718 scenes: 1 048 590 eyes, more than the 2^20 workgroups a launch has at most, so some workgroups take a second
    eye.  The batch repeats three scenes; every copy must get its original's bits"""
    n, width, distinct = 5, 128, 3
    b = (1 << 20) // n + distinct
    assert b * n > 1 << 20
    row = (1100, n, width, 0.05, distinct)
    pos3, vel3 = K.batch(oracle, row)
    with nb.Scene(pos3[0], vel3[0]) as sc:
        assert (sc.eyes(width=width)[0] != NONE).any()                 # somebody is seen
    want_p, want_v = per_scene(nb, pos3, vel3, 1, width=width)
    reps = -(-b // distinct)
    pos, vel = np.tile(pos3, (reps, 1, 1))[:b], np.tile(vel3, (reps, 1, 1))[:b]
    got_p, got_v = batch_step(nb, pos, vel, 1, width=width)
    assert_words(got_p.reshape(-1, 3), np.tile(want_p, (reps, 1, 1))[:b].reshape(-1, 3), "positions")
    assert_words(got_v.reshape(-1, 3), np.tile(want_v, (reps, 1, 1))[:b].reshape(-1, 3), "velocities")
    assert (bits(got_v) != 0).any()


# -- SV2, SV4 ----------------------------------------------------------------------------------------------------------------------------
def test_a_hostile_scene_between_two_clean_ones(nb, oracle):
    row = K.SIZES[100]
    pos, vel, want_p, want_v = expected(nb, oracle, row, 3)
    bad_p, bad_v = pos.copy(), vel.copy()
    rng = np.random.default_rng(3)
    bad_p[1] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), (100, 3))
    bad_v[1] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1.0], F), (100, 3))
    got_p, got_v = batch_step(nb, bad_p, bad_v, 3)
    for s in (0, 2):
        assert_words(got_p[s], want_p[s], f"scene {s} beside a hostile one: positions")
        assert_words(got_v[s], want_v[s], f"scene {s} beside a hostile one: velocities")
    two_p, two_v = batch_step(nb, pos[[0, 2]], vel[[0, 2]], 3)        # the run without it
    assert (bits(two_p) == bits(got_p[[0, 2]])).all() and (bits(two_v) == bits(got_v[[0, 2]])).all()


def test_k_steps_in_one_call_are_k_calls_of_one(nb, oracle):
    pos, vel, want_p, want_v = expected(nb, oracle, K.SIZES[129], 3)
    with nb.SceneBatch(pos, vel) as sb:
        for _ in range(3):
            sb.step_boids_seen(1)
        assert sb.steps_done == 3
        assert_words(sb.positions().reshape(-1, 3), want_p.reshape(-1, 3), "three calls: positions")
        assert_words(sb.velocities().reshape(-1, 3), want_v.reshape(-1, 3), "three calls: velocities")


def test_mixed_context_steps_twice(nb, oracle):
    """step(2), step_boids_seen(1), step_boids(1), step_boids_seen(2) against per-scene Scenes doing the same; two runs, the same bits"""
    pos, vel = K.batch(oracle, K.SIZES[100])
    want_p, want_v = np.empty_like(pos), np.empty_like(vel)
    for s in range(len(pos)):
        with nb.Scene(pos[s], vel[s]) as sc:
            sc.step_n(2)
            sc.step_boids_seen_n(1)
            sc.step_boids_n(1)
            sc.step_boids_seen_n(2)
            sc.sync()
            sc._refresh(False)
            want_p[s], want_v[s] = sc.state()
    runs = []
    for _ in range(2):
        with nb.SceneBatch(pos, vel) as sb:
            sb.step(2)
            sb.step_boids_seen(1)
            sb.step_boids(1)
            sb.step_boids_seen(2)
            assert sb.steps_done == 6
            p_dev, v_dev, _ = sb.device_state()
            assert p_dev and v_dev
            runs.append((sb.positions(), sb.velocities()))
    assert_words(runs[0][0].reshape(-1, 3), want_p.reshape(-1, 3), "mixed: positions")
    assert_words(runs[0][1].reshape(-1, 3), want_v.reshape(-1, 3), "mixed: velocities")
    assert (bits(runs[0][0]) == bits(runs[1][0])).all() and (bits(runs[0][1]) == bits(runs[1][1])).all()      # SV4


# -- the stateless step launch -----------------------------------------------------------------------------------------------------------
def device_matrices(nb, lib, _lib, torch, t_pos, t_vel, width, stream):
    """(cams, inst) tensors (records, 16) of the records t_pos / t_vel, by nb_launch_cameras / nb_launch_instances"""
    records = t_pos.shape[0]
    cams = torch.empty((records, 16), dtype=torch.float32, device=t_pos.device)
    inst = torch.empty((records, 16), dtype=torch.float32, device=t_pos.device)
    cpm = np.ascontiguousarray(nb.eye_constant(width), F).reshape(16)
    _lib.check(lib.nb_launch_instances(records, t_pos.data_ptr(), t_vel.data_ptr(), inst.data_ptr(), stream.cuda_stream))
    _lib.check(lib.nb_launch_cameras(records, t_pos.data_ptr(), t_vel.data_ptr(), UP.ctypes.data, cpm.ctypes.data, cams.data_ptr(),
                                     stream.cuda_stream))
    return cams, inst


def records_of(a):
    r = np.zeros(a.shape[:-1] + (4,), F)
    r[..., :3] = a
    return r.reshape(-1, 4)


@pytest.mark.parametrize("n", [100, 129])
def test_stateless_step_launch_between_guard_scenes(nb, oracle, n):
    """pos_out and vel_out lie inside tensors with one scene of NaN records in front and one behind: the guards come back bit for
    bit, the inputs are unmodified, and what lies between is the step"""
    import torch

    from nenbody_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    pos, vel, want_p, want_v = expected(nb, oracle, K.SIZES[n], 1)
    b = len(pos)
    t_pos, t_vel = torch.from_numpy(records_of(pos)).to(dev), torch.from_numpy(records_of(vel)).to(dev)
    guard = np.full(((b + 2) * n, 4), np.uint32(0x7FC0BEEF).view(F), F)
    o_pos, o_vel = torch.from_numpy(guard.copy()).to(dev), torch.from_numpy(guard.copy()).to(dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        cams, inst = device_matrices(nb, lib, _lib, torch, t_pos, t_vel, 1024, s)
        _lib.check(lib.nb_scenes_boids_seen_step_launch(None, b, n, cams.data_ptr(), inst.data_ptr(), 1024, t_pos.data_ptr(),
                                                        t_vel.data_ptr(), o_pos.data_ptr() + 16 * n, o_vel.data_ptr() + 16 * n,
                                                        s.cuda_stream))
    s.synchronize()
    gp, gv = o_pos.cpu().numpy(), o_vel.cpu().numpy()
    for got in (gp, gv):
        assert (bits(got[:n]) == 0x7FC0BEEF).all() and (bits(got[-n:]) == 0x7FC0BEEF).all()
        assert (got[n:-n, 3] == 0).all()
    assert_words(gp[n:-n, :3], want_p.reshape(-1, 3), "stateless: positions")
    assert_words(gv[n:-n, :3], want_v.reshape(-1, 3), "stateless: velocities")
    assert (bits(t_pos.cpu().numpy()) == bits(records_of(pos))).all() and (bits(t_vel.cpu().numpy()) == bits(records_of(vel))).all()


# -- SV3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,width", sorted(K.LISTS))
def test_the_seen_sets_are_scene_seens(nb, oracle, n, width):
    import torch

    from nenbody_amd import _lib

    lib = _lib.load()
    pos, vel = K.batch(oracle, K.LISTS[(n, width)])
    b = len(pos)
    want_c, want_i = np.empty((b, n), np.uint32), np.empty((b, n, width), np.uint32)
    for s in range(b):
        with nb.Scene(pos[s], vel[s]) as sc:
            want_c[s], want_i[s] = sc.seen(width=width)[0:2]
    assert (want_c == 0).any(1).all() and ((want_c > 0).mean(1) > 0.5).all() and want_c.max() > 1
    with nb.SceneBatch(pos, vel) as sb:
        got_c, got_i = sb.seen(width=width)
        assert (got_c == want_c).all() and (got_i == want_i).all()
        sub_c, sub_i = sb.seen(first_scene=1, scene_count=2, width=width)
        assert (sub_c == want_c[1:]).all() and (sub_i == want_i[1:]).all()
        assert sb.seen(first_scene=3, scene_count=0, width=width)[1].shape == (0, n, width)
    # nb_scenes_seen_launch over a range of eyes that starts and ends inside a scene; every word of the outputs is written
    dev = torch.device("cuda", 0)
    t_pos, t_vel = torch.from_numpy(records_of(pos)).to(dev), torch.from_numpy(records_of(vel)).to(dev)
    first, count = n // 2, b * n - n // 2 - 7
    o_c = torch.full((count + 1,), FILL, dtype=torch.int32, device=dev)
    o_i = torch.full((count + 1, width), FILL, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        cams, inst = device_matrices(nb, lib, _lib, torch, t_pos, t_vel, width, s)
        _lib.check(lib.nb_scenes_seen_launch(b, n, first, count, cams.data_ptr(), inst.data_ptr(), width, o_c.data_ptr(), o_i.data_ptr(),
                                             s.cuda_stream))
    s.synchronize()
    gc, gi = o_c.cpu().numpy().view(np.uint32), o_i.cpu().numpy().view(np.uint32)
    assert (gc[:count] == want_c.reshape(-1)[first:first + count]).all() and gc[count] == FILL
    assert (gi[:count] == want_i.reshape(-1, width)[first:first + count]).all() and (gi[count] == FILL).all()


# -- the context's refusals that need a device --------------------------------------------------------------------------------------------
def test_context_entries_refuse_with_their_texts(nb, oracle):
    from nenbody_amd import _lib

    lib = _lib.load()
    cp = np.ascontiguousarray(nb.eye_constant(64), F).reshape(16)
    up, cpp = UP.ctypes.data, cp.ctypes.data
    buf = np.zeros(3 * 8 * 64 + 64, np.uint32)
    out = buf.ctypes.data
    err = lambda ctx: lib.nb_scenes_last_error(ctx).decode()
    ctx = ctypes.c_void_p()
    _lib.check(lib.nb_scenes_create(3, 8, None, ctypes.byref(ctx)))
    try:
        assert lib.nb_scenes_step_boids_seen(ctx, 1, None, up, cpp, 64) == _lib.NB_ERR_STATE
        assert err(ctx) == "nb_scenes_step_boids_seen: no state uploaded (call nb_scenes_upload first)"
        assert lib.nb_scenes_eyes_seen(ctx, 0, 3, up, cpp, 64, out, None) == _lib.NB_ERR_STATE
        assert err(ctx) == "nb_scenes_eyes_seen: no state uploaded (call nb_scenes_upload first)"
        assert lib.nb_scenes_step_boids_seen(ctx, 1, None, up, cpp, 0) == _lib.NB_ERR_INVALID       # the arguments come first
        assert err(ctx) == "nb_scenes_step_boids_seen: width must be 1 .. NB_EYES_MAX_WIDTH (4096)"
    finally:
        lib.nb_scenes_destroy(ctx)
    pos, vel = K.batch(oracle, (1100, 8, 64, 0.1, 3))
    tile100 = nb.default_boids_params(tile=100)
    with nb.SceneBatch(pos, vel) as sb:
        c = sb._ctx
        for args, text in (((1, None, None, cpp, 64), "null argument"), ((1, None, up, None, 64), "null argument"),
                           ((1, None, up, cpp, 4097), "width must be 1 .. NB_EYES_MAX_WIDTH (4096)"),
                           ((1, ctypes.byref(tile100), up, cpp, 64), "params.tile must be 0, 256, 512 or 1024")):
            assert lib.nb_scenes_step_boids_seen(c, *args) == _lib.NB_ERR_INVALID, args
            assert err(c) == "nb_scenes_step_boids_seen: " + text
        for args, text in (((0, 3, None, cpp, 64, out, None), "null argument"), ((0, 3, up, cpp, 0, out, None), "width must be 1 .. NB_EYES_MAX_WIDTH (4096)"),
                           ((1, 3, up, cpp, 64, out, None), "scenes [first_scene, first_scene + scene_count) exceed the batch"),
                           ((0, 3, up, cpp, 64, None, None), "seen_count and seen_ids are both NULL"),
                           ((0, 3, up, cpp, 64, out, out + 4), "the outputs must not overlap each other or an input")):
            assert lib.nb_scenes_eyes_seen(c, *args) == _lib.NB_ERR_INVALID, args
            assert err(c) == "nb_scenes_eyes_seen: " + text
        assert lib.nb_scenes_step_boids_seen(c, 0, None, up, cpp, 64) == _lib.NB_OK and sb.steps_done == 0     # k = 0: a checked no-op
        assert lib.nb_scenes_eyes_seen(c, 0, 3, up, cpp, 64, out, None) == _lib.NB_OK                          # one output is enough
        assert lib.nb_scenes_eyes_seen(c, 0, 3, up, cpp, 64, None, out) == _lib.NB_OK


# -- the C++ host ------------------------------------------------------------------------------------------------------------------------
def test_cpp_host_matches_the_contexts(nb, oracle, tmp_path):
    from test_scenes_seen_cpu import EXE, build_exe

    build_exe()
    row = K.SIZES[100]
    b, n, width, k = row[4], 100, 1024, 1
    out = tmp_path / "out.bin"
    r = subprocess.run([EXE, str(b), str(n), str(width), str(k), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, dtype=np.uint32)
    eyes = b * n
    count, ids, p, v = np.split(raw, [eyes, eyes + eyes * width, eyes + eyes * width + 3 * eyes])
    pos, vel, want_p, want_v = expected(nb, oracle, row, k)
    for s in range(b):
        with nb.Scene(pos[s], vel[s]) as sc:
            wc, wi = sc.seen(width=width)[0:2]
        assert (count.reshape(b, n)[s] == wc).all() and (ids.reshape(b, n, width)[s] == wi).all()
    assert_words(p.view(F).reshape(-1, 3), want_p.reshape(-1, 3), "C++: positions")
    assert_words(v.view(F).reshape(-1, 3), want_v.reshape(-1, 3), "C++: velocities")


# -- the floor ---------------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_64_scenes_beats_64_contexts_fourfold(nb, oracle):
    """n = 100, B = 64, W = 1024, k = 4: the batch's step against the only way the library offered before, 64 contexts'
    nb_step_boids_seen(4) issued back to back -- wall time to the last sync, median of 5, after a warm-up, the procedure of
    test_gpu_scenes.py::test_a_batch_of_256_small_scenes_beats_256_contexts_fourfold.  A quarter is that test's own convention."""
    k = 4
    pos, vel = K.batch(oracle, K.FLOOR)
    batch = len(pos)

    def timed(run, wait):
        run(), wait()
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            run()
            wait()
            times.append(time.perf_counter() - t0)
        return statistics.median(times)

    with nb.SceneBatch(pos, vel) as sb:
        t_batch = timed(lambda: sb.step_boids_seen(k), sb.sync)
    ctxs = [nb.Scene(pos[s], vel[s]) for s in range(batch)]
    try:
        t_ctx = timed(lambda: [sc.step_boids_seen_n(k) for sc in ctxs], lambda: [sc.sync() for sc in ctxs])
    finally:
        for sc in ctxs:
            sc.close()
    print(f"batch {t_batch * 1e3:.3f} ms, {batch} contexts {t_ctx * 1e3:.3f} ms, ratio {t_ctx / t_batch:.1f}")
    assert t_batch < t_ctx / 4, (t_batch, t_ctx)
