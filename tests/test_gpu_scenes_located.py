"""GPU tests of the scene batches' gravity from located vision: the fused kernel of nb_scenes_located.inc
against what a context per scene computes and against the numpy restatement, every word of every body's position and velocity (SL1,
SL2, SL4), and every word of the located sets it folds over against Scene.located (SL3).

Expected values are formed as tests/test_gpu_located.py::assert_step forms them: per scene a Scene, per step the located sets of that
Scene's eye rows of the state before the step through located_restatement (located_of_rows, nbody_located_step), and the Scene's own
step, which must agree with it; for k > 1 a second Scene's step_nbody_located_n(k) must give the same words too.  The rows (seed, n,
width, scale, scenes) are tests/scenes_located_cases.py's; tests/test_scenes_located_cpu.py holds their premises.  A NaN of the
reference is met by a NaN."""
import ctypes
import statistics
import subprocess
import time

import numpy as np
import pytest

import located_restatement as L
import scenes_located_cases as K
import seen_cases as SK

pytestmark = pytest.mark.gpu

F = np.float32
NONE = L.NONE
UP = K.UP
FILL = 0x07070707


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_words(got, want, what):
    ok, rows = SK.same_words(got, want)
    assert ok, f"{what}: {len(rows)} bodies differ, first {rows[:8]}"


def device_params(nb, consts):
    prm = nb.default_params()
    for key, val in (consts or {}).items():
        setattr(prm, key, val)
    return prm


def per_scene(nb, pos, vel, k, width=1024, cp=None, up=UP, consts=None):
    """scene after scene k located steps of a Scene: (positions, velocities) (B, n, 3) by the restatement, which the Scene's own
    steps must give too"""
    prm = device_params(nb, consts)
    cpm = nb.eye_constant(width) if cp is None else cp
    out_p, out_v = np.empty_like(pos), np.empty_like(vel)
    for s in range(len(pos)):
        with nb.Scene(pos[s], vel[s], prm) as sc:
            for step in range(k):
                p0, v0 = sc.state()
                ids, depth = sc.eyes(width=width, up=up, cp=cp)
                count, _, _, _, _, rel = L.located_of_rows(ids, depth, v0, up, cpm)
                want = L.nbody_located_step(p0, v0, count, rel, dt=prm.dt, g=prm.G, bias=prm.bias)
                sc.step_nbody_located(width, up, cp)
                p1, v1 = sc.state()
                assert_words(p1, want[0], f"the context's own step {step} of scene {s}: positions")
                assert_words(v1, want[1], f"the context's own step {step} of scene {s}: velocities")
            out_p[s], out_v[s] = p1, v1
        if k > 1:                                                      # and the k steps as ONE call of the context's entry
            with nb.Scene(pos[s], vel[s], prm) as sc:
                sc.step_nbody_located_n(k, width, up, cp)
                pk, vk = sc.state()
            assert_words(pk, out_p[s], f"step_nbody_located_n({k}) of scene {s}: positions")
            assert_words(vk, out_v[s], f"step_nbody_located_n({k}) of scene {s}: velocities")
    return out_p, out_v


_expected = {}


def expected(nb, oracle, row, k):
    """per_scene for every scene of a row, computed once"""
    if (row, k) not in _expected:
        pos, vel = K.batch(oracle, row)
        _expected[(row, k)] = (pos, vel) + per_scene(nb, pos, vel, k, width=row[2])
    return _expected[(row, k)]


def batch_step(nb, pos, vel, k, width=1024, cp=None, up=UP, consts=None):
    with nb.SceneBatch(pos, vel, device_params(nb, consts)) as sb:
        sb.step_nbody_located(k, width, up, cp)
        assert sb.steps_done == k
        return sb.positions(), sb.velocities()


def scene_located(nb, pos, vel, width, cp=None):
    """Scene.located of every scene without its column counts: (count, ids, depth bits, col, rel bits)"""
    out = []
    for s in range(len(pos)):
        with nb.Scene(pos[s], vel[s]) as sc:
            count, ids, depth, _, col, rel = sc.located(width=width, cp=cp)
        out.append((count, ids, bits(depth), col, bits(rel)))
    return tuple(np.stack([o[a] for o in out]) for a in range(5))


# -- SL1 ---------------------------------------------------------------------------------------------------------------------------------
SIZE_CASES = [(n, b, k) for n in sorted(K.SIZES) if n != 2048 for b in (1, 3) for k in (1, 3)] + [(2048, 2, 1)]


@pytest.mark.parametrize("n,b,k", SIZE_CASES)
def test_every_scene_gets_its_contexts_bits(nb, oracle, n, b, k):
    row = K.SIZES[n]
    pos, vel, want_p, want_v = expected(nb, oracle, row, k)
    got_p, got_v = batch_step(nb, pos[:b], vel[:b], k, width=row[2])
    assert_words(got_p.reshape(-1, 3), want_p[:b].reshape(-1, 3), f"n={n} B={b} k={k}: positions")
    assert_words(got_v.reshape(-1, 3), want_v[:b].reshape(-1, 3), f"n={n} B={b} k={k}: velocities")


@pytest.mark.parametrize("width", sorted(K.WIDTHS))
def test_widths(nb, oracle, width):
    row = K.WIDTHS[width]
    pos, vel, want_p, want_v = expected(nb, oracle, row, 2)
    got_p, got_v = batch_step(nb, pos, vel, 2, width=width)
    assert_words(got_p.reshape(-1, 3), want_p.reshape(-1, 3), f"W={width}: positions")
    assert_words(got_v.reshape(-1, 3), want_v.reshape(-1, 3), f"W={width}: velocities")


def three_dimensional(oracle, n=300, b=3):
    pos, vel = K.batch(oracle, (9, n, 1024, 1.0, b))
    rng = np.random.default_rng(9)
    pos[:, :, 2] = rng.uniform(-30, 30, (b, n)).astype(F)
    vel[:, :, 2] = rng.uniform(-0.05, 0.05, (b, n)).astype(F)
    return pos, vel, oracle.camera_constant(30.0, 1.0, 1.0, 10000.0)


@pytest.mark.parametrize("up", [(0, 0, 1), (0.6, 0, 0.8)])
def test_three_dimensional_data_under_a_callers_camera(nb, oracle, up):
    pos, vel, cp = three_dimensional(oracle)
    up = np.array(up, F)
    want_p, want_v = per_scene(nb, pos, vel, 1, cp=cp, up=up)
    got_p, got_v = batch_step(nb, pos, vel, 1, cp=cp, up=up)
    assert_words(got_p.reshape(-1, 3), want_p.reshape(-1, 3), "3-D: positions")
    assert_words(got_v.reshape(-1, 3), want_v.reshape(-1, 3), "3-D: velocities")
    assert (bits(got_v[:, :, 2]) != bits(vel[:, :, 2])).any(1).all()


def test_other_constants(nb, oracle):
    consts = dict(dt=0.05, G=0.02, bias=1e-3)
    pos, vel = K.batch(oracle, K.SIZES[129])
    want_p, want_v = per_scene(nb, pos, vel, 2, consts=consts)
    got_p, got_v = batch_step(nb, pos, vel, 2, consts=consts)
    assert_words(got_p.reshape(-1, 3), want_p.reshape(-1, 3), "other constants: positions")
    assert_words(got_v.reshape(-1, 3), want_v.reshape(-1, 3), "other constants: velocities")
    plain = expected(nb, oracle, K.SIZES[129], 1)
    assert (bits(got_v) != bits(plain[3])).any()


def test_hand_case_in_scene_one_of_three(nb, oracle):
    """DESIGN.md section 13's hand case: eye 0 sees body 1 at column 440, rel = (9 - 2 ulp, 0.98712, 0); eye 1 sees nobody and coasts"""
    pos, vel = K.batch(oracle, (1100, 2, 1024, 1.0, 3))
    pos[1], vel[1] = [[0, 0, 0], [10, 0, 0]], [[1, 0, 0], [1, 0, 0]]
    with nb.SceneBatch(pos, vel) as sb:
        count, ids, depth, col, rel = sb.located()
        assert (count[1] == [1, 0]).all() and ids[1, 0, 0] == 1 and col[1, 0, 0] == 440
        assert (ids[1, 0, 1:] == NONE).all() and (ids[1, 1] == NONE).all() and (col[1, 0, 1:] == NONE).all() and (col[1, 1] == NONE).all()
        assert (bits(rel[1, 0, 0]) == [0x410FFFFE, 0x3F7CB3AE, 0, 0x410FFFFE]).all()
        assert (bits(rel[1, 0, 1:]) == 0).all() and (bits(rel[1, 1]) == 0).all()
        assert (bits(depth[1, 0, 1:]) == 0x3F800000).all() and (bits(depth[1, 1]) == 0x3F800000).all()
        sb.step_nbody_located()
        p, v = sb.positions()[1], sb.velocities()[1]
    assert (bits(p[1]) == bits(F([11, 0, 0]))).all() and (bits(v[1]) == bits(F([1, 0, 0]))).all()
    vec = rel[1, 0, 0, :3]                                             # G2-G3 on that rel, one binary32 operation a step
    dist = ((vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2]) + F(0.0000001)
    total = F([0, 0, 0]) + (vec * F(0.001)) / dist
    want_v = vel[1, 0] + total * F(0.1)
    want_p = want_v + pos[1, 0]
    assert (bits(v[0]) == bits(want_v)).all() and (bits(p[0]) == bits(want_p)).all() and v[0, 0] > 1 and v[0, 1] > 0


def test_more_eyes_than_the_grid_cap(nb, oracle):
    """n = 5 and 209 718 scenes: 1 048 590 eyes, more than the 2^20 workgroups a launch has at most, so some workgroups take a second
    eye, which must start from clean LDS.  The batch repeats three scenes; every copy must get its original's bits"""
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
    assert (bits(got_v) != bits(vel)).any()


# -- SL2, SL4 ----------------------------------------------------------------------------------------------------------------------------
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
            sb.step_nbody_located(1)
        assert sb.steps_done == 3
        assert_words(sb.positions().reshape(-1, 3), want_p.reshape(-1, 3), "three calls: positions")
        assert_words(sb.velocities().reshape(-1, 3), want_v.reshape(-1, 3), "three calls: velocities")


def test_mixed_context_steps_twice(nb, oracle):
    """step(2), step_nbody_located(1), step_boids_seen(1), step_nbody_located(2) against per-scene Scenes doing the same; two runs,
    the same bits"""
    pos, vel = K.batch(oracle, K.SIZES[100])
    want_p, want_v = np.empty_like(pos), np.empty_like(vel)
    for s in range(len(pos)):
        with nb.Scene(pos[s], vel[s]) as sc:
            sc.step_n(2)
            sc.step_nbody_located_n(1)
            sc.step_boids_seen_n(1)
            sc.step_nbody_located_n(2)
            sc.sync()
            sc._refresh(False)
            want_p[s], want_v[s] = sc.state()
    runs = []
    for _ in range(2):
        with nb.SceneBatch(pos, vel) as sb:
            sb.step(2)
            sb.step_nbody_located(1)
            sb.step_boids_seen(1)
            sb.step_nbody_located(2)
            assert sb.steps_done == 6
            p_dev, v_dev, _ = sb.device_state()
            assert p_dev and v_dev
            runs.append((sb.positions(), sb.velocities()))
    assert_words(runs[0][0].reshape(-1, 3), want_p.reshape(-1, 3), "mixed: positions")
    assert_words(runs[0][1].reshape(-1, 3), want_v.reshape(-1, 3), "mixed: velocities")
    assert (bits(runs[0][0]) == bits(runs[1][0])).all() and (bits(runs[0][1]) == bits(runs[1][1])).all()      # SL4


# -- the stateless step launch -----------------------------------------------------------------------------------------------------------
def device_matrices(nb, lib, _lib, torch, t_pos, t_vel, cpm, stream):
    """(cams, inst) tensors (records, 16) of the records t_pos / t_vel, by nb_launch_cameras / nb_launch_instances"""
    records = t_pos.shape[0]
    cams = torch.empty((records, 16), dtype=torch.float32, device=t_pos.device)
    inst = torch.empty((records, 16), dtype=torch.float32, device=t_pos.device)
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
    cpm = np.ascontiguousarray(nb.eye_constant(1024), F).reshape(16)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        cams, inst = device_matrices(nb, lib, _lib, torch, t_pos, t_vel, cpm, s)
        _lib.check(lib.nb_scenes_nbody_located_step_launch(None, b, n, cams.data_ptr(), inst.data_ptr(), UP.ctypes.data, cpm.ctypes.data,
                                                           1024, t_pos.data_ptr(), t_vel.data_ptr(), o_pos.data_ptr() + 16 * n,
                                                           o_vel.data_ptr() + 16 * n, s.cuda_stream))
    s.synchronize()
    gp, gv = o_pos.cpu().numpy(), o_vel.cpu().numpy()
    for got in (gp, gv):
        assert (bits(got[:n]) == 0x7FC0BEEF).all() and (bits(got[-n:]) == 0x7FC0BEEF).all()
        assert (bits(got[n:-n, 3]) == 0).all()
    assert_words(gp[n:-n, :3], want_p.reshape(-1, 3), "stateless: positions")
    assert_words(gv[n:-n, :3], want_v.reshape(-1, 3), "stateless: velocities")
    assert (bits(t_pos.cpu().numpy()) == bits(records_of(pos))).all() and (bits(t_vel.cpu().numpy()) == bits(records_of(vel))).all()


# -- SL3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,width", sorted(K.LISTS))
def test_the_located_sets_are_scene_locateds(nb, oracle, n, width):
    import torch

    from nenbody_amd import _lib

    lib = _lib.load()
    pos, vel = K.batch(oracle, K.LISTS[(n, width)])
    b = len(pos)
    want = scene_located(nb, pos, vel, width)
    want_c = want[0]
    assert (want_c == 0).any(1).all() and ((want_c > 0).mean(1) > 0.5).all() and want_c.max() > 1
    with nb.SceneBatch(pos, vel) as sb:
        got = sb.located(width=width)
        got = (got[0], got[1], bits(got[2]), got[3], bits(got[4]))
        for name, g, w in zip(("count", "ids", "depth", "col", "rel"), got, want):
            assert g.shape == w.shape and (g == w).all(), name
        sub = sb.located(first_scene=1, scene_count=2, width=width)
        sub = (sub[0], sub[1], bits(sub[2]), sub[3], bits(sub[4]))
        for name, g, w in zip(("count", "ids", "depth", "col", "rel"), sub, want):
            assert (g == w[1:]).all(), name
        empty = sb.located(first_scene=3, scene_count=0, width=width)
        assert empty[1].shape == (0, n, width) and empty[4].shape == (0, n, width, 4)
    # nb_scenes_located_launch over a range of eyes that starts and ends inside a scene; every word of the outputs is written
    dev = torch.device("cuda", 0)
    t_pos, t_vel = torch.from_numpy(records_of(pos)).to(dev), torch.from_numpy(records_of(vel)).to(dev)
    first, count = n // 2, b * n - n // 2 - 7
    cpm = np.ascontiguousarray(nb.eye_constant(width), F).reshape(16)
    flat = [want[0].reshape(-1), want[1].reshape(-1, width), want[2].reshape(-1, width), want[3].reshape(-1, width),
            want[4].reshape(-1, width * 4)]
    s = torch.cuda.Stream(dev)
    for only_rel in (False, True):
        outs = [torch.full((count + 1,) + f.shape[1:], FILL, dtype=torch.int32, device=dev) for f in flat]
        ptrs = [None if only_rel and a < 4 else o.data_ptr() for a, o in enumerate(outs)]
        with torch.cuda.stream(s):
            cams, inst = device_matrices(nb, lib, _lib, torch, t_pos, t_vel, cpm, s)
            _lib.check(lib.nb_scenes_located_launch(b, n, first, count, cams.data_ptr(), inst.data_ptr(), t_vel.data_ptr(), UP.ctypes.data,
                                                    cpm.ctypes.data, width, *ptrs, s.cuda_stream))
        s.synchronize()
        for a, (o, f) in enumerate(zip(outs, flat)):
            g = o.cpu().numpy().view(np.uint32)
            if ptrs[a] is None:
                assert (g == FILL).all()
            else:
                assert (g[:count] == f[first:first + count]).all() and (g[count] == FILL).all(), (only_rel, a)


# -- the context's refusals that need a device --------------------------------------------------------------------------------------------
def test_context_entries_refuse_with_their_texts(nb, oracle):
    from nenbody_amd import _lib

    lib = _lib.load()
    cp = np.ascontiguousarray(nb.eye_constant(64), F).reshape(16)
    flat = cp.copy()
    flat[11] = 0
    skew = cp.copy()
    skew[4] = 0.25
    null = cp.copy()
    null[14] = 0
    up, cpp = UP.ctypes.data, cp.ctypes.data
    buf = np.zeros(7 * (3 * 8 * 64) + 64, np.uint32)
    out = buf.ctypes.data
    cells = 3 * 8 * 64 * 4
    o = [out, out + 128, out + 128 + cells, out + 128 + 2 * cells, out + 128 + 3 * cells]     # count, ids, depth, col, rel (16-aligned or not: host)
    err = lambda ctx: lib.nb_scenes_last_error(ctx).decode()
    St, Ey = "nb_scenes_step_nbody_located: ", "nb_scenes_eyes_located: "
    shape = " (a perspective constant as nb_camera_constant forms it)"
    ctx = ctypes.c_void_p()
    _lib.check(lib.nb_scenes_create(3, 8, None, ctypes.byref(ctx)))
    try:
        assert lib.nb_scenes_step_nbody_located(ctx, 1, up, cpp, 64) == _lib.NB_ERR_STATE
        assert err(ctx) == St + "no state uploaded (call nb_scenes_upload first)"
        assert lib.nb_scenes_eyes_located(ctx, 0, 3, up, cpp, 64, *o) == _lib.NB_ERR_STATE
        assert err(ctx) == Ey + "no state uploaded (call nb_scenes_upload first)"
        assert lib.nb_scenes_step_nbody_located(ctx, 1, up, cpp, 0) == _lib.NB_ERR_INVALID          # the arguments come first
        assert err(ctx) == St + "width must be 1 .. NB_EYES_MAX_WIDTH (4096)"
        assert lib.nb_scenes_step_nbody_located(ctx, 1, up, flat.ctypes.data, 64) == _lib.NB_ERR_INVALID
        assert err(ctx) == St + "cp16 cannot be inverted: cp16[11] must be -1" + shape
    finally:
        lib.nb_scenes_destroy(ctx)
    pos, vel = K.batch(oracle, (1100, 8, 64, 0.1, 3))
    with nb.SceneBatch(pos, vel) as sb:
        c = sb._ctx
        for args, text in (((1, None, cpp, 64), "null argument"), ((1, up, None, 64), "null argument"),
                           ((1, up, cpp, 4097), "width must be 1 .. NB_EYES_MAX_WIDTH (4096)"),
                           ((1, up, cpp, 0), "width must be 1 .. NB_EYES_MAX_WIDTH (4096)"),
                           ((1, up, flat.ctypes.data, 64), "cp16 cannot be inverted: cp16[11] must be -1" + shape),
                           ((1, up, skew.ctypes.data, 64), "cp16 cannot be inverted: cp16[4] must be 0" + shape),
                           ((1, up, null.ctypes.data, 64), "cp16 cannot be inverted: cp16[14] must not be 0" + shape),
                           ((1, up, flat.ctypes.data, 0), "width must be 1 .. NB_EYES_MAX_WIDTH (4096)")):
            assert lib.nb_scenes_step_nbody_located(c, *args) == _lib.NB_ERR_INVALID, args
            assert err(c) == St + text
        assert sb.steps_done == 0
        for args, text in (((0, 3, None, cpp, 64, *o), "null argument"), ((0, 3, up, cpp, 0, *o), "width must be 1 .. NB_EYES_MAX_WIDTH (4096)"),
                           ((0, 3, up, flat.ctypes.data, 64, *o), "cp16 cannot be inverted: cp16[11] must be -1" + shape),
                           ((1, 3, up, cpp, 64, *o), "scenes [first_scene, first_scene + scene_count) exceed the batch"),
                           ((0, 3, up, cpp, 64, None, None, None, None, None),
                            "seen_count, seen_ids, seen_depth, seen_col and seen_rel are all NULL"),
                           ((0, 3, up, cpp, 64, o[0], o[1], o[1] + 4, o[3], o[4]), "the outputs must not overlap each other or an input")):
            assert lib.nb_scenes_eyes_located(c, *args) == _lib.NB_ERR_INVALID, args
            assert err(c) == Ey + text
        assert lib.nb_scenes_step_nbody_located(c, 0, up, cpp, 64) == _lib.NB_OK and sb.steps_done == 0        # k = 0: a checked no-op
        assert lib.nb_scenes_eyes_located(c, 0, 3, up, cpp, 64, o[0], None, None, None, None) == _lib.NB_OK     # one output is enough
        assert lib.nb_scenes_eyes_located(c, 0, 3, up, cpp, 64, None, None, None, None, o[4]) == _lib.NB_OK
        with pytest.raises(nb.NbError, match="cp16 cannot be inverted"):
            sb.step_nbody_located(1, 64, cp=flat.reshape(4, 4))


# -- the C++ host ------------------------------------------------------------------------------------------------------------------------
def test_cpp_host_matches_the_contexts(nb, oracle, tmp_path):
    from test_scenes_located_cpu import EXE, build_exe

    build_exe()
    row = K.SIZES[100]
    b, n, width, k = row[4], 100, 1024, 1
    assert row[0] == 1100 and row[3] == 1.0                             # the program draws seeds 1100, 1101, ... unscaled
    out = tmp_path / "out.bin"
    r = subprocess.run([EXE, str(b), str(n), str(width), str(k), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, dtype=np.uint32)
    eyes = b * n
    cells = eyes * width
    cuts = np.cumsum([eyes, cells, cells, cells, 4 * cells, 3 * eyes])
    count, ids, depth, col, rel, p, v = np.split(raw, cuts)
    pos, vel, want_p, want_v = expected(nb, oracle, row, k)
    want = scene_located(nb, pos, vel, width)
    for name, g, w in zip(("count", "ids", "depth", "col", "rel"), (count, ids, depth, col, rel), want):
        assert (g == w.reshape(-1)).all(), name
    assert_words(p.view(F).reshape(-1, 3), want_p.reshape(-1, 3), "C++: positions")
    assert_words(v.view(F).reshape(-1, 3), want_v.reshape(-1, 3), "C++: velocities")


# -- the floor ---------------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_64_scenes_beats_64_contexts_fourfold(nb, oracle):
    """n = 100, B = 64, W = 1024, k = 4: the batch's step against the only way the library offered before, 64 contexts'
    nb_step_nbody_located(4) issued back to back -- wall time to the last sync, median of 5, after a warm-up, the procedure of
    test_gpu_scenes_seen.py::test_a_batch_of_64_scenes_beats_64_contexts_fourfold.  A quarter is that test's own convention."""
    k = 4
    pos, vel = K.batch(oracle, K.FLOOR)
    batch = len(pos)
    assert batch == 64

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
        t_batch = timed(lambda: sb.step_nbody_located(k), sb.sync)
    ctxs = [nb.Scene(pos[s], vel[s]) for s in range(batch)]
    try:
        t_ctx = timed(lambda: [sc.step_nbody_located_n(k) for sc in ctxs], lambda: [sc.sync() for sc in ctxs])
    finally:
        for sc in ctxs:
            sc.close()
    print(f"batch {t_batch * 1e3:.3f} ms, {batch} contexts {t_ctx * 1e3:.3f} ms, ratio {t_ctx / t_batch:.1f}")
    assert t_batch < t_ctx / 4, (t_batch, t_ctx)
