"""GPU tests of scene batches: B scenes of n <= 2 048 bodies stepped k times by one launch, one workgroup per
scene.  Every word of every record is compared with tests/scenes_restatement.py -- the C oracle applied scene by scene --, a NaN of
the reference met by a NaN.  Every stateless launch runs inside a larger tensor with one guard scene of NaN records in front of the
batch and one behind it, which must come back untouched (B3).  tests/test_scenes_cpu.py shows on the same data that stepping two
scenes as one set differs from stepping them apart."""
import ctypes
import statistics
import subprocess
import time

import numpy as np
import pytest

import scenes_cases as K
import scenes_restatement as R
import seen_cases as SK
from seen_cases import same_words
from test_gpu_boids import matrices_equal

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [1, 2, 63, 64, 65, 100, 255, 256, 257, 1023, 1024, 1025, 2047, 2048]
GRID_CAP = 2048                                             # nb_scenes.h: kScenesMaxGrid
BIG = F(2.0 ** 64)                                          # a coordinate where the ladder gives NaN and '/' gives 0


def launch(nb, law, pos, vel, k, params=None, launches=1):
    """`launches` launches of k steps each on a (B + 2, n, 4) tensor whose first and last scene are NaN guards; returns the batch's
    (pos, vel) records, (B, n, 4) each, after checking that w is 0 and that the guards kept every bit"""
    import torch

    from nenbody_amd import _lib

    batch, n = pos.shape[:2]
    dev = torch.device("cuda", 0)

    def rec(a):
        r = np.full((batch + 2, n, 4), np.nan, F)
        r[1:-1, :, :3] = a
        r[1:-1, :, 3] = 0
        return r

    hp, hv = rec(pos), rec(vel)
    tp, tv = torch.from_numpy(hp).to(dev), torch.from_numpy(hv).to(dev)
    entry = _lib.load().nb_scenes_nbody_step_launch if law == "nbody" else _lib.load().nb_scenes_boids_step_launch
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        for _ in range(launches):
            _lib.check(entry(ctypes.byref(params) if params is not None else None, batch, n, k, tp.data_ptr() + n * 16,
                             tv.data_ptr() + n * 16, s.cuda_stream))
    s.synchronize()
    gp, gv = tp.cpu().numpy(), tv.cpu().numpy()
    for g, h, name in ((gp, hp, "pos"), (gv, hv, "vel")):
        for guard in (0, -1):
            assert (g[guard].view(np.uint32) == h[guard].view(np.uint32)).all(), f"{name}: guard scene {guard} was written"
        if k * launches:
            assert (g[1:-1, :, 3].view(np.uint32) == 0).all(), f"{name}: w is not +0"
    return gp[1:-1], gv[1:-1]


def assert_scenes(got, want, what):
    for g, w, name in zip(got, want, ("positions", "velocities")):
        batch, n = w.shape[:2]
        ok, rows = same_words(g[:, :, :3].reshape(batch * n, 3), w.reshape(batch * n, 3))
        assert ok, f"{what}: {name} of {len(rows)} of {batch * n} bodies differ, first (scene, body) {[divmod(int(r), n) for r in rows[:6]]}"


def restate(oracle, law, pos, vel, k, constants=None, oparams=None):
    return R.nbody(oracle, pos, vel, k, **(constants or {})) if law == "nbody" else R.boids(oracle, pos, vel, k, oparams)


# -- sizes: every workgroup size, both sides of the one-to-two-bodies-per-lane line -------------------------------------------------------
@pytest.mark.parametrize("law", ["nbody", "boids"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_batches_and_step_counts(nb, oracle, law, n):
    pos, vel = K.scenes(oracle, law, 3, n, seed=100 + n)
    for k in (1, 2, 5):
        want = restate(oracle, law, pos, vel, k)                       # scene by scene: scene 0 alone is its first row
        for batch in (1, 3):
            got = launch(nb, law, pos[:batch], vel[:batch], k)
            assert_scenes(got, tuple(w[:batch] for w in want), f"{law} n={n} B={batch} k={k}")


@pytest.mark.parametrize("law", ["nbody", "boids"])
def test_more_scenes_than_the_grid_cap(nb, oracle, law):
    batch, n, k = GRID_CAP + 52, 5, 2
    pos, vel = K.scenes(oracle, law, batch, n, seed=9000)
    assert_scenes(launch(nb, law, pos, vel, k), restate(oracle, law, pos, vel, k), f"{law}: {batch} scenes")


# -- both laws under other constants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 257, 1025])
def test_gravity_under_a_second_set_of_constants(nb, oracle, n):
    pos, vel = K.scenes(oracle, "nbody", 3, n, seed=300 + n)
    got = launch(nb, "nbody", pos, vel, 3, K.gravity_params(nb, **K.ALT_GRAVITY))
    assert_scenes(got, R.nbody(oracle, pos, vel, 3, **K.ALT_GRAVITY), f"n={n}")


@pytest.mark.parametrize("n", [65, 300, 1100])
def test_boids_where_every_rule_cuts(nb, oracle, n):
    """tests/test_gpu_seen_contract.py's constants on its data: each rule holds for some pairs and fails for others"""
    out = [SK.cut_cloud(oracle, n, 5 + s) for s in range(3)]
    pos, vel = np.stack([p for p, _ in out]), np.stack([v for _, v in out])
    got = launch(nb, "boids", pos, vel, 2, SK.device_params(nb, **SK.CUT))
    assert_scenes(got, R.boids(oracle, pos, vel, 2, SK.oracle_params(oracle, **SK.CUT)), f"n={n}")


def test_boids_radius_boundaries(nb, oracle):
    """pairs exactly at, just inside and just outside rule 2's 5.0 and rule 1's sqrt(1000), under the reference's constants; the
    same rows shifted make the other scenes"""
    p0, v0 = SK.boundary_rows()
    pos = np.stack([p0, p0 + F(0.25), p0[::-1].copy()])
    vel = np.stack([v0, v0, v0[::-1].copy()])
    assert_scenes(launch(nb, "boids", pos, vel, 1), R.boids(oracle, pos, vel, 1), "boundaries")


# -- isolation (B3) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", ["nbody", "boids"])
def test_a_scene_of_non_finite_records_leaves_its_neighbours_alone(nb, oracle, law):
    n, k = 130, 3
    pos, vel = K.scenes(oracle, law, 3, n, seed=40)
    clean = launch(nb, law, pos, vel, k)
    pos[1, 0::3], pos[1, 1::3], pos[1, 2::3] = np.nan, np.inf, -np.inf
    vel[1, ::2] = np.nan
    got = launch(nb, law, pos, vel, k)
    assert_scenes(got, restate(oracle, law, pos, vel, k), law)
    for g, c in zip(got, clean):
        assert (g[[0, 2]].view(np.uint32) == c[[0, 2]].view(np.uint32)).all()


@pytest.mark.parametrize("law", ["nbody", "boids"])
@pytest.mark.parametrize("n", [100, 1500])
def test_one_launch_of_k_steps_is_k_launches_and_a_batch_is_its_scenes_apart(nb, oracle, law, n):
    k = 4
    pos, vel = K.scenes(oracle, law, 3, n, seed=50 + n)
    want = restate(oracle, law, pos, vel, k)
    once = launch(nb, law, pos, vel, k)
    assert_scenes(once, want, "one launch")
    again = launch(nb, law, pos, vel, k)
    stepwise = launch(nb, law, pos, vel, 1, launches=k)
    for a, b, c in zip(once, again, stepwise):
        assert (a.view(np.uint32) == b.view(np.uint32)).all(), "two runs differ"
        assert (a.view(np.uint32) == c.view(np.uint32)).all(), "k launches of one step differ from one launch of k steps"
    for s in range(3):
        alone = launch(nb, law, pos[s:s + 1], vel[s:s + 1], k)
        for a, b in zip(once, alone):
            assert (a[s].view(np.uint32) == b[0].view(np.uint32)).all(), f"scene {s} alone differs"


# -- the divide guard, where a missed flag must show ---------------------------------------------------------------------------------------
GUARD_CASES = {                      # name: (n, (scene, body) of the 2^64 coordinate)
    "own body, first lane": (100, (1, 0)),
    "another body, last of the scene": (100, (1, 99)),
    "j < 1024 of 2048": (2048, (1, 5)),
    "j >= 1024 of 2048": (2048, (1, 1500)),
    "scene 0 only": (300, (0, 150)),
    "last scene only": (300, (2, 150)),
}


@pytest.mark.parametrize("name", list(GUARD_CASES))
def test_divide_guard_one_coordinate_of_2_to_the_64(nb, oracle, name):
    n, (scene, body) = GUARD_CASES[name]
    pos, vel = K.scenes(oracle, "nbody", 3, n, seed=60)
    pos[scene, body, 1] = BIG
    want = R.nbody(oracle, pos, vel, 2)
    assert np.isfinite(want[1]).all()                      # '/' gives 0 where the ladder would give NaN
    assert_scenes(launch(nb, "nbody", pos, vel, 2), want, name)


@pytest.mark.parametrize("n", [100, 1500])
def test_divide_guard_arising_mid_launch(nb, oracle, n):
    """every position in range at launch, one velocity of 2^64: from step 2 on that body lies outside the ladder's range, which only a
    flag recomputed per step catches"""
    pos, vel = K.scenes(oracle, "nbody", 3, n, seed=70)
    vel[1, n // 2, 0] = BIG
    want = R.nbody(oracle, pos, vel, 3)
    assert np.isfinite(want[1]).all()
    assert_scenes(launch(nb, "nbody", pos, vel, 3), want, f"n={n}")


# -- the planar shortcut -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 1500])
def test_a_scene_that_leaves_the_plane_after_step_one(nb, oracle, n):
    pos, vel = K.scenes(oracle, "nbody", 3, n, seed=80)
    assert not pos[..., 2].any() and not vel[..., 2].any()
    vel[1, n - 1, 2] = 1
    want = R.nbody(oracle, pos, vel, 3)
    assert want[0][1, :, 2].all() and not want[0][0, :, 2].any()      # scene 1 is 3-D by step 3, scene 0 stays planar
    assert_scenes(launch(nb, "nbody", pos, vel, 3), want, f"n={n}")


def test_three_dimensional_gravity_from_the_start(nb, oracle):
    pos, vel = K.scenes(oracle, "boids", 3, 257, seed=81)             # the 3-D clouds
    assert_scenes(launch(nb, "nbody", pos, vel, 3), R.nbody(oracle, pos, vel, 3), "3-D")


@pytest.mark.parametrize("knob", ["NB_FORCE_3D", "NB_STRICT_FORCE_IEEE"])
def test_forced_paths_give_the_same_bits(nb, oracle, monkeypatch, knob):
    pos, vel = K.scenes(oracle, "nbody", 3, 300, seed=82)
    plain = launch(nb, "nbody", pos, vel, 3)
    monkeypatch.setenv(knob, "1")
    forced = launch(nb, "nbody", pos, vel, 3)
    assert_scenes(forced, R.nbody(oracle, pos, vel, 3), knob)
    for a, b in zip(plain, forced):
        assert (a.view(np.uint32) == b.view(np.uint32)).all()


# -- the context ---------------------------------------------------------------------------------------------------------------------------
def test_context_steps_mixed_against_per_scene_scenes(nb, oracle):
    from nenbody_amd import _lib

    batch, n = 3, 100
    pos, vel = K.scenes(oracle, "nbody", batch, n, seed=1234)
    with nb.SceneBatch(pos, vel) as sb:
        assert sb.steps_done == 0
        for _ in range(2):                                            # two runs of every entry give identical bits
            sb._check(_lib.load().nb_scenes_upload(sb._ctx, pos.ctypes.data, vel.ctypes.data))
            sb.step(2)
            sb.step_boids(1)
            sb.step()
            sb.sync()
            run = (sb.positions(), sb.velocities(), sb.instances())
            first = run if _ == 0 else first
        assert sb.steps_done == 4
    for a, b in zip(first, run):
        assert (a.view(np.uint32) == b.view(np.uint32)).all()
    for s in range(batch):
        with nb.Scene(pos[s], vel[s]) as sc:
            sc.step_n(2)
            sc.step_boids_n(1)
            sc.step_n(1)
            p, v = sc.state()
            inst = sc.instances()
        assert (run[0][s].view(np.uint32) == p.view(np.uint32)).all() and (run[1][s].view(np.uint32) == v.view(np.uint32)).all(), s
        assert matrices_equal(run[2][s], inst), s
    # and against the restatement, so that the two hosts cannot be wrong together
    p, v = R.nbody(oracle, pos, vel, 2)
    p, v = R.boids(oracle, p, v, 1)
    p, v = R.nbody(oracle, p, v, 1)
    assert (run[0].view(np.uint32) == p.view(np.uint32)).all() and (run[1].view(np.uint32) == v.view(np.uint32)).all()


def test_new_draws_scene_s_from_seed_plus_s_and_new_SceneBatch_is_the_initial_state(nb, oracle):
    with nb.SceneBatch.new(3, 65, 11) as sb:
        p, v = sb.positions(), sb.velocities()
    for s in range(3):
        po, vo = oracle.init_state(65, 11 + s)
        assert (p[s].view(np.uint32) == po.view(np.uint32)).all() and (v[s].view(np.uint32) == vo.view(np.uint32)).all()


def test_context_refuses_a_step_before_an_upload(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    ctx = ctypes.c_void_p()
    _lib.check(lib.nb_scenes_create(2, 10, None, ctypes.byref(ctx)))
    try:
        buf = np.zeros(2 * 10 * 16, F)
        for rc, fn in ((lib.nb_scenes_step(ctx, 1), "nb_scenes_step"), (lib.nb_scenes_step_boids(ctx, 1, None), "nb_scenes_step_boids"),
                       (lib.nb_scenes_download(ctx, buf.ctypes.data, None, None), "nb_scenes_download"),
                       (lib.nb_scenes_device_state(ctx, None, None, None), "nb_scenes_device_state")):
            assert rc == _lib.NB_ERR_STATE, fn
        assert lib.nb_scenes_step(ctx, 1) == _lib.NB_ERR_STATE
        assert lib.nb_scenes_last_error(ctx).decode() == "nb_scenes_step: no state uploaded (call nb_scenes_upload first)"
        assert lib.nb_scenes_download(ctx, None, None, None) == _lib.NB_ERR_INVALID
        assert lib.nb_scenes_last_error(ctx).decode() == "nb_scenes_download: pos_xyz, vel_xyz and inst_16 are all NULL"
        assert lib.nb_scenes_upload(ctx, None, buf.ctypes.data) == _lib.NB_ERR_INVALID
    finally:
        lib.nb_scenes_destroy(ctx)


def test_device_state_feeds_the_eye_launch_for_one_scene(nb, oracle):
    """scene 1 of 3 through pointer offsets, n_total = n: the rows Scene.eyes gives that scene's state"""
    import torch

    from nenbody_amd import _lib

    lib = _lib.load()
    batch, n, width = 3, 64, 128
    pos, vel = K.scenes(oracle, "nbody", batch, n, seed=21)
    pos *= F(0.1)                                                     # close enough to see one another
    up, cp = np.array([0, 0, 1], F), np.ascontiguousarray(nb.eye_constant(width), F).reshape(16)
    dev = torch.device("cuda", 0)
    with nb.SceneBatch(pos, vel) as sb:
        sb.step(2)
        p, v, inst = sb.device_state()
        sb.sync()
        state = sb.positions()[1], sb.velocities()[1]
        cams = torch.empty((n, 16), dtype=torch.float32, device=dev)
        ids = torch.empty((n, width), dtype=torch.int32, device=dev)
        depth = torch.empty((n, width), dtype=torch.float32, device=dev)
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            _lib.check(lib.nb_launch_cameras(n, p + n * 16, v + n * 16, up.ctypes.data, cp.ctypes.data, cams.data_ptr(), s.cuda_stream))
            _lib.check(lib.nb_launch_eyes(n, 0, n, cams.data_ptr(), inst + n * 64, width, 0, ids.data_ptr(), depth.data_ptr(), s.cuda_stream))
        s.synchronize()
        got_ids, got_depth = ids.cpu().numpy().view(np.uint32), depth.cpu().numpy()
    with nb.Scene(*state) as sc:
        want_ids, want_depth = sc.eyes(width=width)
    assert (want_ids != _lib.NB_EYES_NONE).any()
    assert (got_ids == want_ids).all() and (got_depth.view(np.uint32) == want_depth.view(np.uint32)).all()


def test_cpp_host_matches_the_restatement(nb, oracle, tmp_path):
    from test_scenes_cpu import EXE, build_exe

    build_exe()
    batch, n, k = 3, 100, 2
    out = tmp_path / "out.bin"
    r = subprocess.run([EXE, str(batch), str(n), str(k), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, dtype=F)
    total = batch * n
    p, v, inst = raw[:3 * total].reshape(batch, n, 3), raw[3 * total:6 * total].reshape(batch, n, 3), raw[6 * total:].reshape(batch, n, 4, 4)
    pos, vel = K.scenes(oracle, "nbody", batch, n, seed=1234)
    pw, vw = R.nbody(oracle, pos, vel, k)
    pw, vw = R.boids(oracle, pw, vw, 1)
    pw, vw = R.nbody(oracle, pw, vw, 1)
    assert (p.view(np.uint32) == pw.view(np.uint32)).all() and (v.view(np.uint32) == vw.view(np.uint32)).all()
    assert all(matrices_equal(inst[s], oracle.instances(pw[s], vw[s])) for s in range(batch))


# -- the floor ------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_256_small_scenes_beats_256_contexts_fourfold(nb, oracle):
    """n = 100, B = 256, k = 8: the batch launch against the only way the library offered before, 256 contexts' nb_step(8) issued
    back to back -- wall time to the last sync, median of 5, after a warm-up.  A quarter against an expected hundredfold."""
    batch, n, k = 256, 100, 8
    pos, vel = K.scenes(oracle, "nbody", batch, n, seed=1)

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
        t_batch = timed(lambda: sb.step(k), sb.sync)
    ctxs = [nb.Scene(pos[s], vel[s]) for s in range(batch)]
    try:
        t_ctx = timed(lambda: [sc.step_n(k) for sc in ctxs], lambda: [sc.sync() for sc in ctxs])
    finally:
        for sc in ctxs:
            sc.close()
    print(f"batch {t_batch * 1e3:.3f} ms, {batch} contexts {t_ctx * 1e3:.3f} ms, ratio {t_ctx / t_batch:.1f}")
    assert t_batch < t_ctx / 4, (t_batch, t_ctx)
