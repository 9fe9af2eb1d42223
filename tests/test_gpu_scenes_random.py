"""Randomised differential tests of the four scene-batch kernels: the seeded problems of
tests/scenes_random_cases.py, every word compared as bit patterns, a NaN of the reference met by a NaN.  No tolerances.

Gravity and boids (scenes_nbody_kernel, scenes_boids_kernel) go through the stateless in-place launches between two guard scenes of
NaN records and are compared with the C oracle scene by scene.  The seen boids step and gravity from located vision
(scenes_boids_seen_kernel, scenes_nbody_located_kernel) go through their stateless step launches, one launch a step with the cameras
and model matrices formed on the device in between, and are compared with the numpy restatements chained step by step and scene by
scene (scenes_random_cases.vision_expected); for problems of one step the lists nb_scenes_seen_launch / nb_scenes_located_launch emit
are compared too, padding included.  The two fused kernels repeat the raster loop and the fold's pair code as text; these problems and
the hand-picked rows of test_gpu_scenes_seen.py / test_gpu_scenes_located.py are what ties them to the kernels they copy.

Every failure prints the case's line: scenes_random_cases.case(law, i) draws the same problem again.  NB_RANDOM_CASES=N widens every
family to N cases."""
import ctypes

import numpy as np
import pytest

import eyes_restatement as R
import scenes_cases as SC
import scenes_random_cases as C
import scenes_restatement as SR
import seen_cases as SK
from test_gpu_scenes import launch

pytestmark = pytest.mark.gpu

F = np.float32
FILL = 0x07070707
GUARD = 0x7FC0BEEF


def differing(got, want, n):
    """[(scene, body)] of the records (rows of the last axis) that differ, a NaN of the reference met by a NaN"""
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert g.shape == w.shape, (g.shape, w.shape)
    ok = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    rows = np.nonzero(~ok.reshape(-1, ok.shape[-1]).all(1))[0]
    return [divmod(int(r), n) for r in rows]


def assert_state(got, want, c):
    for g, w, name in zip(got, want, ("positions", "velocities")):
        bad = differing(g[..., :3], w, c["n"])
        assert not bad, f"{name} of {len(bad)} bodies differ, first (scene, body) {bad[:6]}: {c['line']}"


# ---- gravity and boids ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(C.CASES))
def test_gravity_random_batches_bit_exact(nb, oracle, i):
    c = C.case("nbody", i)
    want = SR.nbody(oracle, c["pos"], c["vel"], c["k"], **{key: F(val) for key, val in c["consts"].items()})
    got = launch(nb, "nbody", c["pos"], c["vel"], c["k"], SC.gravity_params(nb, **c["consts"]))
    assert_state(got, want, c)


@pytest.mark.parametrize("i", range(C.CASES))
def test_boids_random_batches_bit_exact(nb, oracle, i):
    c = C.case("boids", i)
    want = SR.boids(oracle, c["pos"], c["vel"], c["k"], SK.oracle_params(oracle, **c["consts"]))
    got = launch(nb, "boids", c["pos"], c["vel"], c["k"], SK.device_params(nb, **c["consts"]))
    assert_state(got, want, c)


# ---- the two vision laws ----------------------------------------------------------------------------------------------------------------
def records_of(a):
    r = np.zeros(a.shape[:-1] + (4,), F)
    r[..., :3] = a
    return r.reshape(-1, 4)


def vision_run(nb, oracle, c):
    """the case's k steps through the stateless step launch of its law, every step's outputs between two guard scenes that must come
    back untouched: ((pos, vel) (B, n, 3), the lists of the first step as the list launch emits them, with one row of FILL behind)"""
    import torch

    from nenbody_amd import _lib

    lib = _lib.load()
    law, b, n, width = c["law"], c["batch"], c["n"], c["width"]
    eyes = b * n
    dev = torch.device("cuda", 0)
    up = np.ascontiguousarray(c["up"], F)
    cp = np.ascontiguousarray(R.eye_constant(oracle, width), F).reshape(16)
    if law == "seen":
        params = SK.device_params(nb, **c["consts"])
    else:
        params = nb.default_params()
        params.dt, params.G, params.bias = c["consts"]["dt"], c["consts"]["g"], c["consts"]["bias"]
    t_pos, t_vel = torch.from_numpy(records_of(c["pos"])).to(dev), torch.from_numpy(records_of(c["vel"])).to(dev)
    cams = torch.empty((eyes, 16), dtype=torch.float32, device=dev)
    inst = torch.empty((eyes, 16), dtype=torch.float32, device=dev)
    guard = np.full(((b + 2) * n, 4), np.uint32(GUARD).view(F), F)
    widths = (1, width) if law == "seen" else (1, width, width, width, 4 * width)          # count, ids[, depth, col, rel]
    lists = [torch.full((eyes + 1, w), FILL, dtype=torch.int32, device=dev) for w in widths]
    torch.cuda.synchronize(dev)                                       # the fills above ran on the default stream
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        for step in range(c["k"]):
            o_pos, o_vel = torch.from_numpy(guard.copy()).to(dev), torch.from_numpy(guard.copy()).to(dev)
            _lib.check(lib.nb_launch_instances(eyes, t_pos.data_ptr(), t_vel.data_ptr(), inst.data_ptr(), s.cuda_stream))
            _lib.check(lib.nb_launch_cameras(eyes, t_pos.data_ptr(), t_vel.data_ptr(), up.ctypes.data, cp.ctypes.data, cams.data_ptr(),
                                             s.cuda_stream))
            outs = (o_pos.data_ptr() + 16 * n, o_vel.data_ptr() + 16 * n)
            if law == "seen":
                if step == 0:
                    _lib.check(lib.nb_scenes_seen_launch(b, n, 0, eyes, cams.data_ptr(), inst.data_ptr(), width,
                                                         *[t.data_ptr() for t in lists], s.cuda_stream))
                _lib.check(lib.nb_scenes_boids_seen_step_launch(ctypes.byref(params), b, n, cams.data_ptr(), inst.data_ptr(), width,
                                                                t_pos.data_ptr(), t_vel.data_ptr(), *outs, s.cuda_stream))
            else:
                if step == 0:
                    _lib.check(lib.nb_scenes_located_launch(b, n, 0, eyes, cams.data_ptr(), inst.data_ptr(), t_vel.data_ptr(),
                                                            up.ctypes.data, cp.ctypes.data, width, *[t.data_ptr() for t in lists],
                                                            s.cuda_stream))
                _lib.check(lib.nb_scenes_nbody_located_step_launch(ctypes.byref(params), b, n, cams.data_ptr(), inst.data_ptr(),
                                                                   up.ctypes.data, cp.ctypes.data, width, t_pos.data_ptr(),
                                                                   t_vel.data_ptr(), *outs, s.cuda_stream))
            s.synchronize()
            for o, name in ((o_pos, "pos_out"), (o_vel, "vel_out")):
                g = o.cpu().numpy().view(np.uint32)
                assert (g[:n] == GUARD).all() and (g[-n:] == GUARD).all(), f"step {step}: a guard scene of {name} was written: {c['line']}"
                assert (g[n:-n, 3] == 0).all(), f"step {step}: w of {name} is not +0: {c['line']}"
            t_pos, t_vel = o_pos[n:-n].clone(), o_vel[n:-n].clone()
    state = tuple(t.cpu().numpy()[:, :3].reshape(b, n, 3) for t in (t_pos, t_vel))
    return state, [t.cpu().numpy().view(np.uint32) for t in lists]


def assert_lists(got, want, c):
    """the emitted lists against the restatement's, padding included, and the row behind the last eye untouched"""
    b, n, width = c["batch"], c["n"], c["width"]
    names = ("count", "ids", "depth", "col", "rel")
    for a, (g, w) in enumerate(zip(got, want)):
        assert (g[-1] == FILL).all(), f"{names[a]}: written behind the last eye: {c['line']}"
        g = g[:-1].reshape(b * n, -1)
        if w.dtype == np.float32:
            w = w.reshape(b * n, -1)
            ok = (g == w.view(np.uint32)) | (np.isnan(g.view(F)) & np.isnan(w))
        else:
            ok = g == w.reshape(b * n, -1)
        bad = [divmod(int(r), n) for r in np.nonzero(~ok.all(1))[0]]
        assert not bad, f"{names[a]} of {len(bad)} eyes differ, first (scene, eye) {bad[:6]}: {c['line']}"


@pytest.mark.parametrize("law,i", [(law, i) for law in ("seen", "located") for i in range(C.CASES)])
def test_vision_random_batches_bit_exact(nb, oracle, law, i):
    c = C.case(law, i)
    want_p, want_v, want_lists = C.vision_expected(oracle, law, i)
    state, lists = vision_run(nb, oracle, c)
    if c["k"] == 1:
        assert_lists(lists, want_lists, c)
    assert_state(state, (want_p, want_v), c)
