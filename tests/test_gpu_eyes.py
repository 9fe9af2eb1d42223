"""GPU tests of every entity's eye view (nb_eyes / nb_launch_eyes): the HIP kernel against the numpy
restatement of the rule (tests/eyes_restatement.py), ids and depth bit for bit, with cameras and model matrices by the oracle."""
import ctypes

import numpy as np
import pytest

import eyes_restatement as R

pytestmark = pytest.mark.gpu

F = np.float32
UP = np.array([0, 0, 1], np.float32)


def expect(oracle, pos, vel, rows, width=1024, cp=None, up=UP, see_self=False):
    """the rule for the eyes of `rows` (ascending body indices) of the state (pos, vel)"""
    cp = R.eye_constant(oracle, width) if cp is None else cp
    cams = oracle.cameras(pos[rows], vel[rows], up, cp)
    inst = oracle.instances(pos, vel)
    rows = np.asarray(rows)
    ids = np.empty((len(rows), width), np.uint32)
    depth = np.empty((len(rows), width), F)
    i = 0
    while i < len(rows):   # runs of consecutive eyes in one call
        k = i + 1
        while k < len(rows) and rows[k] == rows[k - 1] + 1:
            k += 1
        ids[i:k], depth[i:k] = R.eyes(cams[i:k], inst, int(rows[i]), width, see_self)
        i = k
    return ids, depth


def assert_same(got, want, what):
    (gi, gd), (wi, wd) = got, want
    assert gi.shape == wi.shape and gd.shape == wd.shape, what
    bad = (gi != wi) | (gd.view(np.uint32) != wd.view(np.uint32))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} columns differ, first at {np.argwhere(bad)[0]}"


def sample(n, k=64):
    return np.unique(np.concatenate([[0, n - 1], np.linspace(0, n - 1, k).astype(np.int64)]))


@pytest.mark.parametrize("n", [1, 2, 3, 100, 257])
def test_every_column_of_every_eye(nb, oracle, n):
    pos, vel = oracle.init_state(n, 1000 + n)
    with nb.Scene(pos, vel) as sc:
        for see_self in (False, True):
            got = sc.eyes(see_self=see_self)
            assert_same(got, expect(oracle, pos, vel, np.arange(n), see_self=see_self), f"N={n} see_self={see_self}")
    if n >= 100:
        assert (got[0] != R.NONE).mean() > 0.1      # the reference's init at N = 100 fills a good share of the columns


@pytest.mark.parametrize("n", [2048, 16384])
def test_sampled_eyes_of_large_sets(nb, oracle, n):
    pos, vel = oracle.init_state(n, 77)
    rows = sample(n)
    with nb.Scene(pos, vel) as sc:
        ids, depth = sc.eyes()
    assert ids.shape == (n, 1024)
    assert_same((ids[rows], depth[rows]), expect(oracle, pos, vel, rows), f"N={n}")


@pytest.mark.parametrize("controller", ["boids", "nbody"])
def test_after_steps(nb, oracle, controller):
    """a flock after 10 boids steps (wide spans) and a set after n-body steps; the state is the device's own (its bit-exactness
    against the oracle is tested elsewhere), the eyes are checked against the rule on it"""
    n = 2048
    pos, vel = oracle.init_state(n, 5)
    with nb.Scene(pos, vel) as sc:
        if controller == "boids":
            sc.step_boids_n(10)
        else:
            sc.step_n(3)
        p, v = sc.state()
        got = sc.eyes()
    rows = sample(n)
    assert_same((got[0][rows], got[1][rows]), expect(oracle, p, v, rows), controller)


@pytest.mark.parametrize("width", [1, 3, 1024, 4096])
def test_widths(nb, oracle, width):
    n = 257
    pos, vel = oracle.init_state(n, 31)
    with nb.Scene(pos, vel) as sc:
        got = sc.eyes(width=width)
    assert_same(got, expect(oracle, pos, vel, np.arange(n), width=width), f"W={width}")


def test_three_dimensional_data_with_a_narrow_vertical_field(nb, oracle):
    """3-D positions and velocities seen through a 30-degree vertical field of view: the y planes B3 / B4 clip real edges"""
    n = 300
    pos, vel = oracle.init_state(n, 9)
    rng = np.random.default_rng(9)
    pos[:, 2] = rng.uniform(-30, 30, n).astype(F)
    vel[:, 2] = rng.uniform(-0.05, 0.05, n).astype(F)
    cp = oracle.camera_constant(30.0, 1.0, 1.0, 10000.0)
    cams = oracle.cameras(pos, vel, UP, cp)
    P = R.clip_vertices(cams, R.world_vertices(oracle.instances(pos, vel)))
    y, z, w = P[..., 1], P[..., 2], P[..., 3]
    assert ((z >= 0) & ((w + y < 0) | (w - y < 0))).sum() > 1000     # vertices in front of the eye, outside the y planes
    with nb.Scene(pos, vel) as sc:
        got = sc.eyes(cp=cp)
    want = expect(oracle, pos, vel, np.arange(n), cp=cp)
    assert (want[0] != R.NONE).sum() > 1000
    assert_same(got, want, "3-D")


def test_subsets_self_and_a_zero_velocity_body(nb, oracle):
    n = 100
    pos, vel = oracle.init_state(n, 12)
    vel[7] = 0
    with nb.Scene(pos, vel) as sc:
        for first, count in ((5, 10), (0, 1), (99, 1), (40, 0), (0, 100)):
            for see_self in (False, True):
                got = sc.eyes(first=first, count=count, see_self=see_self)
                assert_same(got, expect(oracle, pos, vel, np.arange(first, first + count), see_self=see_self),
                            f"first={first} count={count} see_self={see_self}")
        ids, depth = sc.eyes(first=7, count=1)
    assert (ids == R.NONE).all() and (depth == 1).all()      # the zero-velocity eye: a NaN camera sees nothing


def launch(nb, n_total, first, count, cams, inst, width, flags, ids, depth, stream):
    from nenbody_amd import _lib

    lib = _lib.load()
    rc = lib.nb_launch_eyes(n_total, first, count, cams.data_ptr(), inst.data_ptr(), width, flags,
                            ids.data_ptr() if ids is not None else None, depth.data_ptr() if depth is not None else None,
                            stream.cuda_stream)
    _lib.check(rc)


def test_exact_lattice_through_the_launch_form(nb, oracle):
    """R.lattice_expectation through nb_launch_eyes with a caller camera, on torch device tensors and a stream of its own"""
    import torch

    from nenbody_amd import _lib

    dev = torch.device("cuda", 0)
    inst = torch.from_numpy(oracle.instances(R.LATTICE_POS, R.LATTICE_VEL).reshape(4, 16)).to(dev)
    cams = torch.from_numpy(np.repeat(R.lattice_camera().reshape(1, 16), 4, 0)).to(dev)
    ids = torch.full((4, 1024), 7, dtype=torch.int32, device=dev)
    depth = torch.full((4, 1024), 7.0, dtype=torch.float32, device=dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        launch(nb, 4, 0, 4, cams, inst, 1024, _lib.NB_EYES_SEE_SELF, ids, depth, s)
    s.synchronize()
    want_ids, want_depth = R.lattice_expectation()
    gi = ids.cpu().numpy().view(np.uint32)
    gd = depth.cpu().numpy()
    for e in range(4):
        assert (gi[e] == want_ids).all(), np.nonzero(gi[e] != want_ids)
        assert (gd[e].view(np.uint32) == want_depth.view(np.uint32)).all()


def test_the_launch_form_equals_scene_eyes(nb, oracle):
    import torch

    n = 257
    pos, vel = oracle.init_state(n, 3)
    cp = nb.eye_constant(1024)
    dev = torch.device("cuda", 0)
    with nb.Scene(pos, vel) as sc:
        cams_all = sc.cameras(UP, cp)
        inst = sc.instances()
        s = torch.cuda.Stream(dev)
        ct = torch.from_numpy(cams_all.reshape(n, 16)).to(dev)
        it = torch.from_numpy(inst.reshape(n, 16).copy()).to(dev)
        for first, count, see_self in ((0, n, False), (13, 50, True), (256, 1, False)):
            want = sc.eyes(first=first, count=count, see_self=see_self)
            ids = torch.empty((count, 1024), dtype=torch.int32, device=dev)
            depth = torch.empty((count, 1024), dtype=torch.float32, device=dev)
            flags = nb._lib.NB_EYES_SEE_SELF if see_self else 0
            with torch.cuda.stream(s):
                launch(nb, n, first, count, ct[first:first + count], it, 1024, flags, ids, depth, s)
                only_ids = torch.empty_like(ids)
                launch(nb, n, first, count, ct[first:first + count], it, 1024, flags, only_ids, None, s)
            s.synchronize()
            got = (ids.cpu().numpy().view(np.uint32), depth.cpu().numpy())
            assert_same(got, want, f"first={first} count={count}")
            assert (only_ids.cpu().numpy().view(np.uint32) == want[0]).all()


def test_two_calls_give_identical_bits(nb, oracle):
    n = 2048
    pos, vel = oracle.init_state(n, 21)
    with nb.Scene(pos, vel) as sc:
        a = sc.eyes()
        b = sc.eyes()
        c = sc.eyes(count=n // 2)      # the device rows shrink-reuse and grow back
        d = sc.eyes()
    for other in (b, d):
        assert (a[0] == other[0]).all() and (a[1].view(np.uint32) == other[1].view(np.uint32)).all()
    assert (c[0] == a[0][:n // 2]).all() and (c[1].view(np.uint32) == a[1][:n // 2].view(np.uint32)).all()
