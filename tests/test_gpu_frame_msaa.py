"""GPU tests of the frame through 8 samples per pixel (nb_frame_msaa / nb_launch_frame_msaa): the HIP
kernels against the numpy restatement of the rule (tests/frame_msaa_restatement.py) -- ids8, depth8, rgba and bgra8 as uint32 words,
bit for bit -- with cameras and model matrices by the oracle.  What the scenes cover (every partial sample count, pixels naming two
bodies, every edge index winning, pixels whose centre is empty) is asserted on the CPU, tests/test_frame_msaa_cpu.py."""
import os

import numpy as np
import pytest

import eyes_colour_restatement as K
import eyes_restatement as R
import frame_msaa_restatement as FM
import frame_restatement as FR

pytestmark = pytest.mark.gpu

F = np.float32
UP = np.array([0, 0, 1], np.float32)
CLEAR_BGRA8 = 0xFF597C95
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def reference_skin():
    """the reference's assets/skin.png, (20, 20, 4) uint8 sRGB"""
    return np.load(os.path.join(GOLDEN, "skin_rgba8.npy"))


def random_skin(tw, th, seed):
    """linear texels in [0, 1) but for one above 1 and one below 0: the bytes clamp, the floats do not"""
    skin = np.random.default_rng(seed).uniform(0, 1, (th, tw, 4)).astype(F)
    skin[0, 0, 0], skin[th - 1, tw - 1, 1] = 1.5, -0.25
    return skin


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    for name, g, w in zip(("ids8", "depth8", "rgba", "bgra8"), got, want):
        assert g.shape == w.shape, f"{what}: {name} {g.shape} != {w.shape}"
        bad = bits(g) != bits(w)
        assert not bad.any(), f"{what}: {name}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0]}"


def assert_clear(got, W, H):
    ids8, depth8, rgba, bgra8 = got
    assert ids8.shape == (H, W, 8) and (ids8 == R.NONE).all() and depth8.shape == (H, W, 8) and (depth8 == 1).all()
    assert bgra8.shape == (H, W) and (bgra8 == CLEAR_BGRA8).all() and (bits(rgba) == bits(np.tile(K.CLEAR, (H, W, 1)))).all()


# -- 1. the scenes of the table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["side", "inside", "top", "three"])
def test_the_scenes(nb, oracle, name):
    pos, vel, cam, (W, H) = FR.scene(oracle, name)
    skin = random_skin(7, 5, 11) if name == "side" else None
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(skin)
        got = sc.frame_msaa(cam, (W, H))
    stats = {}
    want = FM.frame_msaa(cam, oracle.instances(pos, vel), W, H, skin=skin, stats=stats)
    assert stats["writes"] > 3000 and (stats["covered_hist"][1:] > 0).all() and stats["two_bodies"] > 0
    assert_same(got, want, name)


def test_the_reference_state_through_its_own_camera(nb, oracle):
    """init_state(100, 1100) at a quarter of the reference's extent, the camera 250 above body 0, the reference skin:
    Scene.scene_camera forms the camera, which must be the oracle's bit for bit"""
    extent = (480, 270)
    pos, vel = oracle.init_state(100, 1100)
    cam = FR.scene_camera(oracle, pos, extent, height=250.0)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(reference_skin())
        assert (bits(sc.scene_camera(extent, height=250.0)) == bits(cam)).all()
        got = sc.frame_msaa(cam, extent)
    stats = {}
    want = FM.frame_msaa(cam, oracle.instances(pos, vel), *extent, skin=K.skin_from_srgb8(reference_skin()), stats=stats)
    assert stats["writes"] > 1000 and len(np.unique(want[0])) > 50
    assert_same(got, want, "reference state")


# -- 2. small and awkward counts and extents --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 257])
def test_small_counts(nb, oracle, n):
    pos, vel = oracle.init_state(n, 1000 + n)
    cam = FR.scene_camera(oracle, pos, (96, 64), height=8.0 if n <= 3 else 60.0)   # (a few bodies: close, so their edges are long)
    with nb.Scene(pos, vel) as sc:
        got = sc.frame_msaa(cam, (96, 64))
    stats = {}
    assert_same(got, FM.frame_msaa(cam, oracle.instances(pos, vel), 96, 64, stats=stats), f"N={n}")
    assert stats["writes"] > 160


@pytest.mark.parametrize("extent", [(1, 1), (3, 2), (1024, 1)])
def test_small_extents(nb, oracle, extent):
    n = 257
    pos, vel = FR.spread_state(oracle, n, 31, 30)
    cam = FR.camera(oracle, [0, 0, 150], [0, 0, -1], [1, 0, 0], FR.frame_constant(oracle, extent))
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(reference_skin())
        got = sc.frame_msaa(cam, extent)
    stats = {}
    want = FM.frame_msaa(cam, oracle.instances(pos, vel), extent[0], extent[1], skin=K.skin_from_srgb8(reference_skin()), stats=stats)
    assert stats["writes"] > 0
    assert_same(got, want, f"{extent}")


@pytest.mark.parametrize("wide", [True, False])
def test_the_largest_dimension(nb, oracle, wide):
    """an orthographic caller camera that magnifies the long axis 512 times: a body whose edges run 1024 pixels along it, up to the
    last column (2048 x 2: the body at (1, 0) heading +x, xs = 1024 + 512 x) or the last row (2 x 2048: the body at (0, -1) heading
    +y, ys = 1024 - 512 y)"""
    from nenbody_amd import _lib

    top = _lib.NB_FRAME_MSAA_MAX_DIM
    W, H = (top, 2) if wide else (2, top)
    pos = np.array([[1, 0, 0] if wide else [0, -1, 0]], F)
    vel = np.array([[1, 0, 0] if wide else [0, 1, 0]], F)
    cam = FR.ortho_camera(W, H, 512 if wide else 1, 1 if wide else 512)
    with nb.Scene(pos, vel) as sc:
        got = sc.frame_msaa(cam, (W, H))
    stats = {}
    want = FM.frame_msaa(cam, oracle.instances(pos, vel), W, H, stats=stats)
    assert_same(got, want, f"{(W, H)}")
    edge8 = stats["edge8"]
    steps = max(len(np.unique(np.argwhere(edge8 == e)[:, 1 if wide else 0])) for e in range(3))
    assert steps > 1000, steps                                   # an edge runs past 1 000 major-axis steps
    last = got[0][:, W - 1] if wide else got[0][H - 1, :]
    assert (last == 0).any()


# -- 3. one row is the eye's 8-sample row ---------------------------------------------------------------------------------------------------
def test_one_row_equals_eyes_msaa_on_the_device(nb, oracle):
    pos, vel = oracle.init_state(100, 1100)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(reference_skin())
        cams = sc.cameras(UP, nb.eye_constant(1024))
        covered = 0
        for e in (0, 1, 17, 50, 99):
            got = sc.frame_msaa(cams[e], (1024, 1))
            assert_same(got, sc.eyes_msaa(first=e, count=1, see_self=True), f"eye {e}")
            covered += int((got[0] != R.NONE).sum())
    assert covered > 4000


# -- 4. after steps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("controller", ["boids", "nbody"])
def test_after_steps(nb, oracle, controller):
    """the frame of the device's own state after 10 boids steps or 3 n-body steps against the rule on the downloaded state"""
    n, extent = 2048, (320, 180)
    pos, vel = oracle.init_state(n, 5)
    skin = random_skin(3, 9, 2)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(skin)
        if controller == "boids":
            sc.step_boids_n(10)
        else:
            sc.step_n(3)
        p, v = sc.state()
        cam = sc.scene_camera(extent, height=200.0)
        got = sc.frame_msaa(cam, extent)
    want_cam = FR.scene_camera(oracle, p, extent, height=200.0)
    assert (bits(cam) == bits(want_cam)).all()
    stats = {}
    want = FM.frame_msaa(want_cam, oracle.instances(p, v), extent[0], extent[1], skin=skin, stats=stats)
    assert stats["writes"] > 8000
    assert_same(got, want, controller)


# -- 5. a NaN camera --------------------------------------------------------------------------------------------------------------------------
def test_a_nan_camera_gives_the_clear_frame(nb, oracle):
    pos, vel = oracle.init_state(64, 12)
    with nb.Scene(pos, vel) as sc:
        cam = sc.camera_at((0, 0, 100), (0, 0, 0), (1, 0, 0), nb.frame_constant((96, 64)))
        assert np.isnan(cam).any()
        assert_clear(sc.frame_msaa(cam, (96, 64)), 96, 64)
        assert_clear(sc.frame_msaa(np.full((4, 4), np.nan, F), (33, 7)), 33, 7)


# -- 6. the launch form ----------------------------------------------------------------------------------------------------------------------
def test_the_launch_form_on_torch_tensors_and_a_stream_of_its_own(nb, oracle):
    """nb_launch_frame_msaa on caller-owned device memory: all four outputs together, then each alone, prefilled with 7, equal to
    Scene.frame_msaa; N = 0 gives the clear frame"""
    import torch

    from nenbody_amd import _lib

    lib = _lib.load()
    pos, vel, cam, (W, H) = FR.scene(oracle, "side")
    skin = random_skin(7, 5, 11)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(skin)
        want = sc.frame_msaa(cam, (W, H))
        inst_h = sc.instances().copy()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    ct = torch.from_numpy(np.ascontiguousarray(cam).reshape(16)).to(dev)
    it = torch.from_numpy(inst_h.reshape(len(pos), 16)).to(dev)
    st = torch.from_numpy(skin).to(dev)
    assert lib.nb_frame_msaa_scratch_bytes(W, H) == W * H * 64
    scratch = torch.empty(lib.nb_frame_msaa_scratch_bytes(W, H) // 8, dtype=torch.int64, device=dev)

    def outs():
        return [torch.full((H, W, 8), 7, dtype=torch.int32, device=dev), torch.full((H, W, 8), 7.0, dtype=torch.float32, device=dev),
                torch.full((H, W, 4), 7.0, dtype=torch.float32, device=dev), torch.full((H, W), 7, dtype=torch.int32, device=dev)]

    def run(n, o):
        with torch.cuda.stream(s):
            _lib.check(lib.nb_launch_frame_msaa(n, ct.data_ptr(), it.data_ptr() if n else None, W, H, 0, st.data_ptr(), 7, 5,
                                                scratch.data_ptr(), *[t.data_ptr() if t is not None else None for t in o], s.cuda_stream))
        s.synchronize()

    torch.cuda.synchronize()
    o = outs()
    run(len(pos), o)
    assert_same(tuple(t.cpu().numpy() for t in o), want, "all four")
    for k in range(4):
        o = outs()
        run(len(pos), [t if i == k else None for i, t in enumerate(o)])
        for i, t in enumerate(o):
            if i == k:
                assert (bits(t.cpu().numpy()) == bits(want[i])).all(), f"output {i} alone"
            else:
                assert (t.cpu().numpy() == 7).all(), f"output {i} was written though NULL"
    o = outs()
    run(0, o)
    ids8, depth8, rgba, bgra8 = (t.cpu().numpy() for t in o)
    assert_clear((ids8.view(np.uint32), depth8, rgba, bgra8.view(np.uint32)), W, H)


# -- 7. run to run ---------------------------------------------------------------------------------------------------------------------------
def test_two_calls_regrown_rows_and_a_changed_skin(nb, oracle):
    pos, vel = FR.spread_state(oracle, 300, 9, 30)
    inst = oracle.instances(pos, vel)
    small, large = (96, 64), (640, 360)
    cams = {e: FR.camera(oracle, [-150, 0, 40], [1, 0, -0.25], [0, 0, 1], FR.frame_constant(oracle, e)) for e in (small, large)}
    skin = random_skin(7, 5, 11)
    with nb.Scene(pos, vel) as sc:
        first = sc.frame_msaa(cams[small], small)
        assert_same(sc.frame_msaa(cams[small], small), first, "the second call")
        big = sc.frame_msaa(cams[large], large)
        assert_same(sc.frame_msaa(cams[small], small), first, "small after large")
        one = sc.frame(cams[small], small)                       # the one-sample frame shares the rows and the key plane
        assert_same(sc.frame_msaa(cams[small], small), first, "after nb_frame")
        sc.set_skin(skin)
        coloured = sc.frame_msaa(cams[small], small)
        sc.set_skin(None)
        assert_same(sc.frame_msaa(cams[small], small), first, "white again")
    assert_same(first, FM.frame_msaa(cams[small], inst, *small), "small")
    assert_same(big, FM.frame_msaa(cams[large], inst, *large), "large")
    assert_same(coloured, FM.frame_msaa(cams[small], inst, *small, skin=skin), "skin")
    assert (bits(coloured[2]) != bits(first[2])).any()
    for g, w in zip(one, FR.frame(cams[small], inst, *small)):
        assert (bits(g) == bits(w)).all()


# -- 8. the bytes are the encoder's -----------------------------------------------------------------------------------------------------------
def test_bgra8_is_srgb_encode_of_the_same_calls_rgba(nb, oracle):
    pos, vel, cam, (W, H) = FR.scene(oracle, "side")
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(random_skin(7, 5, 11))
        _, _, rgba, bgra8 = sc.frame_msaa(cam, (W, H))
    by = nb.srgb_encode(rgba).astype(np.uint32)
    assert (bgra8 == (by[..., 2] | by[..., 1] << 8 | by[..., 0] << 16 | 0xFF000000)).all()
