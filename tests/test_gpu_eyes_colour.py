"""GPU tests of the eye view's colour row (nb_eyes_colour / nb_launch_eyes_colour): the HIP kernel
against the numpy restatement of the rule (tests/eyes_colour_restatement.py) -- rgba as uint32 views and bgra8, bit for bit -- with
cameras and model matrices by the oracle; ids and depth of the colour entry against nb_eyes' own.  The seeds' coverage (every edge
index winning, unequal end w, near-clipped winners) is checked on the CPU, tests/test_eyes_colour_cpu.py."""
import os

import numpy as np
import pytest

import eyes_colour_restatement as K
import eyes_restatement as R

pytestmark = pytest.mark.gpu

F = np.float32
UP = np.array([0, 0, 1], np.float32)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def reference_skin():
    """the reference's assets/skin.png, (20, 20, 4) uint8 sRGB"""
    return np.load(os.path.join(GOLDEN, "skin_rgba8.npy"))


def random_skin(tw, th, seed):
    """linear texels in [0, 1) but for one above 1 and one below 0: the bytes clamp, the floats do not"""
    skin = np.random.default_rng(seed).uniform(0, 1, (th, tw, 4)).astype(F)
    skin[0, 0, 0], skin[th - 1, tw - 1, 1] = 1.5, -0.25
    return skin


def expect(oracle, pos, vel, rows, width=1024, cp=None, up=UP, see_self=False, skin=None, stats=None):
    """the rule for the eyes of `rows` (ascending body indices) of the state (pos, vel)"""
    cp = R.eye_constant(oracle, width) if cp is None else cp
    cams = oracle.cameras(pos[rows], vel[rows], up, cp)
    inst = oracle.instances(pos, vel)
    rows = np.asarray(rows)
    out = (np.empty((len(rows), width), np.uint32), np.empty((len(rows), width), F), np.empty((len(rows), width, 4), F),
           np.empty((len(rows), width), np.uint32))
    i = 0
    while i < len(rows):   # runs of consecutive eyes in one call
        k = i + 1
        while k < len(rows) and rows[k] == rows[k - 1] + 1:
            k += 1
        for o, part in zip(out, K.colour(cams[i:k], inst, int(rows[i]), width, see_self, skin, stats=stats)):
            o[i:k] = part
        i = k
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    for name, g, w in zip(("ids", "depth", "rgba", "bgra8"), got, want):
        assert g.shape == w.shape, f"{what}: {name} {g.shape} != {w.shape}"
        bad = bits(g) != bits(w)
        assert not bad.any(), f"{what}: {name}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0]}"


def assert_ids_depth_are_nb_eyes(colour, plain, what):
    assert (colour[0] == plain[0]).all() and (bits(colour[1]) == bits(plain[1])).all(), what


def sample(n, k=64):
    return np.unique(np.concatenate([[0, n - 1], np.linspace(0, n - 1, k).astype(np.int64)]))


def skin_for(n):
    """(what Scene.set_skin takes, the linear texels it must become): white for the small sets, the reference's at N = 100, a
    random 7 x 5 at N = 257"""
    if n == 100:
        return reference_skin(), K.skin_from_srgb8(reference_skin())
    if n == 257:
        s = random_skin(7, 5, 11)
        return s, s
    return None, None


@pytest.mark.parametrize("n", [1, 2, 3, 100, 257])
def test_every_column_of_every_eye(nb, oracle, n):
    pos, vel = oracle.init_state(n, 1000 + n)
    given, lin = skin_for(n)
    stats = {}
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(given)
        for see_self in (False, True):
            got = sc.eyes_colour(see_self=see_self)
            assert_same(got, expect(oracle, pos, vel, np.arange(n), see_self=see_self, skin=lin, stats=stats), f"N={n} see_self={see_self}")
            assert_ids_depth_are_nb_eyes(got, sc.eyes(see_self=see_self), f"N={n} see_self={see_self}")
    if n >= 100:
        assert stats["covered"] > 0.1 * stats["columns"]      # the reference's init fills a good share of the columns
        assert (stats["edge"] > 100).all() and stats["unequal_w"] > 1000 and stats["s0>0"] > 0, stats


@pytest.mark.parametrize("n", [2048, 16384])
def test_sampled_eyes_of_large_sets(nb, oracle, n):
    pos, vel = oracle.init_state(n, 77)
    rows = sample(n)
    skin = K.skin_from_srgb8(reference_skin())
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(skin)
        got = sc.eyes_colour()
        plain = sc.eyes()
    assert got[2].shape == (n, 1024, 4) and got[3].shape == (n, 1024)
    assert_ids_depth_are_nb_eyes(got, plain, f"N={n}")
    assert_same(tuple(g[rows] for g in got), expect(oracle, pos, vel, rows, skin=skin), f"N={n}")


@pytest.mark.parametrize("controller", ["boids", "nbody"])
def test_after_steps(nb, oracle, controller):
    """a flock after 10 boids steps (wide spans) and a set after 3 n-body steps; the state is the device's own, the colour rows are
    checked against the rule on it"""
    n = 2048
    pos, vel = oracle.init_state(n, 5)
    skin = random_skin(3, 9, 2)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(skin)
        if controller == "boids":
            sc.step_boids_n(10)
        else:
            sc.step_n(3)
        p, v = sc.state()
        got = sc.eyes_colour()
    rows = sample(n)
    assert_same(tuple(g[rows] for g in got), expect(oracle, p, v, rows, skin=skin), controller)


@pytest.mark.parametrize("width", [1, 3, 1024, 4096])
def test_widths(nb, oracle, width):
    n = 257
    pos, vel = oracle.init_state(n, 31)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(reference_skin())
        got = sc.eyes_colour(width=width)
        plain = sc.eyes(width=width)
    assert_ids_depth_are_nb_eyes(got, plain, f"W={width}")
    assert_same(got, expect(oracle, pos, vel, np.arange(n), width=width, skin=K.skin_from_srgb8(reference_skin())), f"W={width}")


def test_three_dimensional_data_with_a_narrow_vertical_field(nb, oracle):
    """3-D positions and velocities seen through a 30-degree vertical field of view: the y planes B3 / B4 clip real edges, whose
    texture coordinate then starts inside the edge"""
    n = 300
    pos, vel = oracle.init_state(n, 9)
    rng = np.random.default_rng(9)
    pos[:, 2] = rng.uniform(-30, 30, n).astype(F)
    vel[:, 2] = rng.uniform(-0.05, 0.05, n).astype(F)
    cp = oracle.camera_constant(30.0, 1.0, 1.0, 10000.0)
    skin = random_skin(16, 4, 3)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(skin)
        got = sc.eyes_colour(cp=cp)
    stats = {}
    want = expect(oracle, pos, vel, np.arange(n), cp=cp, skin=skin, stats=stats)
    assert stats["covered"] > 1000 and stats["s0>0"] > 0
    assert_same(got, want, "3-D")


def test_subsets_self_and_a_zero_velocity_body(nb, oracle):
    n = 100
    pos, vel = oracle.init_state(n, 12)
    vel[7] = 0
    with nb.Scene(pos, vel) as sc:
        for first, count in ((5, 10), (0, 1), (99, 1), (40, 0), (0, 100)):
            for see_self in (False, True):
                got = sc.eyes_colour(first=first, count=count, see_self=see_self)
                assert_same(got, expect(oracle, pos, vel, np.arange(first, first + count), see_self=see_self),
                            f"first={first} count={count} see_self={see_self}")
        ids, depth, rgba, bgra8 = sc.eyes_colour(first=7, count=1)
    # the zero-velocity eye: a NaN camera sees nothing, every column is the clear colour
    assert (ids == R.NONE).all() and (depth == 1).all()
    assert (bits(rgba) == bits(np.tile(K.CLEAR, (1, 1024, 1)))).all() and (bgra8 == 0xFF597C95).all()


def launch(nb, n_total, first, count, cams, inst, width, flags, skin, ids, depth, rgba, bgra8, stream):
    from nenbody_amd import _lib

    def ptr(t):
        return t.data_ptr() if t is not None else None

    tw, th = (skin.shape[1], skin.shape[0]) if skin is not None else (0, 0)
    _lib.check(_lib.load().nb_launch_eyes_colour(n_total, first, count, cams.data_ptr(), inst.data_ptr(), width, flags, ptr(skin), tw, th,
                                                 ptr(ids), ptr(depth), ptr(rgba), ptr(bgra8), stream.cuda_stream))


def test_exact_lattice_through_the_launch_form(nb, oracle):
    """the lattice's hand-derived colours through nb_launch_eyes_colour with a caller camera, on torch device tensors and a stream
    of its own: 0.5 / 0.75 on the visible bodies' two columns, the clear colour elsewhere; a 7 x 5 skin pins ix / iy on the device"""
    import torch

    from nenbody_amd import _lib

    dev = torch.device("cuda", 0)
    inst_h = oracle.instances(R.LATTICE_POS, R.LATTICE_VEL)
    cams_h = np.repeat(R.lattice_camera()[None], 4, 0)
    inst = torch.from_numpy(inst_h.reshape(4, 16)).to(dev)
    cams = torch.from_numpy(cams_h.reshape(4, 16)).to(dev)
    skin_h = (np.arange(5 * 7 * 4, dtype=np.float32).reshape(5, 7, 4) + F(1)) / F(256)
    s = torch.cuda.Stream(dev)
    for skin in (None, skin_h):
        ids = torch.full((4, 1024), 7, dtype=torch.int32, device=dev)
        depth = torch.full((4, 1024), 7.0, dtype=torch.float32, device=dev)
        rgba = torch.full((4, 1024, 4), 7.0, dtype=torch.float32, device=dev)
        bgra8 = torch.full((4, 1024), 7, dtype=torch.int32, device=dev)
        st = torch.from_numpy(skin).to(dev) if skin is not None else None
        with torch.cuda.stream(s):
            launch(nb, 4, 0, 4, cams, inst, 1024, _lib.NB_EYES_SEE_SELF, st, ids, depth, rgba, bgra8, s)
        s.synchronize()
        got = (ids.cpu().numpy().view(np.uint32), depth.cpu().numpy(), rgba.cpu().numpy(), bgra8.cpu().numpy().view(np.uint32))
        assert_same(got, K.colour(cams_h, inst_h, 0, 1024, True, skin), "lattice")
        if skin is None:
            want = np.tile(K.CLEAR, (1024, 1))
            want[[511, 514, 518]] = F([0.5, 0.5, 0.5, 1])
            want[[512, 515, 519]] = F([0.75, 0.75, 0.75, 1])
            for e in range(4):
                assert (bits(got[2][e]) == bits(want)).all()
        else:
            assert (bits(got[2][0, 512, :3]) == bits(skin_h[2, 0, :3] * F(0.75))).all()


def test_the_launch_form_equals_scene_eyes_colour_with_each_output_alone(nb, oracle):
    import torch

    n = 257
    pos, vel = oracle.init_state(n, 3)
    cp = nb.eye_constant(1024)
    dev = torch.device("cuda", 0)
    skin = random_skin(5, 12, 8)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(skin)
        cams_all = sc.cameras(UP, cp)
        inst = sc.instances()
        s = torch.cuda.Stream(dev)
        ct = torch.from_numpy(cams_all.reshape(n, 16)).to(dev)
        it = torch.from_numpy(inst.reshape(n, 16).copy()).to(dev)
        st = torch.from_numpy(skin).to(dev)
        for first, count, see_self in ((0, n, False), (13, 50, True), (256, 1, False)):
            want = sc.eyes_colour(first=first, count=count, see_self=see_self)
            flags = nb._lib.NB_EYES_SEE_SELF if see_self else 0

            def fresh():
                return [torch.empty((count, 1024), dtype=torch.int32, device=dev), torch.empty((count, 1024), dtype=torch.float32, device=dev),
                        torch.empty((count, 1024, 4), dtype=torch.float32, device=dev), torch.empty((count, 1024), dtype=torch.int32, device=dev)]

            every = fresh()
            alone = [fresh()[k] for k in range(4)]
            with torch.cuda.stream(s):
                launch(nb, n, first, count, ct[first:first + count], it, 1024, flags, st, *every, s)
                launch(nb, n, first, count, ct[first:first + count], it, 1024, flags, st, None, None, alone[2], None, s)
                launch(nb, n, first, count, ct[first:first + count], it, 1024, flags, st, None, None, None, alone[3], s)
                # ids / depth alone need a colour output beside them (without one the call is nb_launch_eyes)
                launch(nb, n, first, count, ct[first:first + count], it, 1024, flags, st, alone[0], None, None, fresh()[3], s)
                launch(nb, n, first, count, ct[first:first + count], it, 1024, flags, st, None, alone[1], fresh()[2], None, s)
            s.synchronize()
            for k in range(4):
                assert (bits(every[k].cpu().numpy()) == bits(want[k])).all(), (first, count, k)
                assert (bits(alone[k].cpu().numpy()) == bits(want[k])).all(), (first, count, k, "alone")


def test_two_calls_give_identical_bits(nb, oracle):
    n = 2048
    pos, vel = oracle.init_state(n, 21)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(reference_skin())
        a = sc.eyes_colour()
        b = sc.eyes_colour()
        c = sc.eyes_colour(count=n // 2)      # the device rows shrink-reuse and grow back
        d = sc.eyes_colour()
    for other in (b, d):
        for x, y in zip(a, other):
            assert (bits(x) == bits(y)).all()
    for x, y in zip(a, c):
        assert (bits(x[:n // 2]) == bits(y)).all()


def test_skins_white_reference_random_and_back(nb, oracle):
    """one scene, the skin changed between calls: white (never set), the reference's as uint8 sRGB, a random 13 x 2 as floats, and
    None again -- each call samples the skin in place at the time"""
    n = 100
    pos, vel = oracle.init_state(n, 1100)
    rows = np.arange(n)
    ref = reference_skin()
    rnd = random_skin(13, 2, 4)
    with nb.Scene(pos, vel) as sc:
        got_white = sc.eyes_colour()
        sc.set_skin(ref)
        got_ref = sc.eyes_colour()
        sc.set_skin(rnd)
        got_rnd = sc.eyes_colour()
        sc.set_skin(None)
        got_none = sc.eyes_colour()
    assert_same(got_white, expect(oracle, pos, vel, rows), "white")
    assert_same(got_ref, expect(oracle, pos, vel, rows, skin=K.skin_from_srgb8(ref)), "reference")
    assert_same(got_rnd, expect(oracle, pos, vel, rows, skin=rnd), "random")
    assert_same(got_none, got_white, "white again")
    assert (bits(got_ref[2]) != bits(got_white[2])).any() and (got_rnd[3] != got_white[3]).any()


def test_bgra8_is_the_srgb_encoding_of_the_same_calls_rgba(nb, oracle):
    n = 257
    pos, vel = oracle.init_state(n, 14)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(random_skin(9, 6, 6))       # texels above 1 and below 0 among them: the bytes clamp
        _, _, rgba, bgra8 = sc.eyes_colour()
    by = nb.srgb_encode(rgba)                    # (n, W, 4) bytes R, G, B, A
    want = by[..., 2].astype(np.uint32) | by[..., 1].astype(np.uint32) << 8 | by[..., 0].astype(np.uint32) << 16 | by[..., 3].astype(np.uint32) << 24
    assert (by[..., 3] == 255).all() and (bgra8 == want).all()
    px = bgra8.view(np.uint8).reshape(n, 1024, 4)
    assert (px[..., 0] == by[..., 2]).all() and (px[..., 2] == by[..., 0]).all()      # in memory B, G, R, A
    assert len(np.unique(bgra8)) > 100


def test_viewport_is_the_eyes_row_repeated(nb, oracle):
    n = 100
    pos, vel = oracle.init_state(n, 1100)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(reference_skin())
        cam = int(np.argmax((sc.eyes()[0] != R.NONE).sum(1)))      # an eye that sees something
        row = sc.eyes_colour(first=cam, count=1)[3][0]
        full = sc.viewport(cam, scale=1.0, extent=(1024, 4))
        tenth = sc.viewport(cam, scale=0.1, extent=(1280, 720))
    assert len(np.unique(row)) > 3
    assert full.shape == (4, 1024) and (full == row[None, :]).all()
    assert tenth.shape == (72, 128) and (tenth == row[(2 * np.arange(128) + 1) * 1024 // 256][None, :]).all()
