"""GPU tests of the eye rows through 8 samples per column (nb_eyes_msaa / nb_launch_eyes_msaa):
the HIP kernel against the numpy restatement of the rule (tests/eyes_msaa_restatement.py) -- every word of ids8, depth8, rgba (as
uint32 views) and bgra8, bit for bit -- with cameras and model matrices by the oracle.  What the seeds cover (partly covered
columns, columns shared by two bodies, extrapolated fragments, every edge winning) is checked on the CPU,
tests/test_eyes_msaa_cpu.py."""
import os

import numpy as np
import pytest

import eyes_colour_restatement as K
import eyes_msaa_restatement as M
import eyes_restatement as R

pytestmark = pytest.mark.gpu

F = np.float32
UP = np.array([0, 0, 1], np.float32)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("ids8", "depth8", "rgba", "bgra8")


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
    out = (np.empty((len(rows), width, 8), np.uint32), np.empty((len(rows), width, 8), F), np.empty((len(rows), width, 4), F),
           np.empty((len(rows), width), np.uint32))
    i = 0
    while i < len(rows):   # runs of consecutive eyes in one call
        k = i + 1
        while k < len(rows) and rows[k] == rows[k - 1] + 1:
            k += 1
        for o, part in zip(out, M.msaa(cams[i:k], inst, int(rows[i]), width, see_self, skin, stats=stats)):
            o[i:k] = part
        i = k
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, f"{what}: {name} {g.shape} != {w.shape}"
        bad = bits(g) != bits(w)
        assert not bad.any(), f"{what}: {name}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0]}"


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
def test_every_sample_of_every_eye(nb, oracle, n):
    pos, vel = oracle.init_state(n, 1000 + n)
    given, lin = skin_for(n)
    stats = {}
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(given)
        for see_self in (False, True):
            got = sc.eyes_msaa(see_self=see_self)
            assert_same(got, expect(oracle, pos, vel, np.arange(n), see_self=see_self, skin=lin, stats=stats), f"N={n} see_self={see_self}")
    if n >= 100:   # the cases are not empty ones (the figures: tests/test_eyes_msaa_cpu.py)
        assert (stats["covered_hist"][1:8] >= 100).all() and stats["two_bodies_full"] >= 300 and stats["extrapolated"] >= 2000, stats


@pytest.mark.parametrize("width", [1, 3, 1024, 2048])
def test_widths(nb, oracle, width):
    """2048 is the widest row (129 KiB of LDS: more than a kernel may take without asking); 1 and 3 have samples either side of
    every span end"""
    n = 257
    pos, vel = oracle.init_state(n, 31)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(reference_skin())
        got = sc.eyes_msaa(width=width)
    assert_same(got, expect(oracle, pos, vel, np.arange(n), width=width, skin=K.skin_from_srgb8(reference_skin())), f"W={width}")


def test_sampled_eyes_of_a_large_set(nb, oracle):
    n = 2048
    pos, vel = oracle.init_state(n, 77)
    rows = sample(n)
    skin = K.skin_from_srgb8(reference_skin())
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(skin)
        got = sc.eyes_msaa()
    assert got[0].shape == (n, 1024, 8) and got[1].shape == (n, 1024, 8) and got[2].shape == (n, 1024, 4) and got[3].shape == (n, 1024)
    assert_same(tuple(g[rows] for g in got), expect(oracle, pos, vel, rows, skin=skin), f"N={n}")


@pytest.mark.parametrize("controller", ["boids", "nbody"])
def test_after_steps(nb, oracle, controller):
    """a flock after 10 boids steps (wide spans) and a set after 3 n-body steps; the state is the device's own, the rows are
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
        got = sc.eyes_msaa()
    rows = sample(n, 32)
    assert_same(tuple(g[rows] for g in got), expect(oracle, p, v, rows, skin=skin), controller)


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
        got = sc.eyes_msaa(cp=cp)
    stats = {}
    want = expect(oracle, pos, vel, np.arange(n), cp=cp, skin=skin, stats=stats)
    assert stats["covered_hist"][1:].sum() > 1000
    assert_same(got, want, "3-D")


def test_subsets_self_and_a_zero_velocity_body(nb, oracle):
    n = 100
    pos, vel = oracle.init_state(n, 12)
    vel[7] = 0
    with nb.Scene(pos, vel) as sc:
        for first, count in ((5, 10), (0, 1), (99, 1), (40, 0), (0, 100)):
            for see_self in (False, True):
                got = sc.eyes_msaa(first=first, count=count, see_self=see_self)
                assert_same(got, expect(oracle, pos, vel, np.arange(first, first + count), see_self=see_self),
                            f"first={first} count={count} see_self={see_self}")
        ids8, depth8, rgba, bgra8 = sc.eyes_msaa(first=7, count=1)
    # the zero-velocity eye: a NaN camera sees nothing, every sample is empty and every column the clear colour
    assert (ids8 == R.NONE).all() and (depth8 == 1).all()
    assert (bits(rgba) == bits(np.tile(K.CLEAR, (1, 1024, 1)))).all() and (bgra8 == 0xFF597C95).all()


def launch(nb, n_total, first, count, cams, inst, width, flags, skin, ids8, depth8, rgba, bgra8, stream):
    from nenbody_amd import _lib

    def ptr(t):
        return t.data_ptr() if t is not None else None

    tw, th = (skin.shape[1], skin.shape[0]) if skin is not None else (0, 0)
    _lib.check(_lib.load().nb_launch_eyes_msaa(n_total, first, count, cams.data_ptr(), inst.data_ptr(), width, flags, ptr(skin), tw, th,
                                               ptr(ids8), ptr(depth8), ptr(rgba), ptr(bgra8), stream.cuda_stream))


def fresh(torch, dev, count, width=1024):
    return [torch.full((count, width, 8), 7, dtype=torch.int32, device=dev), torch.full((count, width, 8), 7.0, dtype=torch.float32, device=dev),
            torch.full((count, width, 4), 7.0, dtype=torch.float32, device=dev), torch.full((count, width), 7, dtype=torch.int32, device=dev)]


def test_exact_lattice_through_the_launch_form(nb, oracle):
    """the lattice's hand-derived rows (tests/test_eyes_msaa_cpu.py) through nb_launch_eyes_msaa with a caller camera, on torch
    device tensors and a stream of its own: the half columns 511 / 513, the full column 512, likewise for bodies 2 and 3"""
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
        out = fresh(torch, dev, 4)
        st = torch.from_numpy(skin).to(dev) if skin is not None else None
        with torch.cuda.stream(s):
            launch(nb, 4, 0, 4, cams, inst, 1024, _lib.NB_EYES_SEE_SELF, st, *out, s)
        s.synchronize()
        got = (out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy().view(np.uint32))
        assert_same(got, M.msaa(cams_h, inst_h, 0, 1024, True, skin), "lattice")
        if skin is None:
            half = np.array([0x3E99999A, 0x3EB33333, 0x3ECCCCCD, 0x3F800000], np.uint32)
            for e in range(4):
                for c0, body in ((511, 0), (514, 2), (518, 3)):
                    assert (got[0][e, c0, [0, 2, 6, 7]] == body).all() and (got[0][e, c0, [1, 3, 4, 5]] == R.NONE).all()
                    assert (got[0][e, c0 + 1] == body).all() and (got[1][e, c0 + 1] == 0.5).all()
                    assert (got[0][e, c0 + 2, [1, 3, 4, 5]] == body).all() and (got[0][e, c0 + 2, [0, 2, 6, 7]] == R.NONE).all()
                    assert (bits(got[2][e, c0]) == half).all() and (bits(got[2][e, c0 + 2]) == half).all()
                    assert (got[2][e, c0 + 1] == F([0.75, 0.75, 0.75, 1])).all()
                    assert got[3][e, c0] == 0xFF95A0AA and got[3][e, c0 + 1] == 0xFFE1E1E1 and got[3][e, c0 + 2] == 0xFF95A0AA


def test_the_launch_form_equals_scene_eyes_msaa_with_each_output_alone(nb, oracle):
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
            want = sc.eyes_msaa(first=first, count=count, see_self=see_self)
            flags = nb._lib.NB_EYES_SEE_SELF if see_self else 0
            every = fresh(torch, dev, count)
            alone = [fresh(torch, dev, count)[k] for k in range(4)]
            with torch.cuda.stream(s):
                launch(nb, n, first, count, ct[first:first + count], it, 1024, flags, st, *every, s)
                for k in range(4):
                    args = [None] * 4
                    args[k] = alone[k]
                    launch(nb, n, first, count, ct[first:first + count], it, 1024, flags, st, *args, s)
            s.synchronize()
            for k in range(4):
                assert (bits(every[k].cpu().numpy()) == bits(want[k])).all(), (first, count, NAMES[k])
                assert (bits(alone[k].cpu().numpy()) == bits(want[k])).all(), (first, count, NAMES[k], "alone")


def test_two_calls_give_identical_bits(nb, oracle):
    n = 2048
    pos, vel = oracle.init_state(n, 21)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(reference_skin())
        a = sc.eyes_msaa()
        b = sc.eyes_msaa()
        c = sc.eyes_msaa(count=n // 2)      # the device rows shrink-reuse and grow back
        d = sc.eyes_msaa()
    for other in (b, d):
        for x, y in zip(a, other):
            assert (bits(x) == bits(y)).all()
    for x, y in zip(a, c):
        assert (bits(x[:n // 2]) == bits(y)).all()


def test_bgra8_is_the_srgb_encoding_of_the_same_calls_rgba(nb, oracle):
    n = 257
    pos, vel = oracle.init_state(n, 14)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(random_skin(9, 6, 6))       # texels above 1 and below 0 among them: the bytes clamp
        _, _, rgba, bgra8 = sc.eyes_msaa()
    assert (rgba[..., 3] == 1).all()
    by = nb.srgb_encode(rgba)                    # (n, W, 4) bytes R, G, B, A
    want = by[..., 2].astype(np.uint32) | by[..., 1].astype(np.uint32) << 8 | by[..., 0].astype(np.uint32) << 16 | by[..., 3].astype(np.uint32) << 24
    assert (by[..., 3] == 255).all() and (bgra8 == want).all()
    assert len(np.unique(bgra8)) > 100


def test_viewport_msaa_is_the_resolved_row_repeated(nb, oracle):
    n = 100
    pos, vel = oracle.init_state(n, 1100)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(reference_skin())
        cam = int(np.argmax((sc.eyes()[0] != R.NONE).sum(1)))      # an eye that sees something
        row = sc.eyes_msaa(first=cam, count=1)[3][0]
        plain = sc.eyes_colour(first=cam, count=1)[3][0]
        full = sc.viewport(cam, scale=1.0, extent=(1024, 4), msaa=True)
        tenth = sc.viewport(cam, scale=0.1, extent=(1280, 720), msaa=True)
        default = sc.viewport(cam, scale=1.0, extent=(1024, 4))
    assert len(np.unique(row)) > 3 and (row != plain).any()
    assert full.shape == (4, 1024) and (full == row[None, :]).all()
    assert tenth.shape == (72, 128) and (tenth == row[(2 * np.arange(128) + 1) * 1024 // 256][None, :]).all()
    assert (default == plain[None, :]).all()                       # the default is the one-sample row, as before


def test_the_one_sample_entries_give_the_bits_they_gave_before(nb, oracle):
    """Scene.eyes and Scene.eyes_colour before and after an 8-sample call (which grows the rows they share): the same bits, and the
    rule's"""
    n = 100
    pos, vel = oracle.init_state(n, 1100)
    skin = K.skin_from_srgb8(reference_skin())
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(skin)
        before = sc.eyes() + sc.eyes_colour()
        sc.eyes_msaa()
        sc.eyes_msaa(width=2048, count=3)
        after = sc.eyes() + sc.eyes_colour()
    for x, y in zip(before, after):
        assert (bits(x) == bits(y)).all()
    cams = oracle.cameras(pos, vel, UP, R.eye_constant(oracle))
    for x, y in zip(after[2:], K.colour(cams, oracle.instances(pos, vel), 0, 1024, False, skin)):
        assert (bits(x) == bits(y)).all()
