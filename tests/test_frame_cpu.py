"""CPU tests of the scene camera's frame (nb_frame / nb_launch_frame / nb_camera_at): the numpy restatement
of the rule (tests/frame_restatement.py) on a hand-derived scene, against the eye row it must reduce to at H = 1, its coverage of
the scenes the GPU tests draw, and the new entry points' argument checks, which run before any device work."""
import os

import numpy as np
import pytest

import eyes_colour_restatement as K
import eyes_restatement as R
import frame_restatement as FR

F = np.float32
CLEAR_BGRA8 = 0xFF597C95
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def reference_skin():
    return K.skin_from_srgb8(np.load(os.path.join(GOLDEN, "skin_rgba8.npy")))


# -- the rule, restated ------------------------------------------------------------------------------------------------------------------
def test_hand_check_on_an_orthographic_camera(oracle):
    """W = 64, H = 32, xs = x + 32, ys = 16 - y, every depth 0.5; one body at (0.5, 0, 0) heading +x, white skin.  Its vertices
    project to (31.5, 17), (33.5, 16), (31.5, 15).  Edge 0 is x-major over columns 31 (t = 0, y = 17) and 32 (t = 0.5, y = 16.5);
    edge 1 is x-major over columns 32 (t = 0.5, y = 15.5) and 31 (t = 1, y = 15); edge 2 is y-major (dx = 0) over rows 15 (t = 0.25)
    and 16 (t = 0.75) at x = 31.5.  Pixel (31, 15) is written by edges 1 and 2 at the same depth: edge 1 shades it.  The vignette
    1 - ((u - 0.5)^2 + (v - 0.5)^2) at (0, 0), (0, 0.5), (1, 1), (0.5, 1), (0.25, 0.25)."""
    W, H = 64, 32
    inst = oracle.instances(np.array([[0.5, 0, 0]], F), np.array([[1, 0, 0]], F))
    stats = {}
    ids, depth, rgba, bgra8 = FR.frame(FR.ortho_camera(W, H), inst, W, H, stats=stats)
    want = {(31, 17): 0.5, (32, 16): 0.75, (31, 15): 0.5, (32, 15): 0.75, (31, 16): 0.875}
    want_ids = np.full((H, W), R.NONE, np.uint32)
    want_rgba = np.tile(K.CLEAR, (H, W, 1))
    for (c, r), v in want.items():
        want_ids[r, c] = 0
        want_rgba[r, c] = F([v, v, v, 1])
    assert (ids == want_ids).all(), np.argwhere(ids != want_ids)
    assert (bits(depth) == bits(np.where(want_ids == 0, F(0.5), F(1)))).all()
    assert (bits(rgba) == bits(want_rgba)).all()
    assert (bgra8[want_ids != 0] == CLEAR_BGRA8).all()
    assert bgra8[17, 31] == 0xFFBCBCBC and bgra8[16, 32] == 0xFFE1E1E1                    # 0.5 -> 188, 0.75 -> 225
    assert bgra8[16, 31] == 0xFF000000 | int(K.encode(F(0.875))) * 0x010101
    assert stats["kept"] == 3 and stats["xmajor"] == 2 and stats["ymajor"] == 1 and stats["writes"] == 6 and stats["covered"] == 5
    assert (stats["edge"] == [2, 2, 1]).all()                                             # the tie went to edge 1


def test_one_row_is_the_eyes_row(oracle):
    """planar data through an eye camera at H = 1: every clip y is +-0, so every edge is x-major at y = 0.5 and the frame is that
    eye's NB_EYES_SEE_SELF row, all four outputs, bit for bit -- with the reference skin"""
    pos, vel = oracle.init_state(100, 1100)
    inst = oracle.instances(pos, vel)
    cams = oracle.cameras(pos, vel, np.array([0, 0, 1], F), R.eye_constant(oracle, 1024))
    skin = reference_skin()
    covered = 0
    for e in range(100):
        stats = {}
        got = FR.frame(cams[e], inst, 1024, 1, skin=skin, stats=stats)
        want = K.colour(cams[e:e + 1], inst, e, 1024, see_self=True, skin=skin)
        for g, w in zip(got, want):
            assert g.shape[1:] == w.shape[1:] and (g.view(np.uint32) == w.view(np.uint32)).all(), e
        assert stats["ymajor"] == 0
        covered += stats["covered"]
    assert covered >= 30000, covered


def test_coverage_of_the_gpu_scenes(oracle):
    """what the GPU tests rest on, checked here with the restatement alone: the thresholds are the issue's, well below what its
    prototype observed (in the comments)"""
    st = {}
    pos, vel, cam, (W, H) = FR.scene(oracle, "reference")
    ids = FR.frame(cam, oracle.instances(pos, vel), W, H, stats=st)[0]
    assert st["bodies"] == 100, st                       # 300 kept, 150 / 150, 569 pixels, one depth value
    assert ids.shape == (1080, 1920)
    st = {}
    pos, vel, cam, (W, H) = FR.scene(oracle, "side")
    FR.frame(cam, oracle.instances(pos, vel), W, H, stats=st)
    assert st["xmajor"] >= 50 and st["ymajor"] >= 50, st  # 882 kept, 4 clipped, 692 / 130, 524 writes onto 276 pixels, 276 depths
    assert st["writes"] - st["covered"] >= 100 and st["depths"] >= 100 and st["clipped"] >= 1, st
    assert (st["edge"] > 0).all(), st                     # every edge index wins somewhere
    st = {}
    pos, vel, cam, (W, H) = FR.scene(oracle, "inside")
    FR.frame(cam, oracle.instances(pos, vel), W, H, stats=st)
    assert st["clipped"] >= 10 and st["writes"] - st["covered"] >= 500, st   # 3277 kept, 36 clipped, 2190 writes onto 779 pixels
    st = {}
    pos, vel, cam, (W, H) = FR.scene(oracle, "top")
    FR.frame(cam, oracle.instances(pos, vel), W, H, stats=st)
    assert st["kept"] >= 527 and st["clipped"] >= 6 and st["xmajor"] >= 275 and st["ymajor"] >= 252 and st["covered"] >= 338, st
    st = {}
    pos, vel, cam, (W, H) = FR.scene(oracle, "three")
    FR.frame(cam, oracle.instances(pos, vel), W, H, stats=st)
    assert st["longest"] > 72, st                         # an own-lane share plus more than one round of the wave (8 + 64)


def test_a_nan_camera_gives_the_clear_frame(oracle):
    pos, vel = oracle.init_state(16, 3)
    ids, depth, rgba, bgra8 = FR.frame(np.full((4, 4), np.nan, F), oracle.instances(pos, vel), 16, 8)
    assert (ids == R.NONE).all() and (depth == 1).all() and (bgra8 == CLEAR_BGRA8).all() and (bits(rgba) == bits(np.tile(K.CLEAR, (8, 16, 1)))).all()


# -- the entry points --------------------------------------------------------------------------------------------------------------------
def test_frame_entry_points_validate_before_touching_the_device(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    assert _lib.NB_FRAME_MAX_DIM == 4096
    buf = np.zeros(64, F)
    p = buf.ctypes.data
    assert lib.nb_frame(None, p, 4, 4, 0, None, None, None, p) == _lib.NB_ERR_INVALID
    assert "ctx is null" in _lib.last_error()
    assert lib.nb_camera_at(None, p, p, p, p, p) == _lib.NB_ERR_INVALID
    assert "ctx is null" in _lib.last_error()
    assert lib.nb_frame_scratch_bytes(1920, 1080) == 1920 * 1080 * 8
    big = _lib.NB_FRAME_MAX_DIM + 1
    assert lib.nb_frame_scratch_bytes(_lib.NB_FRAME_MAX_DIM, _lib.NB_FRAME_MAX_DIM) == 8 * 4096 * 4096
    for w, h in ((0, 4), (4, 0), (big, 4), (4, big), (0, 0)):
        assert lib.nb_frame_scratch_bytes(w, h) == 0
    fn = lib.nb_launch_frame
    # 16-byte aligned, never dereferenced: the checks come first
    cam, inst, skin, scr, a, b, c, d = 0x100000, 0x200000, 0x300000, 0x380000, 0x400000, 0x500000, 0x600000, 0x700000

    def rc(n=4, cam=cam, inst=inst, width=8, height=2, flags=0, skin=skin, tw=4, th=4, scratch=scr, ids=a, depth=b, rgba=c, bgra8=d):
        return fn(n, cam, inst, width, height, flags, skin, tw, th, scratch, ids, depth, rgba, bgra8, None)

    bigskin = _lib.NB_EYES_MAX_SKIN + 1
    cases = {
        "width 0": dict(width=0), "height 0": dict(height=0), "width above the maximum": dict(width=big),
        "height above the maximum": dict(height=big), "a flag": dict(flags=1), "flag bit 31": dict(flags=1 << 31),
        "no output": dict(ids=None, depth=None, rgba=None, bgra8=None),
        "ids = depth": dict(depth=a), "ids = rgba": dict(rgba=a), "ids = bgra8": dict(bgra8=a), "depth = rgba": dict(rgba=b),
        "depth = bgra8": dict(bgra8=b), "rgba = bgra8": dict(bgra8=c),
        "rgba over depth": dict(depth=c + 2 * 8 * 16 - 4), "bgra8 inside rgba": dict(bgra8=c + 64), "ids overlap depth": dict(depth=a + 60),
        "ids over cam": dict(ids=cam + 16), "depth over inst": dict(depth=inst + 200), "rgba over inst end": dict(rgba=inst + 4 * 64 - 16),
        "bgra8 over skin": dict(bgra8=skin + 4 * 4 * 16 - 4), "rgba over skin": dict(rgba=skin + 16),
        "scratch over ids": dict(scratch=a), "scratch over depth end": dict(scratch=b + 2 * 8 * 4 - 8), "scratch over rgba": dict(scratch=c + 16),
        "scratch over bgra8": dict(scratch=d - 8), "ids inside scratch": dict(ids=scr + 2 * 8 * 8 - 4),
        "null cam": dict(cam=None), "null inst": dict(inst=None), "null scratch": dict(scratch=None),
        "misaligned cam": dict(cam=cam + 4), "misaligned inst": dict(inst=inst + 8), "misaligned skin": dict(skin=skin + 4),
        "misaligned rgba": dict(rgba=c + 8), "misaligned scratch": dict(scratch=scr + 4), "misaligned bgra8": dict(bgra8=d + 2),
        "misaligned ids": dict(ids=a + 1), "misaligned depth": dict(depth=b + 3),
        "tw 0": dict(tw=0), "th 0": dict(th=0), "tw above the maximum": dict(tw=bigskin), "th above the maximum": dict(th=bigskin),
    }
    for what, kw in cases.items():
        assert rc(**kw) == _lib.NB_ERR_INVALID, what
    assert "alias" in (rc(bgra8=a) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "NB_FRAME_MAX_DIM" in (rc(width=0) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "NB_EYES_MAX_SKIN" in (rc(tw=bigskin) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "flags" in (rc(flags=1) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "all NULL" in (rc(ids=None, depth=None, rgba=None, bgra8=None) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert lib.nb_abi_version() == 2   # the change only adds symbols
    if lib.nb_device_count() == 0:
        # right up against each other is not an overlap; each output alone is enough; no skin: white; no bodies: no matrices
        for kw in (dict(), dict(depth=a + 2 * 8 * 4), dict(bgra8=c + 2 * 8 * 16), dict(scratch=a + 2 * 8 * 4), dict(ids=scr + 2 * 8 * 8),
                   dict(depth=None, rgba=None, bgra8=None), dict(ids=None, rgba=None, bgra8=None), dict(ids=None, depth=None, bgra8=None),
                   dict(ids=None, depth=None, rgba=None), dict(width=_lib.NB_FRAME_MAX_DIM, height=1), dict(width=1, height=_lib.NB_FRAME_MAX_DIM),
                   dict(width=1, height=1), dict(skin=None, tw=0, th=0), dict(tw=_lib.NB_EYES_MAX_SKIN, th=1), dict(n=0, inst=None)):
            assert rc(**kw) == _lib.NB_ERR_NO_DEVICE, kw
        with pytest.raises(nb.NbError):
            nb.Scene.new(4)


def test_the_python_names_are_exported(nb):
    assert nb.frame_constant is nb.scene.frame_constant and "frame_constant" in nb.__all__
    for name in ("frame", "scene_camera", "camera_at"):
        assert callable(getattr(nb.Scene, name))
    # host arithmetic, no device: the constant is camera_constant(90 / a, a, 1, 10000) with a = (float)W / (float)H
    a = F(1920) / F(1080)
    assert (bits(nb.frame_constant()) == bits(nb.camera_constant(float(F(90) / a), float(a), 1.0, 10000.0))).all()
