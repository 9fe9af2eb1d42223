"""CPU tests of the frame through 8 samples per pixel (nb_frame_msaa / nb_launch_frame_msaa): the numpy
restatement of the rule (tests/frame_msaa_restatement.py) on the hand-derived scene, against the 8-sample eye row it must reduce to
at H = 1 and the one-sample frame it must reduce to where one fragment fills a pixel, its coverage of the scenes the GPU tests draw,
and the sample offsets, which are host arithmetic."""
import os

import numpy as np
import pytest

import eyes_colour_restatement as K
import eyes_msaa_restatement as M
import eyes_restatement as R
import frame_msaa_restatement as FM
import frame_restatement as FR

F = np.float32
CLEAR_BGRA8 = 0xFF597C95
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ("reference", "side", "inside", "top", "three")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def reference_skin():
    return K.skin_from_srgb8(np.load(os.path.join(GOLDEN, "skin_rgba8.npy")))


def tree(a):
    """FM5 on eight binary32 values"""
    a = [F(v) for v in a]
    return (((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) * F(0.125)


@pytest.fixture(scope="module")
def scenes(oracle):
    """each scene once: (the 8-sample frame, its stats, the one-sample frame)"""
    out = {}
    for name in SCENES:
        pos, vel, cam, (W, H) = FR.scene(oracle, name)
        inst = oracle.instances(pos, vel)
        stats = {}
        out[name] = (FM.frame_msaa(cam, inst, W, H, stats=stats), stats, FR.frame(cam, inst, W, H))
    return out


# -- the rule, restated ------------------------------------------------------------------------------------------------------------------
def test_hand_check_on_an_orthographic_camera(oracle):
    """W = 64, H = 32, xs = x + 32, ys = 16 - y, every depth 0.5; one body at (0.5, 0, 0) heading +x, white skin: the vertices
    project to (31.5, 17), (33.5, 16), (31.5, 15), as in section 11's hand check.  Every t is a multiple of 1/32: each step is exact.

    Edge 0, (31.5, 17) -> (33.5, 16), x-major: t_k = (m + ox_k - 31.5) / 2, e_k = 17.5 - t_k - oy_k.  Step 31 tries the samples with
    ox_k >= 1/2, k = 0, 2, 6, 7: e = 17.5 - (11, 23, 33, 9) / 32, rows 17, 16, 16, 17.  Step 32 tries all eight:
    e_k = 17.25 - (ox_k / 2 + oy_k) = 17.25 - (19, 29, 31, 11, 29, 15, 41, 17) / 32, row 16 but for k = 6, row 15.  Step 33 tries
    ox_k < 1/2, k = 1, 3, 4, 5: e = 16.75 - (29, 11, 29, 15) / 32, rows 15, 16, 15, 16.
    Edge 1, (33.5, 16) -> (31.5, 15), x-major: t_k = (33.5 - m - ox_k) / 2, e_k = 16.5 - t_k - oy_k.  Step 33, k = 1, 3, 4, 5:
    e = 16.25 + (-15, -1, -23, -13) / 32, rows 15, 16, 15, 15.  Step 32: e_k = 15.75 + (-1, -15, -5, -1, -23, -13, -19, 13) / 32, row
    15 for k = 0 .. 6 and row 16 for k = 7.  Step 31, k = 0, 2, 6, 7: e = 15.25 + (-1, -5, -19, 13) / 32, rows 15, 15, 14, 15.
    Edge 2, (31.5, 15) -> (31.5, 17), y-major (dx = 0): a_k = m + oy_k lies in [15, 17) for all eight samples of rows 15 and 16 and
    for none of any other row; e_k = 31.5 + (0.5 - ox_k) = 32 - ox_k, column 31 for every k.
    That is 16 sample writes per edge, 48, onto 38 samples of 8 pixels.  Every depth is 0.5, so a sample two edges write has one key
    and FM3 gives it to the first edge in draw order: edge 0 keeps (32, 15)'s k = 6, (33, 15)'s k = 1, 4, (33, 16)'s k = 3, (32, 16)'s
    k = 7 against edge 1, and (31, 16)'s k = 2, 6 against edge 2; edge 1 keeps (31, 15)'s k = 0, 2, 7 against edge 2.

    The fragments (FM4; no clip, every w is 1, so s = t at the pixel centre, clamped).  Edge 0, (u, v) = (0, s): column 31, t = 0,
    0.5; column 32, t = 1/2, 0.75; column 33, t = 1, 0.5 -- its centre 33.5 is the edge's open end: extrapolated, four samples.
    Edge 1, (s, 1): column 33, t = 0, 0.5 -- the centre 33.5 is again outside [31.5, 33.5): one sample; column 32, t = 1/2, 0.75;
    column 31, t = 1, 0.5.  Edge 2, (1 - s, 1 - s): row 15, t = 1/4, 1 - 2/16 = 0.875; row 16, t = 3/4, 0.875.
    The resolve (FM5): (31, 15) holds 0.5 in k = 0, 2, 7 and 0.875 in the rest: ((1.375 + 1.375) + (1.75 + 1.375)) / 8 = 0.734375;
    (31, 16) holds 0.5 in k = 2, 6: ((1.75 + 1.375) + (1.75 + 1.375)) / 8 = 0.78125; (33, 15) holds 0.5 in k = 1, 4, 5 and the clear
    colour elsewhere: red ((0.6 + 0.2) + (1.0 + 0.2)) / 8 = 0.25, green 0.3125, blue 0.375 once rounded."""
    W, H = 64, 32
    inst = oracle.instances(np.array([[0.5, 0, 0]], F), np.array([[1, 0, 0]], F))
    stats = {}
    ids8, depth8, rgba, bgra8 = FM.frame_msaa(FR.ortho_camera(W, H), inst, W, H, stats=stats)
    # (column, row): {sample: winning edge}
    want = {
        (31, 14): {6: 1},
        (31, 15): {0: 1, 1: 2, 2: 1, 3: 2, 4: 2, 5: 2, 6: 2, 7: 1},
        (32, 15): {0: 1, 1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 0},
        (33, 15): {1: 0, 4: 0, 5: 1},
        (31, 16): {0: 2, 1: 2, 2: 0, 3: 2, 4: 2, 5: 2, 6: 0, 7: 2},
        (32, 16): {0: 0, 1: 0, 2: 0, 3: 0, 4: 0, 5: 0, 7: 0},
        (33, 16): {3: 0, 5: 0},
        (31, 17): {0: 0, 7: 0},
    }
    # the fragment of (column, row, edge): the vignette under the white skin
    frag = {(31, 14, 1): 0.5, (31, 15, 1): 0.5, (31, 15, 2): 0.875, (32, 15, 1): 0.75, (32, 15, 0): 0.75, (33, 15, 0): 0.5, (33, 15, 1): 0.5,
            (31, 16, 2): 0.875, (31, 16, 0): 0.5, (32, 16, 0): 0.75, (33, 16, 0): 0.5, (31, 17, 0): 0.5}
    want_ids8 = np.full((H, W, 8), R.NONE, np.uint32)
    want_edge8 = np.full((H, W, 8), -1, np.int8)
    want_rgba = np.tile(K.CLEAR, (H, W, 1))
    for (c, r), samples in want.items():
        for k, e in samples.items():
            want_ids8[r, c, k], want_edge8[r, c, k] = 0, e
        for ch in range(4):
            want_rgba[r, c, ch] = tree([(1.0 if ch == 3 else frag[c, r, samples[k]]) if k in samples else K.CLEAR[ch] for k in range(8)])
    assert sum(len(s) for s in want.values()) == 38
    assert (ids8 == want_ids8).all(), np.argwhere(ids8 != want_ids8)
    assert (bits(depth8) == bits(np.where(want_ids8 == 0, F(0.5), F(1)))).all()
    assert (stats["edge8"] == want_edge8).all(), np.argwhere(stats["edge8"] != want_edge8)
    assert (bits(rgba) == bits(want_rgba)).all(), np.argwhere(bits(rgba) != bits(want_rgba))
    # the two full pixels and one partial one, written out: 3 x 0.5 + 5 x 0.875 and 2 x 0.5 + 6 x 0.875 over 8, all exact
    assert (rgba[15, 31] == F([0.734375, 0.734375, 0.734375, 1])).all() and (rgba[16, 31] == F([0.78125, 0.78125, 0.78125, 1])).all()
    # (33, 15): three fragments of 0.5 and five clear samples, in the tree's order: k = 1, 4, 5 hold the body
    c = K.CLEAR
    assert (rgba[15, 33, :3] == [((((c[i] + F(0.5)) + (c[i] + c[i])) + ((F(0.5) + F(0.5)) + (c[i] + c[i]))) * F(0.125)) for i in range(3)]).all()
    assert (bits(rgba[15, 33]) == bits(F([0.25, 0.3125, 0.375, 1]))).all()
    assert (bgra8[(want_ids8 != 0).all(-1)] == CLEAR_BGRA8).all()
    assert bgra8[15, 31] == 0xFF000000 | int(K.encode(F(0.734375))) * 0x010101 == 0xFFDFDFDF
    assert bgra8[16, 31] == 0xFF000000 | int(K.encode(F(0.78125))) * 0x010101 == 0xFFE5E5E5
    assert bgra8[15, 33] == (0xFF000000 | int(K.encode(F(0.25))) << 16 | int(K.encode(F(0.3125))) << 8 | int(K.encode(F(0.375)))) == 0xFF8998A5
    assert stats["writes"] == 48 and (stats["covered_hist"] == [64 * 32 - 8, 1, 2, 1, 0, 0, 0, 2, 2]).all()
    assert (stats["edge"] == [16, 11, 11]).all() and stats["two_bodies"] == 0
    # the one-sample rule sets five of the eight pixels; (31, 14), (33, 15) and (33, 16) only show through their samples
    assert stats["empty_centre"] == 3 and stats["centre_only"] == 0
    # shaded at a centre outside their edge's half-open span: edge 0's four samples and edge 1's one in column 33
    assert stats["extrapolated"] == 5


def test_one_row_is_the_eyes_msaa_row(oracle):
    """planar data through an eye camera at H = 1: every ys is 0.5, so every edge is x-major and every e_k = 1 - oy_k lies in
    (0, 1): the frame is that eye's NB_EYES_SEE_SELF 8-sample row, all four outputs, bit for bit -- with the reference skin, all
    100 eyes of N = 100"""
    pos, vel = oracle.init_state(100, 1100)
    inst = oracle.instances(pos, vel)
    cams = oracle.cameras(pos, vel, np.array([0, 0, 1], F), R.eye_constant(oracle, 1024))
    skin = reference_skin()
    want = M.msaa(cams, inst, 0, 1024, see_self=True, skin=skin)
    covered = 0
    for e in range(100):
        got = FM.frame_msaa(cams[e], inst, 1024, 1, skin=skin)
        for g, w in zip(got, want):
            assert g.shape[1:] == w.shape[1:] and (g.view(np.uint32) == w[e:e + 1].view(np.uint32)).all(), e
        covered += int((got[0] != R.NONE).sum())
    assert covered >= 250000, covered                                                        # 281 524


def test_where_one_fragment_fills_a_pixel_it_is_the_one_sample_frame(scenes, oracle):
    """every pixel whose eight samples hold one (body, edge), which is also F1-F6's winner and edge there: the fragment is F6's (the
    same t at the same centre) and the mean of eight equal values is that value, so rgba and bgra8 equal the one-sample frame's bit
    for bit.  Such pixels exist in every scene (17, 3, 22, 1, 59 of them)."""
    for name in SCENES:
        (_, _, rgba, bgra8), stats, (_, _, rgba1, bgra1) = scenes[name]
        one = stats["one"]
        assert one.sum() > 0, name
        assert (bits(rgba[one]) == bits(rgba1[one])).all() and (bgra8[one] == bgra1[one]).all(), name


def test_where_the_skin_varies_too(oracle):
    """the same property under a random skin on "inside", the scene with the most such pixels per area"""
    pos, vel, cam, (W, H) = FR.scene(oracle, "inside")
    inst = oracle.instances(pos, vel)
    skin = np.random.default_rng(11).uniform(0, 1, (5, 7, 4)).astype(F)
    stats = {}
    _, _, rgba, bgra8 = FM.frame_msaa(cam, inst, W, H, skin=skin, stats=stats)
    _, _, rgba1, bgra1 = FR.frame(cam, inst, W, H, skin=skin)
    one = stats["one"]
    assert one.sum() >= 10 and len(np.unique(bgra8[one])) > 3
    assert (bits(rgba[one]) == bits(rgba1[one])).all() and (bgra8[one] == bgra1[one]).all()


def test_coverage_of_the_gpu_scenes(scenes):
    """what the GPU tests rest on, checked here with the restatement alone (the issue's prototype counts in the comments: they are
    reproduced exactly)"""
    seen = {
        "reference": (5356, [189, 132, 112, 118, 110, 132, 198, 64], 6, 486),
        "side": (3931, [210, 134, 101, 82, 70, 44, 34, 25], 82, 424),
        "inside": (17633, [96, 91, 79, 127, 104, 151, 165, 321], 491, 355),
        "top": (4129, [206, 138, 97, 106, 69, 57, 67, 49], 33, 451),
        "three": (5907, [157, 259, 136, 360, 145, 270, 71, 64], 6, 728),
    }
    for name in SCENES:
        (ids8, depth8, rgba, bgra8), st, _ = scenes[name]
        assert (st["covered_hist"][1:] > 0).all(), (name, st["covered_hist"])              # every partial count 1 .. 8
        assert st["two_bodies"] > 0, name
        assert (st["edge"] > 0).all(), (name, st["edge"])                                   # every edge index wins samples
        assert st["centre_only"] == 0, name                                                 # a covered centre has a covered sample
        writes, hist, two, empty = seen[name]
        assert st["writes"] == writes and (st["covered_hist"][1:] == hist).all() and st["two_bodies"] == two and st["empty_centre"] == empty, name
        assert (rgba[..., 3] == 1).all()                                                     # eight alphas of 1
    assert scenes["reference"][0][0].shape == (1080, 1920, 8)


def test_a_nan_camera_gives_the_clear_frame(oracle):
    pos, vel = oracle.init_state(16, 3)
    ids8, depth8, rgba, bgra8 = FM.frame_msaa(np.full((4, 4), np.nan, F), oracle.instances(pos, vel), 16, 8)
    assert ids8.shape == (8, 16, 8) and (ids8 == R.NONE).all() and (depth8 == 1).all() and (bgra8 == CLEAR_BGRA8).all()
    assert (bits(rgba) == bits(np.tile(K.CLEAR, (8, 16, 1)))).all()                          # the mean of eight clear samples is the clear colour


# -- host arithmetic of the library ---------------------------------------------------------------------------------------------------------
def test_the_sample_offsets(nb):
    from nenbody_amd import _lib

    o = nb.frame_sample_offsets()
    assert o.shape == (2, 8) and o.dtype == np.float32
    assert (o[0] * 16 == [9, 7, 13, 5, 3, 1, 11, 15]).all() and (o[1] * 16 == [5, 11, 9, 3, 13, 7, 15, 1]).all()
    assert (bits(o[0]) == bits(FM.OX)).all() and (bits(o[1]) == bits(FM.OY)).all()
    assert (bits(o[0]) == bits(nb.eye_sample_offsets())).all() and (bits(FM.OX) == bits(M.OFFSETS)).all()
    assert _lib.load().nb_frame_sample_offsets(None) == _lib.NB_ERR_INVALID and "null" in _lib.last_error()
    assert nb.frame_sample_offsets is nb.scene.frame_sample_offsets and "frame_sample_offsets" in nb.__all__
    assert callable(nb.Scene.frame_msaa) and _lib.NB_FRAME_MSAA_MAX_DIM == 2048
