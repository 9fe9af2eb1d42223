"""CPU tests of the eye view's colour row (nb_eyes_colour / nb_launch_eyes_colour / nb_eyes_skin):
the library's two sRGB tables against high-precision arithmetic, the numpy restatement of the rule
(tests/eyes_colour_restatement.py) on hand-checked scenes, and the new entry points' argument checks, which run before any
device work."""
import math
import os

import numpy as np
import pytest

import eyes_colour_restatement as K
import eyes_restatement as R

F = np.float32
UP = np.array([0, 0, 1], np.float32)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def reference_skin():
    """the reference's 20 x 20 skin (assets/skin.png) as its RGBA bytes, (20, 20, 4) uint8, row 0 first"""
    return np.load(os.path.join(GOLDEN, "skin_rgba8.npy"))


def lattice(oracle, skin=None, stats=None):
    cams = np.repeat(R.lattice_camera()[None], 4, 0)
    return K.colour(cams, oracle.instances(R.LATTICE_POS, R.LATTICE_VEL), 0, 1024, see_self=True, skin=skin, stats=stats)


# -- the tables ----------------------------------------------------------------------------------------------------------------------
def test_the_librarys_tables_are_the_high_precision_ones(nb):
    """D[b] = binary32(decode(b / 255)), bit for bit against 50-digit arithmetic; T[b] = binary32(decode((b - 0.5) / 255)) is not
    exported, so it is pinned through the encoder: T[b] encodes to b and the float just below it to b - 1, for every b, which no
    other strictly increasing table satisfies"""
    D, T = K.decode_table(), K.encode_thresholds()
    assert (bits(nb.srgb_decode(np.arange(256))) == bits(D)).all()
    assert D[0] == 0 and D[255] == 1
    assert (np.diff(T[1:].astype(np.float64)) > 0).all() and T[1] > 0 and T[255] < 1
    b = np.arange(1, 256)
    assert (nb.srgb_encode(T[1:]) == b).all()
    assert (nb.srgb_encode(np.nextafter(T[1:], F(0))) == b - 1).all()
    assert (nb.srgb_encode(D) == np.arange(256)).all()
    # the restatement's encoder is the definition (a count of thresholds): the same on a dense sweep and on the specials
    x = np.concatenate([np.random.default_rng(5).uniform(-0.1, 1.1, 200000).astype(F),
                        F([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 2.0, 1e-30, -1.0])])
    assert (nb.srgb_encode(x) == K.encode(x)).all()
    assert nb.srgb_encode(F([np.nan]))[0] == 0 and nb.srgb_encode(F([1.0]))[0] == 255 and nb.srgb_encode(F([np.inf]))[0] == 255


def test_the_tables_in_the_source_are_constants_not_a_pow_at_load_time():
    """the committed header holds 2 x 256 literals which are the high-precision values"""
    import re

    from conftest import ROOT

    text = open(os.path.join(ROOT, "nenbody_amd", "csrc", "nb_srgb_tables.h")).read()
    assert "pow" not in re.sub(r"//.*", "", text)
    vals = [float.fromhex(v) for v in re.findall(r"(0x[0-9a-f.]+p[+-]\d+)f,", text)]
    assert len(vals) == 512
    assert (bits(F(vals[:256])) == bits(K.decode_table())).all()
    assert (bits(F(vals[256:])) == bits(K.encode_thresholds())).all()


def test_srgb_helpers_keep_shapes_and_reject_null(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    assert nb.srgb_decode(np.zeros((3, 5), np.uint8)).shape == (3, 5)
    assert nb.srgb_encode(np.zeros((2, 3, 4), F)).shape == (2, 3, 4) and nb.srgb_encode(np.zeros((2, 3, 4), F)).dtype == np.uint8
    assert lib.nb_srgb_decode_table(None) == _lib.NB_ERR_INVALID
    assert lib.nb_srgb_encode(None, 4, None) == _lib.NB_ERR_INVALID
    assert lib.nb_srgb_encode(None, 0, None) == _lib.NB_OK


# -- the rule, restated ------------------------------------------------------------------------------------------------------------------
def test_exact_lattice_white_skin(oracle):
    """the visible bodies 0, 2, 3 show 0.5 on their first column and 0.75 on their second: edge 0 runs from tc (0, 0) at t = 0 to
    (0, 0.5) at t = 0.5 with w = 1 throughout, so the vignette is 1 - (0.25 + 0.25) and 1 - (0.25 + 0); edge 1 ties it in depth on
    both columns and loses by draw order (body 3's edge 1 is cut by B4 and ties on 519).  Every other column is the clear colour.
    Bit for bit."""
    stats = {}
    ids, depth, rgba, bgra8 = lattice(oracle, stats=stats)
    want_ids, want_depth = R.lattice_expectation()
    want = np.tile(K.CLEAR, (1024, 1))
    want[[511, 514, 518]] = F([0.5, 0.5, 0.5, 1])
    want[[512, 515, 519]] = F([0.75, 0.75, 0.75, 1])
    for e in range(4):
        assert (ids[e] == want_ids).all() and (bits(depth[e]) == bits(want_depth)).all()
        assert (bits(rgba[e]) == bits(want)).all(), np.argwhere(bits(rgba[e]) != bits(want))[:4]
    assert (stats["edge"] == [4 * 6, 0, 0]).all()
    # the bytes: 0.5 -> 188, 0.75 -> 225, the clear colour (0.1, 0.2, 0.3) -> (89, 124, 149); in memory B, G, R, A
    assert bgra8[0, 511] == 0xFFBCBCBC and bgra8[0, 512] == 0xFFE1E1E1 and bgra8[0, 0] == 0xFF597C95
    assert (bgra8[0].view(np.uint8).reshape(1024, 4)[0] == [149, 124, 89, 255]).all()


@pytest.mark.parametrize("tw,th", [(2, 2), (7, 5)])
def test_exact_lattice_pins_the_texel_and_the_orientation(oracle, tw, th):
    """skins of distinct texels: edge 0 has u = 0 and v = s, so the first column (v = 0) fetches texel (ix 0, iy 0) and the second
    (v = 0.5) fetches (0, floor(th / 2)) -- row iy of the image as stored, NOT column iy and not a flipped row"""
    skin = (np.arange(th * tw * 4, dtype=np.float32).reshape(th, tw, 4) + F(1)) / F(256)      # exact, all distinct
    _, _, rgba, _ = lattice(oracle, skin=skin)
    for c0 in (511, 514, 518):
        assert (bits(rgba[0, c0, :3]) == bits(skin[0, 0, :3] * F(0.5))).all()
        assert (bits(rgba[0, c0 + 1, :3]) == bits(skin[th // 2, 0, :3] * F(0.75))).all()
        assert rgba[0, c0, 3] == 1 and rgba[0, c0 + 1, 3] == 1
    if tw != th:      # a transposed fetch would read another texel
        assert not (skin[th // 2, 0, :3] == skin[0, min(tw - 1, tw // 2), :3]).any()


def hand_check(oracle, skin=None, stats=None):
    pos, vel = np.array([[0, 0, 0], [10, 0, 0]], F), np.array([[1, 0, 0], [1, 0, 0]], F)
    cams = oracle.cameras(pos[:1], vel[:1], UP, R.eye_constant(oracle))
    return K.colour(cams, oracle.instances(pos, vel), 0, 1024, skin=skin, stats=stats)


def test_hand_check_one_body_straight_ahead(oracle):
    """eye at the origin, body at (10, 0, 0), both heading +x, white skin: columns 440 .. 583 are the rear edge (k = 2, both ends
    at w = 9, so s = t up to rounding and u = v = 1 - s): colour = 1 - 2 (0.5 - s)^2, greatest at the centre pair and 0.5 at the
    ends of the whole edge.

    The centre value.  The edge's ends project to xs = 512 -+ D with D = f / 18, f = 1 / tan(90 / 2048 degrees) (D = 72.43).  On
    columns 511 / 512, |0.5 - s| = 0.25 / D, so colour = 1 - 0.125 / D^2 = 1 - 40.5 tan^2(90 / 2048 degrees) = 0.99997617.
    Its error: allow each projected end an absolute error of E = 4 ulp(512) = 2^-12 (three roundings at magnitude < 1024 and the
    clip vertices' own).  t = (xc - xs0) / (xs1 - xs0) then errs by at most (E + 2 E t) / (2 D) + 2^-24 < 3.5e-6, s = (t i1) / i0 by
    0.2e-6 more (three roundings, i0 and i1 an ulp apart at most), du = (1 - s) - 0.5 by 2^-25 more: < 3.7e-6.  With
    |du| = 0.00345, m2 = 2 du^2 errs by 4 |du| 3.7e-6 = 5.1e-8 = 0.86 ulp of a value just below 1 (2^-24); the last subtraction
    adds half an ulp: 2 ulps bound the total.  Away from the centre |du| <= 0.5, so a column and its mirror image agree to
    2 * (4 * 0.5 * 3.7e-6) = 1.5e-5."""
    stats = {}
    ids, depth, rgba, bgra8 = hand_check(oracle, stats=stats)
    c = np.arange(440, 584)
    assert (np.nonzero(ids[0] != R.NONE)[0] == c).all() and (stats["edge"] == [0, 0, 144]).all()
    r = rgba[0, :, 0].astype(np.float64)
    assert (bits(rgba[0, c, 0]) == bits(rgba[0, c, 1])).all() and (bits(rgba[0, c, 0]) == bits(rgba[0, c, 2])).all()
    assert (rgba[0, c, 3] == 1).all()
    want = 1.0 - 40.5 * math.tan(math.radians(90.0 / 2048.0)) ** 2
    for col in (511, 512):
        assert abs(r[col] - want) <= 2 * 2.0 ** -24, (col, r[col], want)
    assert np.abs(r[c] - r[c][::-1]).max() <= 1.5e-5                      # symmetric about the centre pair
    assert r[c].max() == max(r[511], r[512]) and r[c].min() >= 0.5       # greatest there, not below 0.5 anywhere
    assert (np.diff(r[440:512]) >= 0).all() and (np.diff(r[512:584]) <= 0).all()
    rest = np.setdiff1d(np.arange(1024), c)
    assert (bits(rgba[0, rest]) == bits(np.tile(K.CLEAR, (len(rest), 1)))).all()
    assert (bgra8[0, rest] == 0xFF597C95).all() and bgra8[0, 511] == 0xFFFFFFFF


def test_the_reference_skin_is_fetched(oracle):
    """the decoded skin.png (20 x 20 Rgba8UnormSrgb): the rear edge has u = v = 1 - s, so the 144 columns walk the image's
    diagonal; each colour is that texel times the white skin's vignette, and texels other than white are among them"""
    img = reference_skin()
    assert img.shape == (20, 20, 4) and img.dtype == np.uint8
    skin = K.skin_from_srgb8(img)
    _, _, white, _ = hand_check(oracle)
    ids, _, rgba, bgra8 = hand_check(oracle, skin=skin)
    c = np.arange(440, 584)
    f = white[0, c, 0]
    diag = skin[np.arange(20), np.arange(20), :3]
    cand = diag[:, None, :] * f[None, :, None]                            # (20, 144, 3): each diagonal texel under each column's vignette
    hit = (bits(cand) == bits(rgba[0, c, :3])[None]).all(-1)
    assert hit.any(0).all()
    assert len({tuple(diag[i]) for i in np.nonzero(hit.any(1))[0]}) >= 3  # several distinct texels, so not the white skin
    assert (bgra8[0, c] != hand_check(oracle)[3][0, c]).any()


def test_the_python_skin_decoding_is_the_restatements(nb):
    """Scene.set_skin's uint8 path decodes through the library's D; here without a device: the same arithmetic by hand"""
    img = reference_skin()
    lin = np.empty(img.shape, F)
    lin[..., :3] = nb.srgb_decode(img[..., :3])
    lin[..., 3] = img[..., 3].astype(F) / F(255)
    assert (bits(lin) == bits(K.skin_from_srgb8(img))).all()


def test_coverage_of_the_gpu_cases(oracle):
    """what the GPU tests rest on, checked here with the restatement (tests/test_gpu_eyes_colour.py uses these seeds): at N = 100
    more than a tenth of the columns see a body; over N = 100 and 257 every edge index wins columns; winning edges with unequal
    end w (step 7 is not the linear case) and winning edges cut where they enter (s0 > 0) both occur"""
    cp = R.eye_constant(oracle)
    total = {}
    for n in (100, 257):
        pos, vel = oracle.init_state(n, 1000 + n)
        stats = {}
        for see_self in (False, True):
            K.colour(oracle.cameras(pos[:40], vel[:40], UP, cp), oracle.instances(pos, vel), 0, 1024, see_self, stats=stats)
        if n == 100:
            assert stats["covered"] > 0.1 * stats["columns"]
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
    assert (total["edge"] > 100).all(), total
    assert total["unequal_w"] > 1000 and total["s0>0"] > 0, total


# -- the entry points --------------------------------------------------------------------------------------------------------------------
def test_colour_entry_points_validate_before_touching_the_device(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    up, cp = np.array([0, 0, 1], F), np.zeros(16, F)
    buf = np.zeros(64, F)
    assert lib.nb_eyes_colour(None, 0, 1, up.ctypes.data, cp.ctypes.data, 8, 0, None, None, buf.ctypes.data, None) == _lib.NB_ERR_INVALID
    assert "ctx is null" in _lib.last_error()
    assert lib.nb_eyes_skin(None, buf.ctypes.data, 2, 2) == _lib.NB_ERR_INVALID
    assert "ctx is null" in _lib.last_error()
    fn = lib.nb_launch_eyes_colour
    # 16-byte aligned, never dereferenced: the checks come first
    cams, inst, skin, a, b, c, d = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000

    def rc(n=4, first=0, count=2, cams=cams, inst=inst, width=8, flags=0, skin=skin, tw=4, th=4, ids=a, depth=b, rgba=c, bgra8=d):
        return fn(n, first, count, cams, inst, width, flags, skin, tw, th, ids, depth, rgba, bgra8, None)

    big = _lib.NB_EYES_MAX_SKIN + 1
    cases = {
        "width 0": dict(width=0), "width above the maximum": dict(width=_lib.NB_EYES_MAX_WIDTH + 1),
        "range past n": dict(first=3), "count past n": dict(count=5), "unknown flag": dict(flags=2), "flag bit 31": dict(flags=1 << 31),
        "no colour output": dict(rgba=None, bgra8=None), "no output at all": dict(ids=None, depth=None, rgba=None, bgra8=None),
        "ids = depth": dict(depth=a), "ids = bgra8": dict(bgra8=a), "depth = bgra8": dict(bgra8=b), "rgba = ids": dict(ids=c),
        "rgba over depth": dict(depth=c + 2 * 8 * 16 - 4), "bgra8 inside rgba": dict(bgra8=c + 64), "ids overlap depth": dict(depth=a + 60),
        "ids over cams": dict(ids=cams + 16), "depth over inst": dict(depth=inst + 200), "rgba over inst end": dict(rgba=inst + 4 * 64 - 16),
        "bgra8 over skin": dict(bgra8=skin + 4 * 4 * 16 - 4), "rgba over skin": dict(rgba=skin + 16),
        "null cams": dict(cams=None), "null inst": dict(inst=None), "misaligned cams": dict(cams=cams + 4),
        "misaligned inst": dict(inst=inst + 8), "misaligned skin": dict(skin=skin + 4), "misaligned rgba": dict(rgba=c + 8),
        "misaligned bgra8": dict(bgra8=d + 2), "misaligned ids": dict(ids=a + 1),
        "tw 0": dict(tw=0), "th 0": dict(th=0), "tw above the maximum": dict(tw=big), "th above the maximum": dict(th=big),
    }
    for what, kw in cases.items():
        assert rc(**kw) == _lib.NB_ERR_INVALID, what
    assert "alias" in (rc(bgra8=a) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "width" in (rc(width=0) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "NB_EYES_MAX_SKIN" in (rc(tw=big) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "rgba and bgra8" in (rc(rgba=None, bgra8=None) == _lib.NB_ERR_INVALID and _lib.last_error())
    # count = 0 is a no-op (no device needed)
    assert rc(count=0) == _lib.NB_OK and rc(count=0, first=4) == _lib.NB_OK
    # the depth / id entry goes on refusing flags = 2, and the ABI version stays: the change only adds symbols
    assert lib.nb_launch_eyes(4, 0, 2, cams, inst, 8, 2, a, b, None) == _lib.NB_ERR_INVALID
    assert lib.nb_abi_version() == 2
    if lib.nb_device_count() == 0:
        # right up against each other is not an overlap; each output alone is enough, given a colour output; no skin: white
        for kw in (dict(), dict(depth=a + 2 * 8 * 4), dict(bgra8=c + 2 * 8 * 16), dict(ids=None, depth=None, bgra8=None),
                   dict(ids=None, depth=None, rgba=None), dict(ids=None), dict(depth=None), dict(flags=_lib.NB_EYES_SEE_SELF),
                   dict(width=_lib.NB_EYES_MAX_WIDTH), dict(width=1), dict(first=2), dict(skin=None, tw=0, th=0),
                   dict(tw=_lib.NB_EYES_MAX_SKIN, th=1)):
            assert rc(**kw) == _lib.NB_ERR_NO_DEVICE, kw
        with pytest.raises(nb.NbError):
            nb.Scene.new(4)
