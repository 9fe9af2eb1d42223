"""CPU tests of the located seen sets and the vision-only gravity step: the numpy restatement
(tests/located_restatement.py) on a two-body case whose bits are derived by hand in exact rational arithmetic, its accuracy against the
TRUE relative positions on the reference's initial state, its fold against the C oracle's n-body step, the rule's corner cases (L1's
tie, the slot without a column, L5, L6), and the new entry points' argument checks, which run before any device work."""
import ctypes
import functools
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import eyes_restatement as R
import located_restatement as L
import seen_restatement as S
from conftest import ROOT

F = np.float32
UP = np.array([0, 0, 1], F)
NONE = L.NONE
EXE = os.path.join(ROOT, "build", "located_check")
NAMES = ("nb_seen_located_launch", "nb_eyes_located", "nb_nbody_located_step_launch", "nb_step_nbody_located")

# The accuracy bound |rel - (p_j - p_n)| <= sqrt(2) + C 2^-24 rho^2 (rho: the true distance of the centres).  sqrt(2): the estimate is
# a point of the seen body's outline, whose farthest point from the centre is a vertex.  2^-24 rho^2: the depth buffer's resolution
# at that range -- d = 1.0001 (1 - 1 / r) lies in [0.5, 1), where binary32 values are 2^-24 apart, and dr/dd = r^2 / 1.0001.
# Measured with this restatement over the four cases below: worst C = 1.33270 (N = 100, seed 1100, W = 1024); fixed at four times that.
C_MEASURED = 1.33270
C_BOUND = 4 * C_MEASURED


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f32(word):
    return np.uint32(word).view(np.float32)


@functools.lru_cache(maxsize=None)
def reference_rows(n, seed, width):
    """(pos, vel, cp, ids, depth) of the reference init by the numpy eye rule, cameras and matrices by the oracle; computed once"""
    import oracle

    oracle.build()
    oracle.load()
    pos, vel = oracle.init_state(n, seed)
    cp = R.eye_constant(oracle, width)
    ids, depth = R.eyes(oracle.cameras(pos, vel, UP, cp), oracle.instances(pos, vel), 0, width)
    for a in (pos, vel, cp, ids, depth):
        a.setflags(write=False)
    return pos, vel, cp, ids, depth


# -- exact rational arithmetic, rounded to binary32 by hand ------------------------------------------------------------------------------
def rn(x):
    """the binary32 nearest to the rational x, ties to even (normal and subnormal range, no overflow), as a Fraction"""
    x = Fraction(x)
    if x == 0:
        return x
    sign, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = Fraction(2) ** (max(e, -126) - 23)
    m, rest = divmod(a, q)
    if rest * 2 > q or (rest * 2 == q and m % 2):
        m += 1
    return sign * m * q


def frac(word):
    return Fraction(float(f32(word)))


def word(x):
    return int(bits(F(float(x)))[0])          # (exact: x is a binary32)


def test_rn_is_numpys_binary32_arithmetic():
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=200).astype(F), rng.normal(size=200).astype(F)
    for x, y in zip(a, b):
        fx, fy = Fraction(float(x)), Fraction(float(y))
        assert word(rn(fx + fy)) == bits(x + y)[0] and word(rn(fx * fy)) == bits(x * y)[0] and word(rn(fx / fy)) == bits(x / y)[0]


# -- the hand case -----------------------------------------------------------------------------------------------------------------------
def test_hand_case_two_bodies_in_binary32(oracle):
    """Bodies at (0,0,0) and (10,0,0), both heading +x, W = 1024, the reference's eye constant: cp[0] = 0x3FA2F981 (1 / tan(45 degrees / 1024) / 1024: 4 / pi less 2 ulp),
    cp[10] = cp[14] = 0xBF800347 (-1.0001).  Eye 0 sees body 1's rear edge x = 9, y in [-1, 1], over columns 440 .. 583 at the one
    depth 0x3F63940C; L1 gives column 440.  L2 in exact rationals, every operation rounded to binary32:
        h = 512, xc = 440.5, xn = -71.5 / 512 (exact);  t = rn(d + cp[10]);  r = rn(cp[14] / t) = 0x410FFFFE = 9 - 2 ulp;
        xv = rn(rn(xn r) / cp[0]) = -0x3F7CB3AE
    |r - 9|: the row's d is within 2^-23 of the exact depth 1.0001 (1 - 1/9) -- two spacings of [0.5, 1) for the eye rule's own
    roundings --, dr/dd = 81 / 1.0001, and L2's two operations round r's 2^-20 spacing twice: |r - 9| <= 81 2^-23 + 2^-20 < 1.1e-5.
    L3: f = (1, 0, 0); f x up = (0 1 - 0 0, 0 0 - 1 1, 1 0 - 0 0) = (0, -1, 0) = s.  L4: rel = (r 1 + xv 0, r 0 + xv (-1), r 0 + xv 0, r)
    = (r, -xv, +0, r) -- the corner (9, 1) seen half a column early: the column's centre 440.5 lies at y = 0.98712.
    Eye 1 looks away from body 0, sees nobody and coasts: v = (1, 0, 0) + 0 dt, p = v + p = (11, 0, 0)."""
    pos = np.array([[0, 0, 0], [10, 0, 0]], F)
    vel = np.array([[1, 0, 0], [1, 0, 0]], F)
    cp = R.eye_constant(oracle, 1024)
    assert (bits(cp).reshape(16)[[0, 10, 11, 14]] == [0x3FA2F981, 0xBF800347, 0xBF800000, 0xBF800347]).all() and L.invertible(cp) is None
    ids, depth = R.eyes(oracle.cameras(pos, vel, UP, cp), oracle.instances(pos, vel), 0, 1024)
    assert (np.nonzero(ids[0] != NONE)[0] == np.arange(440, 584)).all() and (bits(depth[0, 440:584]) == 0x3F63940C).all()
    count, sids, sdepth, _, col, rel = L.located_of_rows(ids, depth, vel, UP, cp)
    assert (count == [1, 0]).all() and sids[0, 0] == 1 and bits(sdepth[0, 0]) == 0x3F63940C
    # L2 by hand
    d, cp0, cp10, cp14 = frac(0x3F63940C), frac(0x3FA2F981), frac(0xBF800347), frac(0xBF800347)
    xn = rn((rn(Fraction(440) + Fraction(1, 2)) - 512) / 512)
    assert xn == Fraction(-143, 1024)
    r = rn(cp14 / rn(d + cp10))
    xv = rn(rn(xn * r) / cp0)
    assert word(r) == 0x410FFFFE and word(-xv) == 0x3F7CB3AE
    assert abs(r - 9) <= Fraction(81, 2 ** 23) + Fraction(1, 2 ** 20) and abs(float(-xv) - 0.98712) < 1e-5
    # L3
    f, s = L.axes(vel, UP)
    assert (bits(f[0]) == bits(F([1, 0, 0]))).all() and (s[0] == [0, -1, 0]).all() and bits(s[0])[1] == 0xBF800000
    # L1, L4, L5: the restatement gives the hand-derived words
    assert col[0, 0] == 440 and (col[0, 1:] == NONE).all() and (col[1] == NONE).all()
    assert (bits(rel[0, 0]) == [0x410FFFFE, 0x3F7CB3AE, 0, 0x410FFFFE]).all()
    assert (bits(rel[0, 1:]) == 0).all() and (bits(rel[1]) == 0).all()
    # G2-G3: body 0 is pulled towards what it sees, body 1 coasts
    p, v = L.nbody_located_step(pos, vel, count, rel)
    assert (bits(v[1]) == bits(F([1, 0, 0]))).all() and (bits(p[1]) == bits(F([11, 0, 0]))).all()
    vec = [frac(0x410FFFFE), frac(0x3F7CB3AE), Fraction(0)]
    dist = rn(rn(rn(rn(vec[0] * vec[0]) + rn(vec[1] * vec[1])) + 0) + Fraction(float(F(0.0000001))))
    g, dt = Fraction(float(F(0.001))), Fraction(float(F(0.1)))
    want_v = [rn(c + rn(rn(rn(x * g) / dist) * dt)) for c, x in zip((1, 0, 0), vec)]
    assert [word(x) for x in want_v] == list(bits(v[0])) and [word(rn(a + b)) for a, b in zip(want_v, (0, 0, 0))] == list(bits(p[0]))
    assert v[0, 0] > 1 and v[0, 1] > 0 and v[0, 2] == 0


# -- accuracy against the truth ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(100, 1100), (257, 1257)])
@pytest.mark.parametrize("width", [64, 1024])
def test_every_member_is_located_within_the_outline_and_the_depth_resolution(n, seed, width):
    pos, vel, cp, ids, depth = reference_rows(n, seed, width)
    count, sids, _, _, col, rel = L.located_of_rows(ids, depth, vel, UP, cp)
    assert (count == S.mask_of_rows(ids, n).sum(1)).all() and count.sum() > 1000
    used = np.arange(width)[None, :] < count[:, None]
    assert (col[used] != NONE).all() and (col[~used] == NONE).all()                       # no member is left out
    e, k = np.nonzero(used)
    true = pos[sids[e, k]].astype(np.float64) - pos[e].astype(np.float64)
    err = np.linalg.norm(rel[e, k, :3].astype(np.float64) - true, axis=1)
    rho = np.linalg.norm(true, axis=1)
    c = (err - math.sqrt(2)) / (2.0 ** -24 * rho * rho)
    print(f"N={n} W={width}: {len(e)} members, worst |estimate - true centre| {err.max():.5f}, worst C {c.max():.5f}, largest range {rel[e, k, 3].max():.1f}")
    assert (err <= math.sqrt(2) + C_BOUND * 2.0 ** -24 * rho * rho).all(), (err.max(), c.max())
    assert c.max() <= C_MEASURED * 1.0001                                                 # the recorded worst is the worst
    assert (rel[e, k, 3] > 0).all() and (rel[e, k, 3].astype(np.float64) <= rho + 1.5).all()         # r: the distance along the heading


def test_vision_only_steps_stay_finite_and_the_blind_coast():
    pos, vel, cp, _, _ = reference_rows(100, 1100, 1024)
    import oracle

    p, v = pos.copy(), vel.copy()
    for step in range(2):
        ids, depth = R.eyes(oracle.cameras(p, v, UP, cp), oracle.instances(p, v), 0, 1024)
        count, _, _, _, _, rel = L.located_of_rows(ids, depth, v, UP, cp)
        blind = count == 0
        p1, v1 = L.nbody_located_step(p, v, count, rel)
        assert np.isfinite(p1).all() and np.isfinite(v1).all()
        assert blind.sum() == 9 and (bits(v1[blind]) == bits(v[blind])).all() and (bits(p1[blind]) == bits(v[blind] + p[blind])).all()
        assert (bits(v1[~blind]) != bits(v[~blind])).any(1).all()
        p, v = p1, v1


# -- the fold against the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,consts", [(1, None), (2, None), (65, None), (100, None), (100, (0.05, 0.02, 1e-3))])
def test_exact_difference_lists_are_the_oracles_nbody_step(oracle, n, consts):
    """every slot's vec = p_i - p_n for i = 0 .. n - 1 in index order (stride = n): the restated G2-G3 is update_instance_nbody"""
    pos, vel = oracle.init_state(n, 1000 + n)
    rel = np.zeros((n, n, 4), F)
    rel[:, :, :3] = pos[None, :, :] - pos[:, None, :]
    kw = {} if consts is None else dict(dt=F(consts[0]), g=F(consts[1]), bias=F(consts[2]))
    p, v = L.nbody_located_step(pos, vel, np.full(n, n, np.uint32), rel, **kw)
    okw = {} if consts is None else dict(dt=consts[0], g=consts[1], bias=consts[2])
    want_p, want_v = oracle.step_range(pos, vel, 0, n, **okw)
    assert (bits(p) == bits(want_p)).all() and (bits(v) == bits(want_v)).all()
    if n >= 65:   # a subset, and a stride below the count (the clamp): the fold stops at the stride
        ps, vs = L.nbody_located_step(pos, vel, np.full(7, n, np.uint32), rel[5:12], first=5, **kw)
        assert (bits(ps) == bits(want_p[5:12])).all() and (bits(vs) == bits(want_v[5:12])).all()
        pc, vc = L.nbody_located_step(pos, vel, np.full(n, n, np.uint32), rel[:, :10], **kw)
        pw, vw = L.nbody_located_step(pos, vel, np.full(n, 10, np.uint32), rel, **kw)
        assert (bits(pc) == bits(pw)).all() and (bits(vc) == bits(vw)).all() and (bits(vc) != bits(want_v)).any()


# -- the rule's corners ----------------------------------------------------------------------------------------------------------------------
def small_case(oracle):
    cp = R.eye_constant(oracle, 8)
    ids = np.array([3, 3, 7, NONE, 3, 7, 3, 0x80000001], np.uint32)
    depth = np.array([0.75, 0.5, 0.625, 1.0, 0.5, 0.625, 0.5, 0.5], F)
    return cp, ids, depth, np.array([1.0, 2.0, 0.0], F)


def test_l1_takes_the_lowest_column_at_which_the_member_is_nearest(oracle):
    cp, ids, depth, direction = small_case(oracle)
    count, sids, sdepth, _ = S.seen(ids, depth)
    assert count == 3 and (sids[:3] == [3, 7, 0x80000001]).all()
    col, rel = L.located(ids, depth, count, sids, sdepth, direction, UP, cp)
    assert (col == [1, 2, 7, NONE, NONE, NONE, NONE, NONE]).all()         # body 3: nearest at columns 1, 4 and 6 -- not column 0, its first
    assert (bits(rel[3:]) == 0).all() and (rel[:3, 3] > 0).all()            # L5: four +0 words
    assert bits(rel[0, 3]) == bits(rel[2, 3]) and rel[0, 0] != rel[2, 0]    # one depth, one range; another column, another bearing
    f, s = L.axes(direction[None], UP)
    for k in range(3):                                                      # the estimate lies in the plane of f and s: no up component
        assert rel[k, 2] == 0 and abs(float(rel[k, :3] @ f[0]) - float(rel[k, 3])) < 1e-5 * float(rel[k, 3])


def test_a_list_that_is_not_of_its_row(oracle):
    cp, ids, depth, direction = small_case(oracle)
    # member 5 is nowhere in the row, member 7 is there but never at this depth, NB_EYES_NONE is no member, member 3 fits
    sids = np.array([3, 5, 7, NONE, 9, 9, 9, 9], np.uint32)
    sdepth = np.array([0.5, 0.5, 0.5, 1.0, 0.5, 0.5, 0.5, 0.5], F)
    col, rel = L.located(ids, depth, 4, sids, sdepth, direction, UP, cp)
    assert (col == [1, NONE, NONE, NONE, NONE, NONE, NONE, NONE]).all() and (bits(rel[1:]) == 0).all() and rel[0, 3] > 0
    col9, rel9 = L.located(ids, depth, 99, sids, sdepth, direction, UP, cp)   # a count above the width is the width
    assert (col9 == col).all() and (bits(rel9) == bits(rel)).all()
    col0, rel0 = L.located(ids, depth, 0, sids, sdepth, direction, UP, cp)
    assert (col0 == NONE).all() and (bits(rel0) == 0).all()


def bad_constants(oracle):
    good = np.ascontiguousarray(R.eye_constant(oracle, 64), F).reshape(16)
    out = {}
    for what, index, value in (("cp16[11] must be -1", 11, 1.0), ("cp16[15] must be 0", 15, 1.0), ("cp16[0] must not be 0", 0, 0.0),
                               ("cp16[14] must not be 0", 14, 0.0), ("cp16[4] must be 0", 4, 0.5), ("cp16[9] must be 0", 9, np.nan)):
        cp = good.copy()
        cp[index] = value
        out[(what, index, float(value))] = cp
    return good, out


def test_l6_the_restatement_names_the_entry_that_does_not_fit(oracle):
    good, bad = bad_constants(oracle)
    assert L.invertible(good) is None
    neg0 = good.copy()
    neg0[[1, 15]] = F(-0.0)
    assert L.invertible(neg0) is None                                       # -0 is zero
    for (what, index, _), cp in bad.items():
        assert L.invertible(cp) == index, what
    assert L.invertible(R.lattice_camera()) == 11                           # an orthographic caller camera: rows yes, located no


def test_l6_refusals_come_before_the_device(nb, oracle):
    from nenbody_amd import _lib

    lib = _lib.load()
    good, bad = bad_constants(oracle)
    up = UP.copy()
    a = [0x100000 * (i + 1) for i in range(9)]          # 16-byte aligned, never dereferenced: the checks come first

    def rc(cp, count=2, width=8):
        return lib.nb_seen_located_launch(count, width, a[0], a[1], a[2], a[3], a[4], a[5], a[6], up.ctypes.data, cp.ctypes.data, a[7], a[8], None)

    for (what, _, _), cp in bad.items():
        assert rc(cp) == _lib.NB_ERR_INVALID, what
        msg = _lib.last_error()
        assert msg.startswith("nb_seen_located_launch: cp16 cannot be inverted: " + what), msg
    assert rc(np.ascontiguousarray(R.lattice_camera(), F).reshape(16)) == _lib.NB_ERR_INVALID and "cp16[11] must be -1" in _lib.last_error()
    assert rc(good, count=0) == _lib.NB_OK
    if lib.nb_device_count() == 0:
        assert rc(good) == _lib.NB_ERR_NO_DEVICE        # the same call with a constant that fits gets as far as the device


# -- the entry points ------------------------------------------------------------------------------------------------------------------------
def test_seen_located_launch_validates_before_touching_the_device(nb, oracle):
    from nenbody_amd import _lib

    lib = _lib.load()
    cp = np.ascontiguousarray(R.eye_constant(oracle, 8), F).reshape(16)
    up = UP.copy()
    names = ("ids", "depth", "cnt", "sids", "sdepth", "eyes", "dirs", "col", "rel")
    base = {name: 0x100000 * (i + 1) for i, name in enumerate(names)}     # count = 2, width = 8: rows of 64 bytes, rel of 256

    def rc(count=2, width=8, up_p=up.ctypes.data, cp_p=cp.ctypes.data, **kw):
        p = dict(base, **kw)
        return lib.nb_seen_located_launch(count, width, p["ids"], p["depth"], p["cnt"], p["sids"], p["sdepth"], p["eyes"], p["dirs"], up_p, cp_p,
                                          p["col"], p["rel"], None)

    big = _lib.NB_EYES_MAX_WIDTH + 1
    cases = {f"null {n}": {n: None} for n in names if n != "col"}
    cases.update({
        "null up": dict(up_p=None), "null cp": dict(cp_p=None), "width 0": dict(width=0), "width above the maximum": dict(width=big),
        "misaligned ids": dict(ids=base["ids"] + 2), "misaligned sdepth": dict(sdepth=base["sdepth"] + 1), "misaligned col": dict(col=base["col"] + 2),
        "misaligned rel": dict(rel=base["rel"] + 4), "misaligned dirs": dict(dirs=base["dirs"] + 8), "misaligned eyes": dict(eyes=base["eyes"] + 4),
        "col = rel": dict(col=base["rel"]), "col inside rel": dict(col=base["rel"] + 192), "rel over ids": dict(rel=base["ids"] - 240),
        "col over depth": dict(col=base["depth"] + 60), "rel over cnt": dict(rel=base["cnt"] - 240), "col over sids": dict(col=base["sids"]),
        "rel over sdepth": dict(rel=base["sdepth"] + 48), "col over eyes": dict(col=base["eyes"] + 28), "rel over dirs": dict(rel=base["dirs"] + 16),
    })
    for what, kw in cases.items():
        assert rc(**kw) == _lib.NB_ERR_INVALID, what
        assert _lib.last_error().startswith("nb_seen_located_launch: "), what
    assert "alias" in (rc(col=base["rel"]) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "NB_EYES_MAX_WIDTH" in (rc(width=0) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "16-byte" in (rc(rel=base["rel"] + 4) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "4-byte" in (rc(col=base["col"] + 2) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert rc(count=0) == _lib.NB_OK
    assert lib.nb_abi_version() == 2                       # the change only adds symbols
    if lib.nb_device_count() == 0:
        for kw in (dict(), dict(col=None), dict(col=base["rel"] + 256), dict(rel=base["ids"] + 64), dict(width=_lib.NB_EYES_MAX_WIDTH, count=1),
                   dict(width=1, count=1)):
            assert rc(**kw) == _lib.NB_ERR_NO_DEVICE, kw


def test_nbody_located_step_launch_validates_before_touching_the_device(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    pin, vin, pout, vout, cnt, rel = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000

    def rc(n=16, first=4, count=8, pos_in=pin, vel_in=vin, seen_count=cnt, seen_rel=rel, stride=32, pos_out=pout, vel_out=vout):
        return lib.nb_nbody_located_step_launch(None, n, first, count, pos_in, vel_in, seen_count, seen_rel, stride, pos_out, vel_out, None)

    cases = {
        "null pos_in": dict(pos_in=None), "null vel_in": dict(vel_in=None), "null pos_out": dict(pos_out=None), "null vel_out": dict(vel_out=None),
        "null seen_count": dict(seen_count=None), "null seen_rel": dict(seen_rel=None),
        "pos_out = pos_in": dict(pos_out=pin), "vel_out = vel_in": dict(vel_out=vin),
        "stride 0": dict(stride=0), "count 0": dict(count=0), "range past the set": dict(first=10, count=8),
        "misaligned seen_count": dict(seen_count=cnt + 2), "misaligned seen_rel": dict(seen_rel=rel + 4), "misaligned pos_in": dict(pos_in=pin + 8),
        "pos_out over seen_count": dict(seen_count=pout + 4 * 16), "pos_out over seen_rel": dict(seen_rel=pout + 4 * 16 - 8 * 32 * 16 + 16),
        "vel_out over seen_count": dict(seen_count=vout + 12 * 16 - 4), "vel_out over seen_rel": dict(seen_rel=vout + 8 * 16),
    }
    for what, kw in cases.items():
        assert rc(**kw) == _lib.NB_ERR_INVALID, what
        assert _lib.last_error().startswith("nb_nbody_located_step_launch: "), what
    assert "lists" in (rc(seen_rel=vout + 8 * 16) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "stride" in (rc(stride=0) == _lib.NB_ERR_INVALID and _lib.last_error())
    if lib.nb_device_count() == 0:
        # the records the launch does not write may hold the lists: only [first, first + count) is an output
        for kw in (dict(), dict(seen_count=pout), dict(seen_rel=vout + 12 * 16), dict(stride=1), dict(first=0, count=16)):
            assert rc(**kw) == _lib.NB_ERR_NO_DEVICE, kw


def test_the_context_entries_reject_a_null_context(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    buf = np.zeros(64, F)
    p = buf.ctypes.data
    assert lib.nb_eyes_located(None, 0, 1, p, p, 8, 0, p, None, None, None, None, None) == _lib.NB_ERR_INVALID
    assert "nb_eyes_located: ctx is null" in _lib.last_error()
    assert lib.nb_step_nbody_located(None, 1, p, p, 1024, 0) == _lib.NB_ERR_INVALID
    assert "nb_step_nbody_located: ctx is null" in _lib.last_error()


def test_header_binding_and_library_agree(nb):
    from nenbody_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nenbody.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == c_args and hasattr(lib, name), name
    for name in ("located", "step_nbody_located", "step_nbody_located_n"):
        assert callable(getattr(nb.Scene, name))
    assert int(re.search(r"#define NB_ABI_VERSION (\d+)", header).group(1)) == 2


def test_the_rust_shim_declares_the_located_entry_points():
    """integration/rust/scene.rs is text (no Rust toolchain here): the context's located symbols are declared in its extern block with
    the header's argument counts, and Scene has located / step_nbody_located"""
    text = open(os.path.join(ROOT, "integration", "rust", "scene.rs")).read()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nenbody.h")).read(), flags=re.S)
    for name in ("nb_eyes_located", "nb_step_nbody_located"):
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        m = re.search(r"fn %s\s*\(([^)]*)\)\s*->\s*c_int;" % name, text)
        assert m, name
        assert m.group(1).strip().rstrip(",").count(",") + 1 == c_args, name
    for method in ("pub fn located(", "pub fn step_nbody_located(", "pub struct Located"):
        assert method in text, method


def build_exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(ROOT, "nenbody_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "located_check.cpp"), "-o", EXE, "-L", libdir, "-lnenbody_hip",
                    f"-Wl,-rpath,{libdir}"], check=True)


def test_cpp_located_host_compiles_and_refuses_to_run_without_a_gpu(nb, tmp_path):
    build_exe()
    from nenbody_amd import _lib

    have_device = _lib.load().nb_device_count() > 0
    r = subprocess.run([EXE, "16", "64", str(tmp_path / "out.bin")], capture_output=True, text=True)
    if have_device:
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 10 and "no HIP device" in r.stderr     # NB_ERR_NO_DEVICE surfaced as nenbody::Error
