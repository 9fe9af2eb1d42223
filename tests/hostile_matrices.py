"""A corpus of arbitrary caller matrices for the eye rows and the scene camera's frame (DESIGN.md sections 10 - 11.1).

TEST INFRASTRUCTURE, no tests in it.  The launch forms take any 16 floats per model matrix and per camera; every other test feeds
them oracle.instances -- a translation times a rotation about z -- and the oracle's cameras.  This module draws seeded matrices off
that family, so that tests/test_hostile_matrices_cpu.py (the host-compiled device functions) and tests/test_gpu_hostile_matrices.py
(the kernels) can be compared with the numpy restatements of the rule on products that overflow, go subnormal, meet an infinity or
a NaN, on w <= 0, on depths that clamp to +0 or are rejected at 1, on ends that sit exactly on a column centre, and on exact ties.

A case is a dict: name, inst (n, 4, 4) float32 ([k] = column k), cls (n,) the class of each body, skin ((5, 7, 4) float32 or None)
and, for the eyes, cams (6, 4, 4), first = 3, width, see_self, views; for the frames, cam (4, 4), extent (W, H).  The body index
picks the class (j % 9), so that the classes interleave within a wave.  expected(view, case) is the restatement's answer, computed
once per process and shared; stats(view, case) what the restatement counted on the way.
"""
import numpy as np

import eyes_colour_restatement as K
import eyes_msaa_restatement as M
import eyes_restatement as R
import frame_msaa_restatement as FM
import frame_restatement as FR

F = np.float32
CLASSES = ("affine", "projective", "huge", "tiny", "inf", "nan", "degenerate", "half", "duplicate")
DRAWING = ("affine", "projective", "huge", "half")          # the classes that put triangles on the screen
N = 300                                                     # two 256-lane passes per eye, two blocks of the frame's edges kernel, the last ragged
FIRST, EYES = 3, 6
VIEWS = ("eyes", "eyes_colour", "eyes_msaa", "frame", "frame_msaa")
MARK = 7                                                    # what the GPU tests prefill their outputs with


def random_skin(tw=7, th=5, seed=11):
    """linear texels in [0, 1) but for one above 1 and one below 0, as the existing tests' random skin"""
    skin = np.random.default_rng(seed).uniform(0, 1, (th, tw, 4)).astype(F)
    skin[0, 0, 0], skin[th - 1, tw - 1, 1] = 1.5, -0.25
    return skin


def matrices(n, seed, half):
    """n model matrices for a scene of half-extents half = (sx, sy, sz) about the origin: (inst (n, 4, 4) with [k] = column k,
    cls (n,) indices into CLASSES).  A vertex is M (-1, -1, 0, 1), M (1, 0, 0, 1), M (-1, 1, 0, 1): columns 0, 1 and 3 matter,
    column 2 only through its products by zero."""
    rng = np.random.default_rng(seed)
    half = np.asarray(half, np.float64)
    cls = np.arange(n) % len(CLASSES)
    A = np.zeros((n, 4, 4), np.float64)                      # A[j, r, c]: row r, column c
    A[:, :3, :3] = rng.standard_normal((n, 3, 3)) * np.exp2(rng.integers(-7, 0, (n, 1, 1))) * half[None, :, None]
    A[:, :3, 3] = rng.uniform(-1, 1, (n, 3)) * half
    A[:, 3, 3] = 1
    for j in np.nonzero(cls == CLASSES.index("projective"))[0]:
        A[j, 3, :3] = rng.uniform(-0.75, 0.75, 3)            # w = -+p0 -+p1 + 1: mostly positive, now and then <= 0
    for j in np.nonzero(cls == CLASSES.index("huge"))[0]:
        A[j] *= np.exp2(rng.integers(20, 121))               # homogeneous: the same triangle until a product overflows
    for j in np.nonzero(cls == CLASSES.index("tiny"))[0]:
        A[j] *= np.exp2(-float(rng.integers(100, 149)))      # products subnormal or zero
    for j in np.nonzero(cls == CLASSES.index("inf"))[0]:
        A[j, rng.integers(4), rng.integers(4)] = rng.choice([-np.inf, np.inf])
    for j in np.nonzero(cls == CLASSES.index("nan"))[0]:
        A[j, rng.integers(4), rng.integers(4)] = np.nan
    A[cls == CLASSES.index("degenerate"), :, :2] = 0         # the three vertices coincide
    for j in np.nonzero(cls == CLASSES.index("half"))[0]:
        # column 0 half-integers, columns 1 and 3 integers: every vertex (-+c0 -+c1 + c3) has half-integer x and y -- a column or
        # pixel centre in a camera that maps the world to pixels --; planar, z one of a few values a pushed depth turns into 0, 0.5, 1
        for r in range(2):
            a = max(1, int(half[r]) // 2)
            A[j, r, 0] = rng.integers(-a, a) + 0.5
            A[j, r, 1] = rng.integers(-a, a + 1)
            A[j, r, 3] = rng.integers(-int(half[r]), int(half[r]) + 1)
        A[j, 2, :3] = 0
        A[j, 2, 3] = rng.choice([-1.0, -0.0, 0.0, 0.0, 0.5, 1.0])
        A[j, 3] = (0, 0, 0, 1)
    draws = [CLASSES.index(c) for c in DRAWING]
    for j in np.nonzero(cls == CLASSES.index("duplicate"))[0]:
        src = j - len(CLASSES) + 1 + draws[(j // len(CLASSES)) % len(draws)]   # an earlier drawing body of this group of nine
        A[j] = A[src]                                        # bit for bit: every key ties, the lower index holds the pixel
    with np.errstate(all="ignore"):
        inst = np.ascontiguousarray(A.transpose(0, 2, 1)).astype(F)
    for j in np.nonzero(cls == CLASSES.index("duplicate"))[0]:
        src = j - len(CLASSES) + 1 + draws[(j // len(CLASSES)) % len(draws)]
        assert (inst[j].view(np.uint32) == inst[src].view(np.uint32)).all() or np.isnan(inst[src]).any()
    return inst, cls


def duplicate_source(j):
    """the body that body j (of class "duplicate") copies"""
    draws = [CLASSES.index(c) for c in DRAWING]
    return j - len(CLASSES) + 1 + draws[(j // len(CLASSES)) % len(draws)]


# -- cameras ---------------------------------------------------------------------------------------------------------------------------
def _zero_row(c, row):
    c = c.copy()
    c[:, row] = 0                                            # c[k, r]: column k, row r
    return c


def eye_cameras(oracle, width, seed):
    """six cameras for a row of `width` columns over a scene of half-extents (width / 2, 8, 1): orthographic (x to columns, y / 8,
    depth 0.5), the same with depth 0.5 z + 0.5 (part of the scene at d <= 0, part at d >= 1), a perspective one from outside the
    scene, one from its middle (bodies behind the eye), a random 4 x 4, and the orthographic one with row 1 + seed % 3 zeroed."""
    rng = np.random.default_rng(seed)
    ortho = np.zeros((4, 4), F)
    ortho[0, 0] = F(1) / (F(width) * F(0.5))
    ortho[1, 1] = 0.125
    ortho[3, 2] = 0.5
    ortho[3, 3] = 1
    pushed = ortho.copy()
    pushed[2, 2] = 0.5
    cp = R.eye_constant(oracle, width)
    up = np.array([0, 0, 1], F)
    outside = oracle.cameras(np.array([[0, -(width * 0.5 + 9), 0]], F), np.array([[0, 1, 0]], F), up, cp)[0]
    inside = oracle.cameras(np.array([[0.25, 0.5, 0]], F), np.array([[1, 0.125, 0]], F), up, cp)[0]
    rand = rng.standard_normal((4, 4))
    rand[:3] /= np.array([width * 0.5, 8, 1])[:, None]       # (column k scales world coordinate k)
    return np.stack([ortho, pushed, outside, inside, rand.astype(F), _zero_row(ortho, 1 + seed % 3)]).astype(F)


def frame_camera(oracle, kind, extent, seed):
    """one camera for a W x H frame over a scene of half-extents (W / 2, H / 2, 1): "ortho" (the world in pixels, depth 0.5),
    "pushed" (depth 0.5 z + 0.5), "persp" (FR.camera from above), "random" (4 x 4), "zero_z" and "zero_w" (ortho with row 2 or row 3 zeroed: every depth +-0, every w zero)"""
    W, H = extent
    ortho = FR.ortho_camera(W, H)
    if kind == "ortho":
        return ortho
    if kind == "pushed":
        ortho[2, 2] = 0.5
        return ortho
    if kind == "persp":
        return FR.camera(oracle, [0, 0, 0.625 * W], [0, 0, -1], [0, 1, 0], FR.frame_constant(oracle, extent))
    if kind == "random":
        rand = np.random.default_rng(seed).standard_normal((4, 4))
        rand[:3] /= np.array([W * 0.5, H * 0.5, 1])[:, None]
        return rand.astype(F)
    if kind in ("zero_z", "zero_w"):
        return _zero_row(ortho, 2 if kind == "zero_z" else 3)
    raise KeyError(kind)


# -- the cases -------------------------------------------------------------------------------------------------------------------------
# (width, see_self, skin, bodies, views): the widths around the 64-column round of a wave and the 256-lane pass; the 8-sample eye
# alone at its LDS limit, with few bodies
_EYE_CASES = ((1, False, False, N, VIEWS[:3]), (33, True, True, N, VIEWS[:3]), (64, False, True, N, VIEWS[:3]),
              (65, True, False, N, VIEWS[:3]), (257, False, True, N, VIEWS[:3]), (2048, True, True, 20, VIEWS[2:3]))
# (extent, camera): (128, 3) and (3, 128) make edges longer than 8 + 64 major-axis steps, x-major and y-major
_FRAME_CASES = (((64, 32), "ortho"), ((64, 32), "pushed"), ((64, 32), "persp"), ((64, 32), "random"), ((64, 32), "zero_z"),
                ((33, 7), "pushed"), ((33, 7), "persp"), ((33, 7), "zero_w"), ((1, 1), "ortho"), ((1, 1), "pushed"), ((128, 3), "ortho"),
                ((128, 3), "persp"), ((3, 128), "pushed"), ((3, 128), "zero_z"))
_cache = {}


def eye_cases(oracle):
    if "eye_cases" not in _cache:
        out = []
        for i, (width, see_self, skin, n, views) in enumerate(_EYE_CASES):
            inst, cls = matrices(n, 100 + i, (width * 0.5, 8, 1))
            out.append(dict(name=f"W{width}-self{int(see_self)}", inst=inst, cls=cls, cams=eye_cameras(oracle, width, 200 + i), first=FIRST,
                            width=width, see_self=see_self, skin=random_skin() if skin else None, views=views))
        _cache["eye_cases"] = out
    return _cache["eye_cases"]


def frame_cases(oracle):
    if "frame_cases" not in _cache:
        out = []
        for i, (extent, kind) in enumerate(_FRAME_CASES):
            inst, cls = matrices(N, 300 + i, (extent[0] * 0.5, extent[1] * 0.5, 1))
            out.append(dict(name=f"{extent[0]}x{extent[1]}-{kind}", inst=inst, cls=cls, cam=frame_camera(oracle, kind, extent, 400 + i),
                            extent=extent, skin=random_skin() if i % 2 else None, views=VIEWS[3:]))
        _cache["frame_cases"] = out
    return _cache["frame_cases"]


EYE_NAMES = tuple(f"W{w}-self{int(s)}" for w, s, _, _, _ in _EYE_CASES)
EYE_NAMES_ONE = tuple(f"W{w}-self{int(s)}" for w, s, _, _, v in _EYE_CASES if "eyes" in v)
FRAME_NAMES = tuple(f"{e[0]}x{e[1]}-{k}" for e, k in _FRAME_CASES)


def case(oracle, name):
    for c in eye_cases(oracle) + frame_cases(oracle):
        if c["name"] == name:
            return c
    raise KeyError(name)


def restate(view, c, inst=None, stats=None):
    """the restatement of `view` on case c (on other matrices where inst is given), not cached"""
    inst = c["inst"] if inst is None else inst
    if view == "eyes":
        return R.eyes(c["cams"], inst, c["first"], c["width"], c["see_self"], stats=stats)
    if view == "eyes_colour":
        return K.colour(c["cams"], inst, c["first"], c["width"], c["see_self"], c["skin"], stats=stats)
    if view == "eyes_msaa":
        return M.msaa(c["cams"], inst, c["first"], c["width"], c["see_self"], c["skin"], stats=stats)
    if view == "frame":
        return FR.frame(c["cam"], inst, *c["extent"], skin=c["skin"], stats=stats)
    if view == "frame_msaa":
        return FM.frame_msaa(c["cam"], inst, *c["extent"], skin=c["skin"], stats=stats)
    raise KeyError(view)


def expected(view, c):
    """the restatement's outputs of `view` on case c, computed once and left unchanged (read-only arrays)"""
    key = (view, c["name"])
    if key not in _cache:
        st = {}
        out = restate(view, c, stats=st)
        for a in out:
            a.setflags(write=False)
        _cache[key] = (out, st)
    return _cache[key][0]


def stats(view, c):
    expected(view, c)
    return _cache[(view, c["name"])][1]


def words(a):
    """an output as uint32 words"""
    return np.ascontiguousarray(a).view(np.uint32)
