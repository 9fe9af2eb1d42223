"""The cases on which the eye rows and the frame are held to the geometric reference (tests/vision_reference.py): small, seeded, the
smallest shapes at which the kernels can still go wrong.  The CPU file (test_vision_reference_cpu.py) checks the caps and the
coverage conditions on the reference alone and holds the restatements to it; the GPU file (test_gpu_vision_reference.py) holds the
device to it and, on the same cases, bit for bit to the restatements.  References are cached per case, for at most 48 eyes.

Caps per case (checked on the CPU): undecided cells at most 5 % of the cells any body touches; at least 200 decided covered cells
(the 1 x 1, 3 x 2 and W <= 3 cases: at least one).  A cell whose COLOUR is not compared counts as undecided as well -- the winner's
second edge within reach, a texel index, an extrapolated centre, a colour bound above 1 / 32 --: at most 5 % of the touched cells
(through 8 samples a cell is a sample), and at least 200 columns whose colour is compared.  One case cannot meet the colour cap
and says so: at positions * 30 every body is thinner than a column and lies 1000 units and more away, where the two edges a column
cuts are 0 .. 7 ulp of a binary32 depth apart, within the rounding of the rule's own last steps: which edge shades the column is
undecided on about half of its cells (55 %, through 8 samples 53 %).  That case holds ids, depth (within the two edges' span where
they are in reach), the seen sets and the caps on those, and the colour of the cells where the edges are apart (at least 50).
Over the list: every edge index wins, each of the four clip planes cuts a
winning edge, a winning edge has end w more than 10 % apart, a column shows a body that hides a farther one, and the frame has
x-major and y-major winning edges."""
import os

import numpy as np

import vision_reference as V

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_EYES = 48
MSAA_EYES = 16          # the 8-sample reference costs eight times a row's: fewer eyes, the same cases
UP = (0.0, 0.0, 1.0)
UP2 = (0.25, -0.125, 1.0)
CAPS = dict(undecided_share=0.05, decided_covered=200, colour_compared=200, colour_compared_exempt=50)


def _eye(n, width, seed, scale=1.0, lift=False, near=1.0, far=10000.0, see_self=False, up=UP, skin=False, eyes=MAX_EYES):
    return dict(n=n, width=width, seed=seed, scale=scale, lift=lift, near=near, far=far, see_self=see_self, up=up, skin=skin,
                eyes=min(n, eyes), exempt=width <= 3, colour_exempt=scale >= 30.0)      # (colour_exempt: see the module's docstring)


# name: init_state(n, seed) with positions * scale; lift: z within +-0.05 and vz within +-0.002 from default_rng(seed); skin: the
# reference's (tests/golden/skin_rgba8.npy), else white
EYE_CASES = {
    "n2_w1024_close": _eye(2, 1024, 54, 0.1),
    "n3_w1024_close_near_self": _eye(3, 1024, 3, 0.1, near=0.5, see_self=True),
    "n100_w1": _eye(100, 1, 1105),
    "n100_w3": _eye(100, 3, 1100, skin=True),
    "n100_w64": _eye(100, 64, 1100),
    "n257_w65_skin": _eye(257, 65, 1257, skin=True),
    "n100_w1024_skin": _eye(100, 1024, 1100, skin=True),
    "n257_w1024_close": _eye(257, 1024, 1257, 0.1),
    "n100_w1024_close_near_self_skin": _eye(100, 1024, 1100, 0.1, near=0.5, see_self=True, skin=True),
    "n100_w256_far_away": _eye(100, 256, 1100, 30.0),
    "n257_w1024_lifted_skin": _eye(257, 1024, 1257, lift=True, skin=True),
    "n100_w1024_lifted_close_up2": _eye(100, 1024, 1100, 0.1, lift=True, up=UP2),
    "n257_w1024_far50": _eye(257, 1024, 1257, far=50.0),
    "n100_w65_lifted_far50_skin": _eye(100, 65, 1100, 0.1, lift=True, far=50.0, skin=True),
    "n100_w4096_close_8eyes": _eye(100, 4096, 1100, 0.1, eyes=8),
}
MSAA_MAX_WIDTH = 2048      # NB_EYES_MSAA_MAX_WIDTH: an 8-sample row of more columns does not fit a workgroup's LDS, the entry refuses it


def _frame(eye, direction, up, extent, skin=False, exempt=False):
    return dict(eye=eye, direction=direction, up=up, extent=extent, skin=skin, exempt=exempt, colour_exempt=False)


FRAME_N, FRAME_SEED, FRAME_SCALE = 40, 1040, 0.1
FRAME_CASES = {
    "down_64x48": _frame((0, 0, 14), (0, 0, -1), (1, 0, 0), (64, 48)),
    "oblique_96x64_skin": _frame((-12, 1, 6), (1, 0.1, -0.5), (0, 0, 1), (96, 64), skin=True),
    "low_96x64": _frame((-2, 0, 0.5), (1, 0.2, -0.1), (0, 0, 1), (96, 64)),          # among the bodies: the near plane cuts outlines
    "down_1x1": _frame((0, 0, 14), (0, 0, -1), (1, 0, 0), (1, 1), exempt=True),
    "down_3x2_skin": _frame((0, 0, 14), (0, 0, -1), (1, 0, 0), (3, 2), skin=True, exempt=True),
}


def golden_skin():
    """the reference's skin, (20, 20, 4) uint8 sRGB: what Scene.set_skin takes"""
    return np.load(os.path.join(GOLDEN, "skin_rgba8.npy"))


def skin_of(case):
    """(what Scene.set_skin takes, the binary64 linear texels the reference shades with); (None, None): white"""
    return (golden_skin(), V.srgb8_to_linear(golden_skin())) if case["skin"] else (None, None)


def eye_state(oracle, name):
    c = EYE_CASES[name]
    pos, vel = oracle.init_state(c["n"], c["seed"])
    pos = (pos * F(c["scale"])).astype(F)
    if c["lift"]:
        rng = np.random.default_rng(c["seed"])
        pos[:, 2] = rng.uniform(-0.05, 0.05, c["n"]).astype(F)
        vel[:, 2] = rng.uniform(-0.002, 0.002, c["n"]).astype(F)
    return pos, vel


def eye_lens(name):
    """(vertical field of view in degrees, aspect) of a row of the case's width, as the reference application forms them: the 90
    degrees divided by the aspect ratio W / 1"""
    w = F(EYE_CASES[name]["width"])
    return float(F(90.0) / w), float(w / F(1.0))


def eye_constant(module, name):
    """the case's camera constant from `module` (the oracle or the product package): (4, 4), [k] = column k"""
    c = EYE_CASES[name]
    return module.camera_constant(*eye_lens(name), c["near"], c["far"])


_cache = {}


def eyes_of(name, samples=False):
    """how many eyes, 0 .. count - 1, the case's reference is computed for"""
    return min(EYE_CASES[name]["eyes"], MSAA_EYES) if samples else EYE_CASES[name]["eyes"]


def eye_reference(oracle, name, samples=False):
    """the reference rows of the case's eyes 0 .. eyes_of(name, samples) - 1, cached"""
    key = (name, samples)
    if key not in _cache:
        c = EYE_CASES[name]
        pos, vel = eye_state(oracle, name)
        _cache[key] = V.eye_rows(pos, vel, np.arange(eyes_of(name, samples)), c["width"], c["up"], *eye_lens(name), c["near"], c["far"], c["see_self"],
                                 skin_of(c)[1], samples)
    return _cache[key]


def frame_state(oracle):
    pos, vel = oracle.init_state(FRAME_N, FRAME_SEED)
    return (pos * F(FRAME_SCALE)).astype(F), vel


def frame_lens(name):
    w, h = FRAME_CASES[name]["extent"]
    a = F(w) / F(h)
    return float(F(90.0) / a), float(a)


def frame_constant(module, name):
    return module.camera_constant(*frame_lens(name), 1.0, 10000.0)


def frame_reference(oracle, name):
    key = ("frame", name)
    if key not in _cache:
        c = FRAME_CASES[name]
        pos, vel = frame_state(oracle)
        _cache[key] = V.frame(pos, vel, np.array(c["eye"], F), np.array(c["direction"], F), np.array(c["up"], F), *frame_lens(name),
                              c["extent"], skin=skin_of(c)[1])
    return _cache[key]


def shares(ref):
    """(cells a body touches, undecided ones among them, decided covered cells) of a reference"""
    touched = int(ref.touched.sum())
    return touched, int((ref.und & ref.touched).sum()), int((~ref.und & (ref.ids != V.NONE)).sum())


def colour_shares(ref):
    """(touched cells whose colour is not compared -- undecided ones among them --, touched columns or pixels, those of them whose
    colour is compared) of a reference; a cell is a sample where the reference has samples"""
    columns = ref.touched.any(-1) if ref.touched.ndim > ref.und_rgba.ndim else ref.touched
    return int((ref.und_colour & ref.touched).sum()), int(columns.sum()), int((columns & ~ref.und_rgba).sum())
