"""The cases on which the scene batches' policy and score are held to their binary64 references (tests/policy_reference.py,
tests/score_reference.py): small, seeded, the smallest shapes at which the kernels can still go wrong.  The CPU file
(test_policy_score_reference_cpu.py) checks the caps on the references alone, holds the restatements to them and shows the control
arms rejected; the GPU file (test_gpu_policy_score_reference.py) holds the device to them and, on the same cases, bit for bit to
the restatements.  References are cached per case.

TEST INFRASTRUCTURE.  A fixed case is a row of FIXED: B scenes of n bodies drawn by state() -- positions uniform in +-scale, planar,
3-D, lifted off the plane (z within +-0.05) or clustered (half of the bodies share positions), velocities uniform in +-speed, with an
eighth of them exactly zero (`zeros`) or body 1 of every scene moving along `up` (`along`) where the row says so --, an `up`, a lens
(near, far), a row of W columns, a policy shape (F, H), a policy per scene or one for all, a limit, and `gain`: the scale of hidden
unit 0's input weights, chosen per case so that a blind eye's unit is off and a seeing eye's on, and that seeing eyes lie on both sides
of the limit (the CPU file asserts it).  `eyes`: the reference is computed for eyes 0 .. eyes - 1 of every scene; every eye where
n <= 129, 48 of n = 257.

case(i), i = 0 .. RANDOM_CASES - 1 (NB_RANDOM_CASES widens the family), draws from numpy's default_rng(25000 + i): n, W, B, `up`, scale
and kind from the lists of scenes_random_cases._vision_case, and F (a divisor of W), H, the limit, the lens and k in {1, 2, 3}.  A
failure prints the case's line, and `case(i)` gives the same arrays again."""
import os

import numpy as np

import policy_reference as PR
import score_cases
import score_reference as QR
from scenes_random_cases import VISION_KINDS, VISION_SCALES, VISION_SIZES, VISION_UPS, VISION_WIDTHS

F32 = np.float32
UP, TILTED = (0.0, 0.0, 1.0), (0.6, 0.0, 0.8)
LENSES = [(1.0, 10000.0), (0.5, 10000.0), (1.0, 50.0)]
LIMITS = [0.0, 0.5, 1.0, float("inf")]
HIDDEN = [1, 2, 33, 63, 64]
MAX_FEATURES, MAX_HIDDEN = 256, 64
DT = F32(0.1)
ALL_EYES, FEW_EYES = 129, 48
RANDOM_CASES = int(os.environ.get("NB_RANDOM_CASES", "24"))
CAPS = dict(uncompared_share=0.05, compared_seeing=20, maybe_pairs=2, maybe_share=0.001)


def pack(w1, b1, w2, b2):
    """one policy in the layout of include/nenbody.h: w1[f H + j], b1[j], w2[k H + j], b2[k]"""
    return np.concatenate([np.asarray(a, F32).reshape(-1) for a in (w1, b1, w2, b2)])


def policies(features, hidden, count, seed, gain=1.0, out_gain=1.0, scale=(1.0, 1.0, 1.0)):
    """(count, floats) float32.  Unit 0 of every policy: b1 = -2^-7 and w1 in [0.5, 1.5) gain / F, so it is off for an eye that sees
    nothing and on for one whose bins are near enough; its w2 has magnitude in [1, 2) out_gain.  The other units: w1 in
    [-1, 1) gain / F, b1 in [-0.02, 0.02), w2 in [-2, 2) out_gain / H; b2 in [-0.01, 0.01).  `scale`: a power of two on the first
    layer's floats, one on w2 and one on b2."""
    rng = np.random.default_rng([seed, features, hidden])
    out = []
    for _ in range(count):
        w1 = rng.uniform(-1, 1, (features, hidden)) * gain / features
        w1[:, 0] = rng.uniform(0.5, 1.5, features) * gain / features
        b1 = rng.uniform(-0.02, 0.02, hidden)
        b1[0] = -2.0 ** -7
        w2 = rng.uniform(-2, 2, (2, hidden)) * out_gain / hidden
        w2[:, 0] = rng.uniform(1, 2, 2) * rng.choice([-1, 1], 2) * out_gain
        b2 = rng.uniform(-0.01, 0.01, 2)
        out.append(pack(F32(w1) * F32(scale[0]), F32(b1) * F32(scale[0]), F32(w2) * F32(scale[1]), F32(b2) * F32(scale[2])))
    return np.stack(out)


def state(rng, n, kind, scale, speed, up, zeros=False, along=False):
    pos = (rng.uniform(-1, 1, (n, 3)) * scale).astype(F32)
    vel = (rng.uniform(-1, 1, (n, 3)) * speed).astype(F32)
    if kind == "planar":
        pos[:, 2] = 0
        vel[:, 2] = 0
    elif kind == "lifted":
        pos[:, 2] = rng.uniform(-0.05, 0.05, n).astype(F32)
        vel[:, 2] = (rng.uniform(-0.02, 0.02, n) * speed).astype(F32)
    elif kind == "clustered":
        pos[rng.integers(0, n, n // 2)] = pos[rng.integers(0, n, n // 2)]
    else:
        assert kind == "3-D", kind
    if zeros:
        vel[rng.choice(n, max(1, n // 8), replace=False)] = 0
    if along:
        vel[1] = F32(2.0) * np.array(up, F32)
    return pos, vel


def _fixed(n, scenes, width, features, hidden, kind, scale, up=UP, lens=0, limit=0.5, own=True, gain=1.0, out_gain=1.0, seed=0,
           zeros=False, along=False, weights=(1.0, 1.0, 1.0), exempt=False):
    return dict(n=n, batch=scenes, width=width, features=features, hidden=hidden, kind=kind, scale=scale, up=up, lens=LENSES[lens],
                limit=limit, own=own, gain=gain, out_gain=out_gain, seed=seed, zeros=zeros, along=along, weights=weights, exempt=exempt,
                speed=0.1, k=2, eyes=min(n, ALL_EYES if n <= ALL_EYES else FEW_EYES))


# `exempt`: the weights x 2^10 case, where every seeing eye is clipped by construction
FIXED = {
    "planar10_n64_w64_f1_h1": _fixed(64, 2, 64, 1, 1, "planar", 10.0, gain=0.5),
    "planar10_n128_w1024_f64_h64_shared": _fixed(128, 2, 1024, 64, 64, "planar", 10.0, limit=1.0, own=False, gain=1.5),
    "3d3_n129_w63_f9_h33_tilted": _fixed(129, 2, 63, 9, 33, "3-D", 3.0, up=TILTED, gain=4.0),
    "3d10_n100_w200_f25_h2_near05": _fixed(100, 3, 200, 25, 2, "3-D", 10.0, lens=1, limit=1.0, gain=32.0),
    "lifted3_n65_w65_f5_h63_tilted_far50": _fixed(65, 3, 65, 5, 63, "lifted", 3.0, up=TILTED, lens=2, gain=2.0),
    "clustered3_n100_w256_f256_h2_shared": _fixed(100, 2, 256, 256, 2, "clustered", 3.0, limit=1.0, own=False, gain=16.0),
    "3d3_n128_w64_f64_h33_zeros": _fixed(128, 2, 64, 64, 33, "3-D", 3.0, zeros=True, gain=8.0),
    "planar3_n65_w7_f7_h1_along": _fixed(65, 4, 7, 7, 1, "planar", 3.0, along=True, gain=0.6),
    "planar3_n33_w7_f1_h2_limit0": _fixed(33, 4, 7, 1, 2, "planar", 3.0, limit=0.0, gain=2.0),
    "3d3_n33_w63_f63_h64_no_limit": _fixed(33, 4, 63, 63, 64, "3-D", 3.0, limit=float("inf"), gain=4.0, out_gain=0.25),
    "3d3_n33_w200_f25_h33_weights_2m130": _fixed(33, 4, 200, 25, 33, "3-D", 3.0, gain=4.0, weights=(2.0 ** -130,) * 3),
    "3d3_n33_w200_f25_h33_first_layer_2m130": _fixed(33, 4, 200, 25, 33, "3-D", 3.0, gain=4.0, weights=(2.0 ** -130, 2.0 ** 126, 1.0)),
    "lifted3_n100_w65_f5_h2_weights_2p10": _fixed(100, 2, 65, 5, 2, "lifted", 3.0, gain=2.0, weights=(2.0 ** 10,) * 3, exempt=True),
    "3d10_n257_w1024_f1_h64_far50_48eyes": _fixed(257, 1, 1024, 1, 64, "3-D", 10.0, lens=2, gain=2.0),
    "lifted10_n129_w1024_f256_h63_tilted": _fixed(129, 1, 1024, 256, 63, "lifted", 10.0, up=TILTED, gain=8.0, seed=1),
    "planar10_n127_w200_f200_h1_tilted_far50": _fixed(127, 2, 200, 200, 1, "planar", 10.0, up=TILTED, lens=2, gain=8.0),
    "3d3_n129_w256_f1_h2_zeros_along_near05": _fixed(129, 2, 256, 1, 2, "3-D", 3.0, lens=1, zeros=True, along=True, limit=1.0, gain=2.0),
}


def _build(name, c, rng, states=None):
    if states is None:
        states = [state(rng, c["n"], c["kind"], c["scale"], c["speed"], c["up"], c["zeros"], c["along"]) for _ in range(c["batch"])]
    out = dict(c, name=name, pos=np.stack([s[0] for s in states]), vel=np.stack([s[1] for s in states]), up=np.array(c["up"], F32))
    out["policies"] = policies(c["features"], c["hidden"], c["batch"] if c["own"] else 1, c["seed"] + 7, c["gain"], c["out_gain"], c["weights"])
    for a in ("pos", "vel", "policies"):
        out[a].setflags(write=False)
    return out


_cases, _refs = {}, {}


def fixed(name):
    """the fixed case `name`: FIXED's row with pos, vel (B, n, 3), up, policies (P, floats) and its name"""
    if name not in _cases:
        c = FIXED[name]
        _cases[name] = _build(name, c, np.random.default_rng([1700, list(FIXED).index(name), c["seed"]]))
    return _cases[name]


def _divisors(width):
    return [f for f in range(1, min(width, MAX_FEATURES) + 1) if width % f == 0]


def case(i):
    """random problem i; its `line` reproduces it"""
    key = ("random", i)
    if key not in _cases:
        rng = np.random.default_rng(25000 + i)
        n = int(rng.choice(VISION_SIZES))
        width = int(rng.choice(VISION_WIDTHS))
        scenes = int(rng.choice([1, 2, 4]))
        k = int(rng.choice([1, 2, 3]))
        up = VISION_UPS[int(rng.integers(0, 2))]
        features = int(rng.choice(_divisors(width)))
        hidden = int(rng.choice(HIDDEN))
        limit = float(rng.choice(LIMITS))
        lens = int(rng.integers(0, len(LENSES)))
        states, kinds = [], []
        for _ in range(scenes):
            scale = float(rng.choice(VISION_SCALES))
            kind = VISION_KINDS[int(rng.integers(0, len(VISION_KINDS)))]
            speed = float(rng.choice([1e-3, 0.1, 2.0]))
            states.append(state(rng, n, {"zero velocities": "3-D"}.get(kind, kind), scale, speed, up, zeros=kind == "zero velocities"))
            kinds.append(f"{kind} +-{scale:g}")
        own = bool(rng.integers(0, 2))
        c = dict(n=n, batch=scenes, width=width, features=features, hidden=hidden, up=up, lens=LENSES[lens], limit=limit, own=own, gain=4.0,
                 out_gain=0.25 if limit == float("inf") else 1.0, seed=i, weights=(1.0, 1.0, 1.0), exempt=False, k=k, kinds=kinds,
                 eyes=min(n, ALL_EYES if n <= ALL_EYES else FEW_EYES))
        c["line"] = (f"case({i}): n={n} W={width} B={scenes} k={k} up={up} F={features} H={hidden} limit={limit} lens={LENSES[lens]} "
                     f"policies={'own' if own else 'shared'} scenes: {kinds}")
        _cases[key] = _build(f"random {i}", c, rng, states)
    return _cases[key]


def reference(c):
    """PR.batch of the case's first step for eyes 0 .. c["eyes"] - 1 of every scene, cached"""
    if c["name"] not in _refs:
        _refs[c["name"]] = PR.batch(c["pos"], c["vel"], np.arange(c["eyes"]), c["width"], c["up"], *c["lens"], c["policies"], c["features"],
                                    c["hidden"], c["limit"], DT)
    return _refs[c["name"]]


def camera_constant(module, c):
    """the case's eye constant from `module` (the oracle or the product package): (4, 4), [k] = column k"""
    w = F32(c["width"])
    return module.camera_constant(float(F32(90.0) / w), float(w / F32(1.0)), *c["lens"])


# -- the score ---------------------------------------------------------------------------------------------------------------------------
SCORE_SIZES = (2, 5, 65, 129, 300, 1025)
SCORE_CASES = [(kind, n) for kind in score_cases.KINDS for n in SCORE_SIZES]
ROLLOUTS = ("3d3_n129_w63_f9_h33_tilted", "planar10_n64_w64_f1_h1", "lifted3_n65_w65_f5_h63_tilted_far50")
ROLLOUT_SCORE = dict(radius_sq=F32(2.25), goal=F32([0.5, -0.25, 0.125]))


def score_reference(kind, n):
    """QR.batch of score_cases.make(kind, n) after one snapshot, cached"""
    key = ("score", kind, n)
    if key not in _refs:
        _refs[key] = QR.batch(*score_cases.make(kind, n))
    return _refs[key]


# -- the restatements on these cases (no test in here) -----------------------------------------------------------------------------------
_rows = {}


def restated_rows(oracle, c, see_self=False):
    """per scene the (ids, depth) rows of the case's initial state by the numpy eye rule on the oracle's cameras, built with the case's
    lens and `up`; cached"""
    import eyes_restatement as R

    key = (c["name"], see_self)
    if key not in _rows:
        cp = camera_constant(oracle, c)
        _rows[key] = [R.eyes(oracle.cameras(p, v, c["up"], cp), oracle.instances(p, v), 0, c["width"], see_self, chunk=64)
                      for p, v in zip(c["pos"], c["vel"])]
    return _rows[key]


def restated(oracle, c, steps=1, variant=None, module=None, see_self=False):
    """policy_restatement (or `module`, a mutated copy) chained over `steps` steps as scenes_random_cases.vision_expected chains the
    vision laws: (x, o of the FIRST step, [(positions, velocities) after step 1, 2, ..])"""
    import eyes_restatement as R
    import policy_restatement as P

    P = P if module is None else module
    cp = camera_constant(oracle, c)
    pos, vel, first, states = c["pos"], c["vel"], None, []
    for step in range(steps):
        if step == 0:
            rows = restated_rows(oracle, c, see_self)
            rows_of = lambda s, p, v: rows[s]
        else:
            rows_of = lambda s, p, v: R.eyes(oracle.cameras(p, v, c["up"], cp), oracle.instances(p, v), 0, c["width"], see_self, chunk=64)
        x, o, pos, vel = P.batch(rows_of, pos, vel, c["policies"], c["features"], c["hidden"], F32(c["limit"]), c["up"], dt=DT, variant=variant)
        first = (x, o) if step == 0 else first
        states.append((pos, vel))
    return first[0], first[1], states
