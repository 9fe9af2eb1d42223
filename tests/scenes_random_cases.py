"""Seeded random problems for the four laws of a scene batch: the data of tests/test_gpu_scenes_random.py and
the numpy expectation of the two vision laws (no test in here).

TEST INFRASTRUCTURE.  case(law, i) is problem i of a law, drawn from numpy's default_rng(BASE[law] + i): a failure prints the case's
line and `case(law, i)` gives the same arrays again.  NB_RANDOM_CASES=N widens every family to N cases, as it does in
tests/test_gpu_random_differential.py.

  * "nbody", "boids" (scenes_nbody_kernel, scenes_boids_kernel): n on both sides of every workgroup size and of the two-bodies-per-lane
    line, B of 1, 2 or 5 scenes, 1 to 3 steps, constants from the choice lists of test_strict_random_problems_bit_exact and
    test_boids_random_problems_bit_exact, and every SCENE its own test_gpu_random_differential.random_state: scales from 1e-3 to 1e5,
    planar, clustered, with outliers of x1e9 and x1e-30, or plain 3-D, so that flagged and unflagged, planar and 3-D scenes share a
    launch.  The x1e-30 coordinates lie on the LOW side of the divide guard.  That half of the data is compared all the same but is
    NOT sharp: a CPU cannot restate v_rcp_f32, so no witness can be sought without the device, and a build of scenes_nbody_kernel that
    never flags a coordinate below 2^a was tried once on an MI355X and gave the reference's bits on every one of the default cases.
    The x1e9 coordinates stay below 2^64, where the ladder would give NaN: they leave the range it is proven for, not the number
    format, and builds with a forgotten high-side flag passed these cases too.  The sharp guard data is
    tests/scenes_guard_cases.py's; what these cases hold is the fold itself on either path, the planar shortcut and the isolation of
    scenes of different kinds in one launch.
  * "seen", "located" (scenes_boids_seen_kernel, scenes_nbody_located_kernel): n on both sides of the one-wave / four-wave line (128)
    and of the second pass over the bodies (64, 256), rows of 1 to 1 024 columns, B of 1, 2 or 4, 1 or 2 steps, two up vectors,
    positions uniform in +-3, 10, 30 or 100, and every scene planar, clustered, with an eighth of its velocities exactly zero (NaN
    cameras and NaN model matrices) or plain 3-D, each kind as likely as another.  tests/test_scenes_random_cpu.py caps the share of
    cases in which nobody sees anybody (of the default 36: 1 for "seen", 4 for "located", all of them scenes of 2 or 5 bodies).

vision_expected() chains the numpy restatements step by step and scene by scene: cameras and model matrices by the C oracle, rows by
eyes_restatement.eyes, sets and step by seen_restatement / located_restatement."""
import os

import numpy as np

import eyes_restatement as R
import located_restatement as L
import seen_restatement as S
from scenes_cases import ALT_GRAVITY
from test_gpu_random_differential import random_state

F = np.float32
CASES = int(os.environ.get("NB_RANDOM_CASES", "36"))
LAWS = ("nbody", "boids", "seen", "located")
BASE = {"nbody": 21000, "boids": 22000, "seen": 23000, "located": 24000}

SIZES = [1, 2, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 700, 1023, 1024, 1025, 1500, 2047, 2048]
GRAVITY_CHOICES = dict(dt=[0.1, 0.01, 1.0], g=[0.001, 1.0, -0.05, 1e-6], bias=[1e-7, 1e-3, 2.0])          # oracle.run's keywords
BOIDS_CHOICES = dict(r1=[1000.0, 50.0, 1e6], r2=[5.0, 0.5, 40.0], r3=[500.0, 0.3, 2.0], dt=[0.04, 0.5], s1=[0.02, -0.01],
                     s2=[0.05, 1.0], s3=[0.5, 0.0])                                                        # seen_cases.FIELDS' keys

VISION_SIZES = [2, 5, 63, 64, 65, 100, 128, 129, 200, 257]
VISION_WIDTHS = [1, 7, 63, 64, 65, 200, 256, 1024]
VISION_UPS = [(0.0, 0.0, 1.0), (0.6, 0.0, 0.8)]
VISION_SCALES = [3.0, 10.0, 30.0, 100.0]
VISION_KINDS = ["planar", "clustered", "zero velocities", "3-D"]
VISION_GRAVITY = [dict(dt=0.1, g=0.001, bias=0.0000001), ALT_GRAVITY]                    # the reference's constants, and a second set


def _draw(rng, choices):
    return {key: float(rng.choice(vals)) for key, vals in choices.items()}


def _whole_set_case(law, i):
    rng = np.random.default_rng(BASE[law] + i)
    n = int(rng.choice(SIZES))
    batch = int(rng.choice([1, 2, 5]))
    k = int(rng.integers(1, 4))
    consts = _draw(rng, GRAVITY_CHOICES if law == "nbody" else BOIDS_CHOICES)
    states = [random_state(rng, n) for _ in range(batch)]
    pos, vel = np.stack([p for p, _ in states]), np.stack([v for _, v in states])
    line = f"case('{law}', {i}): n={n} B={batch} k={k} {consts} scenes: {[scene_kind(p) for p in pos]}"
    return dict(law=law, i=i, n=n, batch=batch, k=k, consts=consts, pos=pos, vel=vel, line=line)


def scene_kind(pos):
    """what random_state drew, read off the positions (n, 3): the scale and "planar" / "high" (a coordinate of x1e9) / "low" (x1e-30)"""
    mag = np.abs(pos)
    tags = []
    if not pos[:, 2].any():
        tags.append("planar")
    if (mag > 1.5e5).any():               # the largest scale is 1e5
        tags.append("high")
    if ((mag > 0) & (mag < 1e-20)).any():
        tags.append("low")
    body = np.median(mag[mag > 0]) if (mag > 0).any() else 0.0
    return f"~{body:.0e}" + "".join(" " + t for t in tags)


def _vision_state(rng, n):
    scale = float(rng.choice(VISION_SCALES))
    kind = VISION_KINDS[int(rng.integers(0, len(VISION_KINDS)))]
    pos = (rng.uniform(-1, 1, (n, 3)) * scale).astype(F)
    vel = (rng.uniform(-1, 1, (n, 3)) * float(rng.choice([1e-3, 0.1, 2.0]))).astype(F)
    if kind == "planar":
        pos[:, 2] = 0
        vel[:, 2] = 0
    elif kind == "clustered":             # coincident bodies: they hide one another at equal depth
        pos[rng.integers(0, n, n // 2)] = pos[rng.integers(0, n, n // 2)]
    elif kind == "zero velocities":       # an eighth of the bodies look nowhere: NaN cameras, NaN model matrices
        vel[rng.choice(n, max(1, n // 8), replace=False)] = 0
    return pos, vel, f"{kind} +-{scale:g}"


def _vision_case(law, i):
    rng = np.random.default_rng(BASE[law] + i)
    n = int(rng.choice(VISION_SIZES))
    width = int(rng.choice(VISION_WIDTHS))
    batch = int(rng.choice([1, 2, 4]))
    k = int(rng.choice([1, 2]))
    up = VISION_UPS[int(rng.integers(0, 2))]
    consts = _draw(rng, BOIDS_CHOICES) if law == "seen" else dict(VISION_GRAVITY[int(rng.integers(0, 2))])
    states = [_vision_state(rng, n) for _ in range(batch)]
    pos, vel = np.stack([p for p, _, _ in states]), np.stack([v for _, v, _ in states])
    kinds = [t for _, _, t in states]
    line = f"case('{law}', {i}): n={n} W={width} B={batch} k={k} up={up} {consts} scenes: {kinds}"
    return dict(law=law, i=i, n=n, width=width, batch=batch, k=k, up=np.array(up, F), consts=consts, pos=pos, vel=vel, kinds=kinds, line=line)


def case(law, i):
    """problem i of a law: a dict of n, batch, k, consts, pos and vel ((B, n, 3) float32), line -- and width, up, kinds for the vision laws"""
    return _whole_set_case(law, i) if law in ("nbody", "boids") else _vision_case(law, i)


_expected = {}


def vision_expected(oracle, law, i):
    """(pos, vel, lists): the state after the case's k steps, (B, n, 3) each, and the sets the FIRST step folds over, scene by scene --
    seen: (count (n,), ids (n, W)); located: (count, ids, depth, col (n, W), rel (n, W, 4)).  Computed once per case, never written to."""
    if (law, i) in _expected:
        return _expected[(law, i)]
    c = case(law, i)
    n, width, up = c["n"], c["width"], c["up"]
    cp = R.eye_constant(oracle, width)
    consts = {key: F(val) for key, val in c["consts"].items()}
    out_p, out_v, lists = np.empty_like(c["pos"]), np.empty_like(c["vel"]), []
    for s in range(c["batch"]):
        p, v = c["pos"][s], c["vel"][s]
        for step in range(c["k"]):
            ids, depth = R.eyes(oracle.cameras(p, v, up, cp), oracle.instances(p, v), 0, width, chunk=64)
            if law == "seen":
                found = S.seen_rows(ids)[:2]
                p, v = S.boids_seen_step(p, v, S.mask_of_rows(ids, n), **consts)
            else:
                count, sids, sdepth, _, col, rel = L.located_of_rows(ids, depth, v, up, cp)
                found = (count, sids, sdepth, col, rel)
                p, v = L.nbody_located_step(p, v, count, rel, **consts)
            if step == 0:
                lists.append(found)
        out_p[s], out_v[s] = p, v
    lists = tuple(np.stack([f[a] for f in lists]) for a in range(len(lists[0])))
    for a in (out_p, out_v) + lists:
        a.setflags(write=False)
    _expected[(law, i)] = (out_p, out_v, lists)
    return _expected[(law, i)]
