"""A boids state on which every sum of update_instance_boids (src/main.rs:443-526) is exact in ANY order (test infrastructure).

The split form of the boids step (nb_launch_boids_step_split) keeps the reference's neighbour sets and counts but reassociates
every sum: each slice of the j range is folded in index order, a body's slice rows are added in slice order, and where rule 3
holds for every pair its sum is the total of all velocities minus the body's own.  Off such a state it can only be held to a
tolerance.  On the states built here it must give the reference's bits on every body.

Why.  Let qp and qv be the largest powers of two that divide every position and every velocity coordinate.  Every value a sum
of the step adds is then an integer multiple of its quantum:

    rule 1   sum of p_j                    |partial sum| <= sum_j |p_j|
    rule 2   sum of (p_n - p_j)            |partial sum| <= sum_j |p_j| + n max|p|
    rule 3   sum of v_j, the prep kernel's total of all v, total - v_n      |partial sum| <= sum_j |v_j|

and every term is itself exact (|p_n - p_j| <= 2 max|p| is below the rule-2 bound for n >= 2).  If each bound stays below
2^24 quanta, per component, every partial sum of every subset in every order is an integer below 2^24 times a power of two: a
binary32 number, so no addition rounds, and the split form's sums equal the reference's.  The counts are sums of ones below
2^24 (the library refuses n >= 2^24), exact in any order too.  Both forms finish with the same binary32 operations
(main.rs:506-521), and their radius predicates take the same operands, so the results agree in every bit.  A dropped or doubled
neighbour, a row read from the wrong slice or body, a stale velocity or the wrong choice of the rule-3 shortcut then shows as a
wrong word.

`expected` computes the exact step in O(n + sites^2): rules 1 and 2 depend only on the body's position site, rule 3 only on
its velocity site, so each predicate is evaluated once per pair of sites (with the reference's binary32 expressions), the sums
are taken in int64 quanta, and the body's own term is removed (the reference skips only j == n, not other bodies on its site).
"""
from __future__ import annotations

from dataclasses import dataclass, fields, replace

import numpy as np

F = np.float32
F32_EXACT = 1 << 24

# nb_boids_params / nbo_boids_params without the tile: the reference's constants, src/main.rs:450-456
DEFAULTS = dict(dt=0.04, rule_1_distance=1000.0, rule_2_distance=5.0, rule_3_distance=500.0, rule_1_scale=0.02,
                rule_2_scale=0.05, rule_3_scale=0.5)


@dataclass(frozen=True)
class Consts:
    dt: float = DEFAULTS["dt"]
    rule_1_distance: float = DEFAULTS["rule_1_distance"]
    rule_2_distance: float = DEFAULTS["rule_2_distance"]
    rule_3_distance: float = DEFAULTS["rule_3_distance"]
    rule_1_scale: float = DEFAULTS["rule_1_scale"]
    rule_2_scale: float = DEFAULTS["rule_2_scale"]
    rule_3_scale: float = DEFAULTS["rule_3_scale"]

    def with_(self, **kw) -> "Consts":
        return replace(self, **kw)

    def items(self):
        return [(f.name, float(F(getattr(self, f.name)))) for f in fields(self)]

    def oracle(self, oracle):
        bp = oracle.boids_params()
        for k, v in self.items():
            setattr(bp, k, v)
        return bp

    def nb(self, nb, tile: int = 0):
        bp = nb.default_boids_params(tile=tile)
        for k, v in self.items():
            setattr(bp, k, v)
        return bp


# -- the certifier ------------------------------------------------------------------------------------------------------------
def quantum(a) -> float:
    """the largest power of two dividing every element of the binary32 array `a` (1.0 if all are zero; nan if one is not finite)"""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).ravel()
    if ((b & 0x7f800000) == 0x7f800000).any():
        return float("nan")
    b = b[(b & 0x7fffffff) != 0]
    if b.size == 0:
        return 1.0
    e = ((b >> 23) & 0xff).astype(np.int64)
    sig = np.where(e > 0, (b & 0x7fffff) | 0x800000, b & 0x7fffff).astype(np.int64)
    tz = np.zeros_like(sig)
    s = sig.copy()
    for _ in range(24):                      # trailing zeros of the significand
        z = (s & 1) == 0
        tz += z
        s = np.where(z, s >> 1, s)
    return float(2.0 ** int((np.maximum(e, 1) - 150 + tz).min()))


def bounds(pos, vel):
    """(qp, qv, the three bounds of the module docstring in quanta, per component): the largest of each is what must stay < 2^24"""
    pos, vel = np.asarray(pos, np.float32), np.asarray(vel, np.float32)
    qp, qv = quantum(pos), quantum(vel)
    if not (np.isfinite(qp) and np.isfinite(qv)):
        return qp, qv, None
    n = len(pos)
    ip = np.abs(pos.astype(np.float64) / qp).astype(np.int64)      # exact: a binary32 over a power of two that divides it
    iv = np.abs(vel.astype(np.float64) / qv).astype(np.int64)
    rule1 = ip.sum(axis=0)
    rule2 = rule1 + n * (ip.max(axis=0) if n else 0)
    rule3 = iv.sum(axis=0)
    return qp, qv, dict(rule1=rule1, rule2=rule2, rule3=rule3)


def why_not_exact(pos, vel) -> str | None:
    """None if the state is exact in the sense of the module docstring, else the reason"""
    pos, vel = np.asarray(pos, np.float32), np.asarray(vel, np.float32)
    if pos.ndim != 2 or pos.shape[1] != 3 or pos.shape != vel.shape:
        return "positions and velocities must both have shape (n, 3)"
    if len(pos) >= F32_EXACT:
        return "n >= 2^24: a count would round"
    qp, qv, b = bounds(pos, vel)
    if b is None:
        return "a coordinate is not finite"
    for name, v in b.items():
        if v.max() >= F32_EXACT:
            return f"{name} sum reaches {int(v.max())} >= 2^24 quanta (qp = {qp!r}, qv = {qv!r})"
    return None


def exact(pos, vel, bp=None) -> bool:
    """is every sum of a boids step of this state exact in any order?  (The constants do not enter: the sums do not scale.)"""
    return why_not_exact(pos, vel) is None


def assert_exact(pos, vel, bp=None) -> None:
    why = why_not_exact(pos, vel)
    if why is not None:
        raise ValueError(f"not an exact boids state: {why}")


# -- the expectation ----------------------------------------------------------------------------------------------------------
def finish(c, r, m, cnt, vcnt, pos, bp):
    """main.rs:506-521 in binary32, as tests/np_restatement.py::boids_step does: means, blend, clamp, move"""
    f = lambda k: F(getattr(bp, k))
    c, r, m = (np.asarray(a, np.float32) for a in (c, r, m))
    cnt, vcnt = np.asarray(cnt, np.float32), np.asarray(vcnt, np.float32)
    has = cnt > 0
    c = np.where(has[:, None], c / np.where(has, cnt, F(1))[:, None], c)
    hasv = vcnt > 0
    m = np.where(hasv[:, None], m / np.where(hasv, vcnt, F(1))[:, None], m)
    with np.errstate(over="ignore", invalid="ignore"):
        v = (c * f("rule_1_scale") + r * f("rule_2_scale")) + m * f("rule_3_scale")
        sq = v * v
        mag = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
        big = mag > F(1.0)
        scale = np.where(big, F(1.0) / np.where(big, mag, F(1.0)), F(1.0)).astype(np.float32)
        v = np.where(big[:, None], v * scale[:, None], v).astype(np.float32)
        p = (v * f("dt") + np.asarray(pos, np.float32)).astype(np.float32)
    return p, v, big


def _pairs(sites, pred, chunk=1 << 22):
    """bool matrix pred(d2) over every pair of sites (row a = the body's site, column b = the neighbour's), d = S[b] - S[a] and
    d2 = (dx*dx + dy*dy) + dz*dz in binary32 (main.rs:474, 485, 497)"""
    S = np.asarray(sites, np.float32)
    k = len(S)
    out = np.empty((k, k), bool)
    rows = max(1, chunk // max(k, 1))
    with np.errstate(over="ignore", invalid="ignore"):
        for a0 in range(0, k, rows):
            d = S[None, :, :] - S[a0:a0 + rows, None, :]
            sq = d * d
            out[a0:a0 + rows] = pred(((sq[..., 0] + sq[..., 1]) + sq[..., 2]).astype(np.float32))
    return out


def sums(pos, vel, bp):
    """the exact sums of one step, per body: (c, r, m, cnt, vcnt) as binary32 -- O(n + sites^2), never a pair loop"""
    assert_exact(pos, vel)
    pos, vel = np.asarray(pos, np.float32), np.asarray(vel, np.float32)
    qp, qv = quantum(pos), quantum(vel)
    P, ip = np.unique(pos, axis=0, return_inverse=True)
    V, iv = np.unique(vel, axis=0, return_inverse=True)
    ip, iv = ip.ravel(), iv.ravel()
    Cp = np.bincount(ip, minlength=len(P)).astype(np.int64)
    Cv = np.bincount(iv, minlength=len(V)).astype(np.int64)
    r1, r2, r3 = F(bp.rule_1_distance), F(bp.rule_2_distance), F(bp.rule_3_distance)
    p1 = _pairs(P, lambda d2: d2 < r1)
    p2 = _pairs(P, lambda d2: np.sqrt(d2) < r2)
    p3 = _pairs(V, lambda d2: np.sqrt(d2) < r3)
    PQ = np.rint(P.astype(np.float64) / qp).astype(np.int64)            # exact integers
    VQ = np.rint(V.astype(np.float64) / qv).astype(np.int64)
    own1, own2, own3 = np.diag(p1).astype(np.int64), np.diag(p2).astype(np.int64), np.diag(p3).astype(np.int64)
    cnt = (p1.astype(np.int64) @ Cp - own1)[ip]
    csum = (p1.astype(np.int64) @ (Cp[:, None] * PQ) - own1[:, None] * PQ)[ip]
    cnt2 = (p2.astype(np.int64) @ Cp - own2)
    rsum = (cnt2[:, None] * PQ - (p2.astype(np.int64) @ (Cp[:, None] * PQ) - own2[:, None] * PQ))[ip]
    vcnt = (p3.astype(np.int64) @ Cv - own3)[iv]
    msum = (p3.astype(np.int64) @ (Cv[:, None] * VQ) - own3[:, None] * VQ)[iv]
    for s in (csum, rsum, msum):
        assert np.abs(s).max(initial=0) < F32_EXACT
    f32 = lambda s, q: (s.astype(np.float64) * q).astype(np.float32)      # exact: < 2^24 quanta
    return f32(csum, qp), f32(rsum, qp), f32(msum, qv), cnt.astype(np.float32), vcnt.astype(np.float32)


def expected(pos, vel, bp, detail: bool = False):
    """the exact boids step of an exact state: (positions, velocities), and with detail=True also a dict of the sums, the counts
    and the clamp mask (|v| > 1, main.rs:516-518)"""
    c, r, m, cnt, vcnt = sums(pos, vel, bp)
    p, v, big = finish(c, r, m, cnt, vcnt, pos, bp)
    if not detail:
        return p, v
    return p, v, dict(c=c, r=r, m=m, cnt=cnt, vcnt=vcnt, clamped=big)


def wrong_bodies(p, v, p_exp, v_exp):
    """indices of the bodies whose position or velocity differs from the expectation in any bit"""
    b = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(len(a), -1)
    return np.flatnonzero((b(p) != b(p_exp)).any(axis=1) | (b(v) != b(v_exp)).any(axis=1))


# -- the host's thresholds, restated ------------------------------------------------------------------------------------------
def _bisect(holds):
    lo, hi = 0, 0x7f7fffff
    if not holds(lo):
        return F(-1)
    if holds(hi):
        return np.array([hi], np.uint32).view(np.float32)[0]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if holds(mid) else (lo, mid)
    return np.array([lo], np.uint32).view(np.float32)[0]


def _f(b):
    return np.array([b], np.uint32).view(np.float32)[0]


def sqrt_threshold(r) -> np.float32:
    """nb_api.hip:sqrt_threshold restated: the largest binary32 x >= 0 with sqrt(x) < r, or -1 if none"""
    r = F(r)
    if not r > 0:
        return F(-1)
    return _bisect(lambda b: np.sqrt(_f(b)) < r)


def rule3_bound(t3) -> np.float32:
    """nb_api.hip:rule3_always_bound restated: the largest binary32 V with ((2V)^2 + (2V)^2) + (2V)^2 <= t3, or -1 if none"""
    t3 = F(t3)
    if not t3 >= 0:
        return F(-1)

    def holds(b):
        v = _f(b)
        with np.errstate(over="ignore"):
            w = F(v + v)
            q = F(w * w)
            return F(F(q + q) + q) <= t3
    return _bisect(holds)


def vlim(bp) -> np.float32:
    """the rule-3 bound of the step (negative: no bound, rule 3 is always tested)"""
    return rule3_bound(sqrt_threshold(bp.rule_3_distance))


NONFINITE, VELFAR = 1, 4                  # nb_boids.inc: kBoidsNonFinite, kBoidsVelFar


def flag_word(pos, vel, bp) -> int:
    """the split form's flag word as boids_prep_kernel leaves it: a non-finite record, a velocity component above the bound"""
    pos, vel = np.asarray(pos, np.float32), np.asarray(vel, np.float32)
    w = 0
    if not (np.isfinite(pos).all() and np.isfinite(vel).all()):
        w |= NONFINITE
    lim = vlim(bp)
    mag = np.ascontiguousarray(vel).view(np.uint32) & 0x7fffffff
    if lim >= 0 and (mag > int(np.array([lim], np.float32).view(np.uint32)[0])).any():
        w |= VELFAR
    return w


def shortcut(word: int, bp, force: int = 0) -> bool:
    """does the split form take rule 3 from the total (boids_no3)?  The flag word clear, NB_BOIDS_FORCE without 4, a bound"""
    return (word & (NONFINITE | VELFAR)) == 0 and (force & 4) == 0 and vlim(bp) >= 0


def split_shape(n_total: int, count: int, tile: int, slices_knob=None):
    """nb_api.hip:boids_split_shape restated: (slices, j_chunk)"""
    ntiles = (n_total + tile - 1) // tile
    groups = max(1, (count + 255) // 256)
    sl = int(slices_knob) if slices_knob is not None else (512 + groups - 1) // groups
    sl = min(max(sl, 1), ntiles, 64)
    per = (ntiles + sl - 1) // sl
    return (ntiles + per - 1) // per, per * tile


def slices_from_scratch_bytes(nbytes: int, n_total: int, count: int) -> int:
    """nb_boids_split_scratch_bytes = slices * count * 48 + ceil(n / 1024) * 16 + 64 (nb_api.hip:boids_split_bytes), solved"""
    rows = nbytes - 64 - ((n_total + 1023) // 1024) * 16
    assert rows > 0 and rows % (48 * count) == 0, (nbytes, n_total, count)
    return rows // (48 * count)


# -- the builder --------------------------------------------------------------------------------------------------------------
KINDS = ("planar", "3d", "mixed", "rule3_holds", "rule3_edge", "rule3_cuts", "ties")


def _sites(rng, k, R, dim):
    """k distinct integer points of [-R, R]^dim (z = 0 for dim 2)"""
    side = 2 * R + 1
    total = side ** dim
    k = min(k, total)
    flat = rng.choice(total, size=k, replace=False)
    pts = np.zeros((k, 3), np.int64)
    for a in range(dim):
        pts[:, a] = flat % side - R
        flat = flat // side
    return pts


def boids_lattice(n: int, seed: int = 0, kind: str = "planar", *, R: int = 63, V: int = 63, qp: float = 1.0, qv: float = 2.0 ** -6,
                  psites: int | None = None, vsites: int | None = None, consts: Consts | None = None):
    """An exact state of n bodies (module docstring): positions are qp times integers in [-R, R], velocities qv times integers in
    [-V, V] (kinds that bound rule 3 use less), on `psites` / `vsites` distinct sites so that many bodies share one.  Returns
    (pos, vel, consts); ValueError for any request the certifier rejects.

      planar       z = 0, vz = 0 (the reference's own workload)
      3d           every coordinate free
      mixed        3-D, with runs of planar records (every other 1 024-record block, and one ragged run): both tile forms
      rule3_holds  rule_3_distance = 1, every velocity component inside rule3_always_bound: the shortcut path
      rule3_edge   the same with ONE component on the first lattice point above the bound: the in-loop path, same neighbours
      rule3_cuts   rule_3_distance = 16 qv: rule 3 cuts, the in-loop path
      ties         r1 = 25 qp^2, r2 = 5 qp, r3 = 5 qv with (3, 4) offsets everywhere: d2 == r1, sqrt(d2) == r2, |dv| == r3
    """
    if kind not in KINDS:
        raise ValueError(f"unknown kind {kind!r}")
    if n < 1:
        raise ValueError("n must be positive")
    for q, what in ((qp, "qp"), (qv, "qv")):
        if np.frexp(q)[0] != 0.5:
            raise ValueError(f"{what} = {q!r} is not a power of two")
    rng = np.random.default_rng(seed)
    cs = consts if consts is not None else Consts()
    dim = 2 if kind == "planar" else 3
    kp = psites if psites is not None else max(1, min(1024, n // 8))
    kv = vsites if vsites is not None else max(1, min(1024, n // 8))
    Vk = V
    if kind in ("rule3_holds", "rule3_edge"):
        cs = cs if consts is not None else cs.with_(rule_3_distance=1.0)
        lim = vlim(cs)
        Vk = min(V, int(np.floor(float(lim) / qv)))
        if Vk < 1:
            raise ValueError("rule3_always_bound leaves no lattice point above zero")
    elif kind == "rule3_cuts":
        cs = cs if consts is not None else cs.with_(rule_3_distance=16 * qv)
    elif kind == "ties":
        cs = cs if consts is not None else cs.with_(rule_1_distance=25 * qp * qp, rule_2_distance=5 * qp, rule_3_distance=5 * qv)
    P = _sites(rng, kp, R, dim)
    W = _sites(rng, kv, Vk, dim)
    if kind == "ties":                       # every site gets partners at (3, 4, 0) and (0, 3, 4) [planar: (4, 3, 0)] offsets
        offs = np.array([[3, 4, 0], [0, 3, 4], [-4, 0, 3]] if dim == 3 else [[3, 4, 0], [-4, 3, 0]], np.int64)
        base_p = P[: max(1, kp // (1 + len(offs)))]
        P = np.concatenate([base_p] + [base_p + o for o in offs])
        base_w = W[: max(1, kv // (1 + len(offs)))]
        W = np.concatenate([base_w] + [base_w + o for o in offs])
        P, W = np.clip(P, -R, R), np.clip(W, -Vk, Vk)
    pos = (P[rng.integers(len(P), size=n)] * qp).astype(np.float32)
    vel = (W[rng.integers(len(W), size=n)] * qv).astype(np.float32)
    if kind == "mixed":
        planar = (np.arange(n) // 1024) % 2 == 1
        planar[n // 3: n // 3 + 300] = True
        if n < 2048:
            planar[: n // 2] = True
        pos[planar, 2] = 0
        vel[planar, 2] = 0
    if kind == "rule3_edge":                 # the first lattice point above the bound, on one body
        lim = float(vlim(cs))
        above = (np.floor(lim / qv) + 1) * qv
        vel[rng.integers(n), rng.integers(dim)] = F(above if rng.integers(2) else -above)
    why = why_not_exact(pos, vel)
    if why is not None:
        raise ValueError(f"boids_lattice(n={n}, kind={kind}, R={R}, V={V}, qp={qp}, qv={qv}): {why}")
    if quantum(pos) < qp or quantum(vel) < qv:
        raise ValueError("a coordinate is off the lattice")
    return pos, vel, cs


def on_lattice(pos, vel, qp: float, qv: float) -> None:
    """ValueError unless every position is a multiple of qp and every velocity one of qv, and the state is exact"""
    if quantum(pos) < qp:
        raise ValueError(f"a position is not a multiple of qp = {qp!r}")
    if quantum(vel) < qv:
        raise ValueError(f"a velocity is not a multiple of qv = {qv!r}")
    assert_exact(pos, vel)


# -- a schedule that stays exact ----------------------------------------------------------------------------------------------
def schedule_consts(qp: float = 1.0, qv: float = 2.0 ** -6) -> Consts:
    """constants of a boids step whose RESULT is again an exact state, for boids -> n-body -> boids schedules: r1 below one
    lattice step (a body's rule-1 neighbours are the bodies on its site, so their mean is the site itself), r2 = 1.5 steps
    (neighbours on the same or an adjacent site), r3 below one velocity step (the mean velocity is the body's own), and s1, s2,
    s3, dt powers of two.  The new velocity p s1 + r s2 + v s3 and position v dt + p then lie on a grid of qp / 256, as long as
    the clamp does not fire: `schedule_state` builds a state where it cannot."""
    return Consts(dt=1.0, rule_1_distance=0.5 * qp * qp, rule_2_distance=1.5 * qp, rule_3_distance=0.5 * qv,
                  rule_1_scale=2.0 ** -8, rule_2_scale=2.0 ** -8, rule_3_scale=0.5)


def schedule_state(n: int, seed: int = 0):
    """(pos, vel, A, B): a 3-D exact state for the schedule  boids(A) -> n-body (dt = 0: p + v) -> boids(B), every state of
    which is exact (ValueError otherwise); A = schedule_consts(), B = the reference's constants.  Positions within +-15 keep
    n max|p| below 2^23 quanta of the schedule's grid up to n = 2 184.  (dt = 0 keeps the velocities: the n-body step moves the
    positions only, so a host that skips rebuilding its velocity replica after it still has the right velocities.)"""
    pos, vel, _ = boids_lattice(n, seed, "3d", R=15, V=63)
    A = schedule_consts()
    p1, v1, d = expected(pos, vel, A, detail=True)
    if d["clamped"].any():
        raise ValueError("the clamp fired in the schedule's first step")
    p2 = (p1 + v1).astype(np.float32)          # main.rs:434-436 with dt = 0: v + s * 0 = v, then p + v
    assert_exact(p1, v1)
    assert_exact(p2, v1)
    return pos, vel, A, Consts()
