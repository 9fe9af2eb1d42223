"""An n-body state whose one- and two-step results are exact binary32 numbers in ANY order of summation (test infrastructure).

The bodies sit on the sites of a small lattice whose distinct sites are all the same distance apart:

    tetra        (0,0,0) (1,1,0) (1,0,1) (0,1,1)   r^2 = 2,  bias = 2: every cross-site denominator is 4
    tetra_mixed  the same without a z offset: two sites in the plane z = 0, two off it (planar and 3-D tiles in one step)
    planar       (0,0,0) (1,1,0)                   r^2 = 2,  bias = 2
    line         (0,0,0) (1,0,0)                   r^2 = 1,  bias = 1: every cross-site denominator is 2

scaled by s = 2^k and shifted by a dyadic offset, with G = G0 s^2 (G0, dt signed powers of two).  Every cross-site term
(d * G) / (r^2 + bias) is then +-G0 s / 4 (line: / 2) in a component where the sites differ and 0 where they do not; bodies on one
site give d = 0 and add exactly 0.  Both denominators, bias and r^2 + bias, are powers of two: FAST's shared reciprocal
(1/a = b * rcp(a * b)) is exact only then -- with bias = 3 s^2 on the line, a same-site pair sharing a v_rcp_f32 with a cross-site
pair makes the cross-site reciprocal round.  Every partial sum is an integer multiple of that unit, so as long as every value stays below 2^24 units
no order of additions can round -- a correct FAST form must reproduce the closed form

    a_i = sum_t c_t G (P_t - P_sigma(i)) / 4 s^2          (c_t bodies on site t, sigma(i) the site of body i; line: 2 s^2)

bit for bit, and one dropped or doubled cross-site pair moves the bodies of that pair by a whole unit.  The expected state is
computed here in integers in O(n), never from a pair loop.

Two steps stay exact if every body of site t starts with w - a_t dt: after the first step every velocity is w, the lattice has
moved by w undeformed and the second step has the same closed form.  That second step cannot tell a stale record from a fresh one:
its pair terms are those of the first step, so a rank that reads last step's forces, last step's positions of a whole slot, or a
slot of its own one step late still reproduces it.  `permute` = pi, a permutation of the kind's sites that moves every occupied
one, closes that gap: the bodies of site t start with w + (P_pi(t) - P_t) - a_t dt, so the first step carries every site onto
ANOTHER site (plus w).  Distinct sites stay distinct and equidistant, so every value stays on the grid, but the second step's
closed form is K'_t = sum_u c_u (P_pi(u) - P_pi(t)), which `lattice` requires to differ from the first step's K_t on every
occupied site: one stale record then moves its bodies.  (tetra_mixed: bodies also change layer, planar and 3-D, between steps.)

`lattice` refuses (ValueError) any parameters for which a value of either step would leave the exact range.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F32_EXACT = 1 << 24           # integers of magnitude < 2^24 times a power of two are binary32 numbers
NORMAL_MIN, NORMAL_MAX = 2.0 ** -126, 2.0 ** 127

KINDS = {
    # sites in units of s, offset in units of s (a multiple of 1/4), bias in units of s^2, cross-site r^2 + bias in units of s^2
    "tetra": (((0, 0, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1)), (-0.75, 0.5, 0.25), 2, 4),
    "tetra_mixed": (((0, 0, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1)), (0.25, -0.5, 0.0), 2, 4),
    "planar": (((0, 0, 0), (1, 1, 0)), (0.5, -0.25, 0.0), 2, 4),
    "line": (((0, 0, 0), (1, 0, 0)), (-0.25, 0.75, 0.0), 1, 2),
}
OFFSET_DENOM = 4              # offsets are multiples of s / 4


def _pow2(x, what):
    m, e = np.frexp(abs(float(x)))
    if x == 0 or m != 0.5:
        raise ValueError(f"{what} = {x!r} is not a signed power of two")
    return int(e) - 1


@dataclass
class Lattice:
    pos: np.ndarray            # (n, 3) binary32
    vel: np.ndarray            # (n, 3) binary32
    dt: np.float32
    G: np.float32
    bias: np.float32
    steps: int
    p_exp: np.ndarray          # (n, 3) binary32: the exact state after `steps` steps
    v_exp: np.ndarray
    site: np.ndarray           # (n,) site of every body
    counts: np.ndarray         # bodies per site
    K: np.ndarray              # (T, 3) integers: the first step's acceleration of site t, sum_u c_u (P_u - P_t) / s
    K2: np.ndarray             # (T, 3) the second step's (steps=2; None for one): K'_t = sum_u c_u (P_pi(u) - P_pi(t)) / s
    permute: tuple             # pi (steps=2 with `permute`), else None
    p_mid: np.ndarray          # (n, 3) binary32: the exact state after the first step
    v_mid: np.ndarray
    unit: float                # the grid every position and velocity lies on
    dv_pair: float             # |dv| one cross-site pair adds in a component where its sites differ
    margin_bits: float         # log2(2^24 / the largest integer in units of `unit` or of the terms)
    kind: str
    scale: float

    @property
    def consts(self):
        return self.dt, self.G, self.bias

    def describe(self) -> str:
        return (f"lattice(n={len(self.pos)}, kind={self.kind}, scale=2^{_pow2(self.scale, 'scale')}, G={float(self.G)!r}, "
                f"dt={float(self.dt)!r}, steps={self.steps}, counts={self.counts.tolist()}, permute={self.permute}, margin {self.margin_bits:.1f} bits)")


def lattice(n: int, seed: int = 0, kind: str = "tetra", scale: float = 1.0, G0: float = -2.0 ** -3, dt: float = 2.0 ** -1,
            steps: int = 1, runs: int = 0, empty=(), skew=None, vmax: int = 1 << 10, sites=None, permute=None) -> Lattice:
    """The exact state described in the module docstring.

    runs:  0 = every body's site drawn at random; r > 0 = one site per run of r consecutive bodies (whole tiles, blocks or ranks
           of one site: pairs that are all zero, or all cross-site).
    empty: sites that get no body.   skew: relative weights of the sites (default: equal).
    vmax:  one step: velocities are random multiples of the unit in [-vmax, vmax]; two steps: w is.
    sites: the site of every body, given outright (overrides runs, empty and skew).
    permute: steps=2 only: pi, the site every site moves onto in the first step (module docstring).  Refused unless it is a
           permutation of the kind's sites that moves every occupied site and changes the acceleration of every occupied site.
    """
    if kind not in KINDS:
        raise ValueError(f"unknown kind {kind!r}")
    if steps not in (1, 2):
        raise ValueError("steps must be 1 or 2")
    if n < 1:
        raise ValueError("n must be positive")
    if permute is not None and steps != 2:
        raise ValueError("permute needs steps=2: it moves the sites between the two steps")
    sites_u, offset_u, bias_u, den_u = KINDS[kind]
    sites_u = np.array(sites_u, np.int64)
    T = len(sites_u)
    k = _pow2(scale, "scale")
    _pow2(G0, "G0"), _pow2(dt, "dt")
    if abs(G0) == abs(dt):
        raise ValueError("|G0| and |dt| must differ (a swap of G and dt must change bits)")
    s = 2.0 ** k
    G, bias = G0 * s * s, bias_u * s * s
    term = abs(G0) * s / den_u                     # |a| of one cross-site pair
    vunit = term * abs(dt)                         # |dv| of one cross-site pair
    unit = min(vunit, s / OFFSET_DENOM)            # grid of every position and velocity (both powers of two)
    # every intermediate the forms compute: d, d^2, r^2 + bias, its reciprocal, d * G, the terms, d / r^2, G * dt
    den = den_u * s * s
    # (the product of two r^2 that a shared reciprocal takes is the library's to guard: it shares only where that stays normal)
    smallest = min(s, s * s, bias, 1 / den, abs(G), abs(G) * s, term, s / den, vunit, unit)
    largest = max(s * 3, den, 1 / bias, abs(G), abs(G) * s, s / bias)
    if smallest < NORMAL_MIN or largest >= NORMAL_MAX:
        raise ValueError(f"scale 2^{k}, G0 {G0}, dt {dt}: a constant or a term leaves binary32's normal range")
    if n >= F32_EXACT:
        raise ValueError("n must stay below 2^24: a partial sum of n terms must be exact")

    rng = np.random.default_rng(seed)
    live = np.array([t for t in range(T) if t not in set(empty)])
    if len(live) == 0:
        raise ValueError("every site is empty")
    w_site = np.ones(T) if skew is None else np.asarray(skew, np.float64)
    p_live = w_site[live] / w_site[live].sum()
    if sites is not None:
        site = np.asarray(sites, np.int64)
        if site.shape != (n,) or site.min() < 0 or site.max() >= T:
            raise ValueError("sites: one site index per body")
    elif runs:
        site = np.repeat(rng.choice(live, size=-(-n // runs), p=p_live), runs)[:n]
    else:
        site = rng.choice(live, size=n, p=p_live)
    counts = np.bincount(site, minlength=T).astype(np.int64)

    # integer counts: K[t] = sum_u c_u (P_u - P_t) / s, the acceleration of site t in units of G0 s / den_u
    K = (counts[:, None, None] * (sites_u[:, None, :] - sites_u[None, :, :])).sum(axis=0)    # (T, 3): [t] = sum_u c_u (P_u - P_t)
    perm = np.arange(T)
    if permute is not None:
        perm = np.asarray(permute)
        if perm.shape != (T,) or perm.dtype.kind not in "iu" or sorted(perm.tolist()) != list(range(T)):
            raise ValueError(f"permute = {permute!r} is not a permutation of the {T} sites of {kind}")
        fixed = [t for t in range(T) if perm[t] == t and counts[t]]
        if fixed:
            raise ValueError(f"permute = {permute!r} leaves occupied site(s) {fixed} in place")
    moved = sites_u[perm]                             # the site every site stands on in the second step
    K2 = (counts[:, None, None] * (moved[:, None, :] - moved[None, :, :])).sum(axis=0)        # [t] = sum_u c_u (P_pi(u) - P_pi(t))
    if permute is not None:
        same = [t for t in range(T) if counts[t] and (K2[t] == K[t]).all()]
        if same:
            raise ValueError(f"permute = {permute!r}: occupied site(s) {same} keep their acceleration in the second step "
                             f"(K'_t == K_t: a stale record of them would be invisible)")
    sgn = int(np.sign(G0) * np.sign(dt))
    r = int(round(vunit / unit))                  # velocity units per grid unit (a power of two >= 1)
    q = int(round(s / unit))                      # grid units per s
    o = int(round(s / OFFSET_DENOM / unit))       # grid units per offset step
    P = sites_u * q + (np.round(np.array(offset_u) * OFFSET_DENOM).astype(np.int64) * o)[None, :]   # (T, 3) grid units
    planar_z = kind in ("planar", "line")
    if steps == 1:
        v0 = rng.integers(-vmax, vmax + 1, size=(n, 3)).astype(np.int64) * r
        if planar_z:
            v0[:, 2] = 0
        w = None
    else:
        w = rng.integers(-vmax, vmax + 1, size=3).astype(np.int64) * r
        if planar_z:
            w[2] = 0
        v0 = w[None, :] + (P[perm] - P)[site] - (sgn * K * r)[site]
    dv = (sgn * K * r)[site]                        # per body, grid units
    p0 = P[site]
    v1 = v0 + dv
    p1 = p0 + v1
    vals = [p0, v0, v1, p1]
    if steps == 2:
        assert (p1 == P[perm][site] + w[None, :]).all()
        v2 = v1 + (sgn * K2 * r)[site]
        p2 = p1 + v2
        vals += [v2, p2]
    biggest = max(int(np.abs(a).max()) for a in vals)
    biggest = max(biggest, n)                       # partial sums of terms: at most n units of `term`
    if biggest >= F32_EXACT:
        raise ValueError(f"n={n}, scale 2^{k}, G0 {G0}, dt {dt}: a value reaches {biggest} >= 2^24 grid units -- not exact")
    if biggest * unit >= NORMAL_MAX:
        raise ValueError("a position or velocity overflows binary32")
    to_f = lambda a: (a.astype(np.float64) * unit).astype(np.float32)   # exact: |a| < 2^24 and unit a power of two
    pos, vel = to_f(p0), to_f(v0)
    p_mid, v_mid = to_f(p1), to_f(v1)
    p_exp, v_exp = (p_mid, v_mid) if steps == 1 else (to_f(p2), to_f(v2))
    for a, b in ((pos, p0), (vel, v0), (p_mid, p1), (v_mid, v1), (p_exp, p1 if steps == 1 else p2)):
        assert (a.astype(np.float64) / unit == b).all()
    return Lattice(pos=pos, vel=vel, dt=np.float32(dt), G=np.float32(G), bias=np.float32(bias), steps=steps, p_exp=p_exp, v_exp=v_exp,
                   site=site, counts=counts, K=K, K2=K2 if steps == 2 else None,
                   permute=tuple(int(x) for x in perm) if permute is not None else None, p_mid=p_mid, v_mid=v_mid, unit=unit,
                   dv_pair=vunit, margin_bits=float(np.log2(F32_EXACT / max(biggest, 1))), kind=kind, scale=s)


def wrong_bodies(lat: Lattice, p, v, first: int = 0, count: int = None) -> np.ndarray:
    """Indices (into the whole set) of the bodies in [first, first + count) whose position or velocity differs from the closed form
    in any bit."""
    count = len(lat.pos) - first if count is None else count
    pe = lat.p_exp[first:first + count].view(np.uint32)
    ve = lat.v_exp[first:first + count].view(np.uint32)
    pg = np.ascontiguousarray(p, np.float32).view(np.uint32)
    vg = np.ascontiguousarray(v, np.float32).view(np.uint32)
    bad = (pg != pe).any(axis=1) | (vg != ve).any(axis=1)
    return first + np.flatnonzero(bad)


def assert_exact(lat: Lattice, p, v, what: str = "", first: int = 0, count: int = None) -> None:
    """Every body in [first, first + count), every component, every bit: the closed form."""
    bad = wrong_bodies(lat, p, v, first, count)
    if len(bad):
        i = int(bad[0])
        k = i - first
        raise AssertionError(f"{what} {lat.describe()}: {len(bad)} bodies differ from the closed form; first {i} (site {lat.site[i]}): "
                             f"p {np.asarray(p)[k].tolist()} v {np.asarray(v)[k].tolist()} expected p {lat.p_exp[i].tolist()} "
                             f"v {lat.v_exp[i].tolist()} (|dv| of one pair: {lat.dv_pair!r})")
