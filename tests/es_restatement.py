"""numpy restatement of DESIGN.md section 14.6: one evolution-strategies generation over a scene batch (include/nenbody.h E1-E8).

TEST INFRASTRUCTURE.  The kernels (nenbody_amd/csrc/nb_scenes_es.inc) and this module implement the same rule independently; the GPU
tests compare every word.  Philox runs in uint64 arithmetic masked to 32 bits, every sum of draws in int64 (or in Python integers),
every float step is one binary32 operation on numpy float32 values in the order the rule writes it, and (float) of a 64-bit integer is
taken from the Python integer by an explicit round to nearest even (f32_of_int), never through binary64.

``variant`` names a CONTROL ARM, a deliberate departure from the rule that tests/test_scenes_es_cpu.py shows its cases can tell from
the rule:
  "swap_sm"      the counter's first two words swapped: (s >> 1, m >> 1, g, 0)
  "odd_x01"      odd m taking (x0, x1) as even m does
  "no_mirror"    scene 2q + 1 drawing k, not -k
  "nine_rounds"  nine Philox rounds
  "no_bump"      the key not bumped between the rounds
  "uncentred"    k without the - 131 070
  "fma"          E3 and E7 with the product not rounded before it is added
  "near_f64"     (float)near through binary64
  "no_skip"      a zero coefficient not skipped: 0 * inf and 0 * NaN enter
  "nan_best"     a NaN fitness ranked above everything
  "ties_desc"    equal fitnesses ranked by descending scene index
  "u_is_r"       the utility not centred: u = r
  "reversed"     the update's sign reversed
  "a32"          A accumulated modulo 2^32"""
import math

import numpy as np

import score_restatement as Q

F32 = np.float32
U64 = np.uint64
MASK = U64(0xFFFFFFFF)
M0, M1 = U64(0xD2511F53), U64(0xCD9E8D57)
W0, W1 = U64(0x9E3779B9), U64(0xBB67AE85)
C_BITS = 0x37DDB3D7
C = np.uint32(C_BITS).view(F32)                     # sqrt(3) * 2^-16
K_MAX = 131070
MAX_POPULATION = 4096
FIELDS = ("near", "spread", "speed2", "momentum2", "goal2", "nonfinite")
REPORT_DTYPE = np.dtype([("best_scene", np.uint32), ("best_fitness", F32), ("nan_count", np.uint32), ("generation", np.uint32)])
ARMS = ("swap_sm", "odd_x01", "no_mirror", "nine_rounds", "no_bump", "uncentred", "fma", "near_f64", "no_skip", "nan_best", "ties_desc",
        "u_is_r", "reversed", "a32")


def policy_floats(features, hidden):
    return features * hidden + hidden + 2 * hidden + 2


# -- E1 -------------------------------------------------------------------------------------------------------------------------------------
def philox(counter, key, rounds=10, bump=True):
    """Philox4x32: counter, four arrays (or scalars) of 32-bit words; key, two; returns the four output words as uint64 arrays < 2^32"""
    c0, c1, c2, c3 = (np.asarray(c, U64) & MASK for c in counter)
    k0, k1 = (np.asarray(k, U64) & MASK for k in key)
    for r in range(rounds):
        if r and bump:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c0, M1 * c2                                                        # 32 x 32 -> 64 bits, exact in uint64
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> U64(32)) ^ c3 ^ k1, p0 & MASK
    return c0, c1, c2, c3


# -- E2 -------------------------------------------------------------------------------------------------------------------------------------
def draws(seed, g, scenes, ms, variant=None):
    """k(s, m) for the scenes `scenes` (S,) and the weights `ms` (M,): int64 (S, M)"""
    s = np.asarray(scenes, U64).reshape(-1, 1)
    m = np.asarray(ms, U64).reshape(1, -1)
    s, m = np.broadcast_arrays(s, m)
    one = U64(1)
    first, second = (s >> one, m >> one) if variant == "swap_sm" else (m >> one, s >> one)
    x = philox((first, second, np.full(s.shape, int(g) & 0xFFFFFFFF, U64), np.zeros(s.shape, U64)),
               (U64(int(seed) & 0xFFFFFFFF), U64((int(seed) >> 32) & 0xFFFFFFFF)),
               rounds=9 if variant == "nine_rounds" else 10, bump=variant != "no_bump")
    odd = (m & one) == one
    if variant == "odd_x01":
        odd = np.zeros_like(odd)
    a, b = np.where(odd, x[2], x[0]), np.where(odd, x[3], x[1])
    lo, sh = U64(0xFFFF), U64(16)
    k = ((a & lo) + (a >> sh) + (b & lo) + (b >> sh)).astype(np.int64)
    if variant != "uncentred":
        k = k - K_MAX
    if variant != "no_mirror":
        k = np.where((s & one) == one, -k, k)
    return k


def noise(k):
    """e = (float)k * C; (float)k is exact: |k| < 2^24"""
    return np.asarray(k).astype(F32) * C


# -- E3 -------------------------------------------------------------------------------------------------------------------------------------
def population(mean, sigma, seed, g, first_scene, count, variant=None):
    """theta of scenes [first_scene, first_scene + count): float32 (count, M)"""
    mean = np.ascontiguousarray(mean, F32).reshape(-1)
    e = noise(draws(seed, g, np.arange(first_scene, first_scene + count), np.arange(len(mean)), variant))
    with np.errstate(all="ignore"):
        if variant == "fma":
            return (mean.astype(np.float64)[None] + np.float64(F32(sigma)) * e.astype(np.float64)).astype(F32)
        return mean[None] + (F32(sigma) * e).astype(F32)


# -- E4 -------------------------------------------------------------------------------------------------------------------------------------
def f32_of_int(n):
    """(float)n for a Python integer 0 <= n < 2^65, rounded to nearest even ONCE, without binary64 in between"""
    n = int(n)
    bits = n.bit_length()
    if bits <= 24:
        return F32(n)
    shift = bits - 24
    q, rem, half = n >> shift, n & ((1 << shift) - 1), 1 << (shift - 1)
    if rem > half or (rem == half and (q & 1)):
        q += 1
    return F32(math.ldexp(float(q), shift))                                              # q <= 2^24: exact


def fitness(records, coef, variant=None):
    """phi of every record (Q.DTYPE, (B,)): float32 (B,)"""
    rec = np.ascontiguousarray(records, Q.DTYPE).reshape(-1)
    coef = np.ascontiguousarray(coef, F32).reshape(6)
    out = np.zeros(len(rec), F32)
    with np.errstate(all="ignore"):
        for s, r in enumerate(rec):
            near = F32(np.float64(int(r["near"]))) if variant == "near_f64" else f32_of_int(int(r["near"]))
            fields = (near, F32(r["spread"]), F32(r["speed2"]), F32(r["momentum2"]), F32(r["goal2"]), f32_of_int(int(r["nonfinite"])))
            phi = F32(0)
            for c, f in zip(coef, fields):
                if c == 0 and variant != "no_skip":
                    continue
                phi = F32(phi + F32(c * f))
            out[s] = phi
    return out


# -- E5, E6 ---------------------------------------------------------------------------------------------------------------------------------
def keys(phi, variant=None):
    """key64 of every scene: Python integers"""
    phi = np.ascontiguousarray(phi, F32).reshape(-1)
    b = len(phi)
    out = []
    for s, (f, w) in enumerate(zip(phi, phi.view(np.uint32))):
        w = int(w)
        if np.isnan(f):
            k32 = 0xFFFFFFFF if variant == "nan_best" else 0
        else:
            k32 = (~w & 0xFFFFFFFF) if w & 0x80000000 else (w | 0x80000000)
        out.append(k32 << 32 | ((b - 1 - s) if variant == "ties_desc" else s))
    return out


def ranks(phi, variant=None):
    """r_s: uint32 (B,), a permutation of 0 .. B-1"""
    k = keys(phi, variant)
    r = np.zeros(len(k), np.uint32)
    for place, s in enumerate(sorted(range(len(k)), key=k.__getitem__)):
        r[s] = place
    return r


def utilities(r, variant=None):
    r = np.asarray(r).astype(np.int64)
    return r if variant == "u_is_r" else 2 * r - (len(r) - 1)


def report(phi, r, g):
    phi = np.ascontiguousarray(phi, F32).reshape(-1)
    out = np.zeros((), REPORT_DTYPE)
    best = int(np.argmax(np.asarray(r)))
    out["best_scene"], out["best_fitness"], out["nan_count"], out["generation"] = best, phi[best], int(np.isnan(phi).sum()), int(g) & 0xFFFFFFFF
    return out


# -- E7 -------------------------------------------------------------------------------------------------------------------------------------
def sums(seed, g, r, m_count, variant=None):
    """A_m as Python integers, (M,)"""
    u = utilities(r, variant)
    k = draws(seed, g, np.arange(len(u)), np.arange(m_count), variant)
    a = (u[:, None] * k).sum(0)                                                          # |A| < 2^42: exact in int64
    if variant == "a32":
        a = a.astype(np.int32).astype(np.int64)                                          # the low 32 bits, as a signed word
    return [int(x) for x in a]


def f32_of_signed(n):
    return F32(-f32_of_int(-n)) if n < 0 else f32_of_int(n)


def update(mean, step, seed, g, r, variant=None):
    """mean' (M,) float32"""
    mean = np.ascontiguousarray(mean, F32).reshape(-1)
    fa = np.array([f32_of_signed(a) for a in sums(seed, g, r, len(mean), variant)], F32)
    step = F32(-step) if variant == "reversed" else F32(step)
    with np.errstate(all="ignore"):
        d = (fa * C).astype(F32)
        if variant == "fma":
            return (mean.astype(np.float64) + np.float64(step) * d.astype(np.float64)).astype(F32)
        return mean + (step * d).astype(F32)


# -- a generation ---------------------------------------------------------------------------------------------------------------------------
def rank_and_update(mean, sigma, step, coef, seed, g, records, variant=None):
    """what nb_scenes_es_update_launch leaves: (ranks, fitnesses, report, mean')"""
    phi = fitness(records, coef, variant)
    r = ranks(phi, variant)
    return r, phi, report(phi, r, g), update(mean, step, seed, g, r, variant)


def same_floats(got, want):
    """every word equal, a NaN met by a NaN"""
    g, w = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    return g.shape == w.shape and bool(((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))).all())


def same_report(got, want):
    g, w = np.ascontiguousarray(got, REPORT_DTYPE).reshape(()), np.ascontiguousarray(want, REPORT_DTYPE).reshape(())
    return all(g[f] == w[f] for f in ("best_scene", "nan_count", "generation")) and same_floats(g["best_fitness"], w["best_fitness"])
