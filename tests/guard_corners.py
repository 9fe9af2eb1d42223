"""STRICT's divide guard, restated for the tests, and data that sits on its corners or just outside it (no test in here).

STRICT divides every pair's (dx*G)/d with the shared-reciprocal ladder while all coordinates lie in {0} U [2^a, 2^b]
(nb_plan.h:strict_divide_guard) and with the IEEE '/' as soon as a tile, a workgroup's own bodies or, for the plane forms, the whole
step holds a coordinate outside that range.  Two kinds of data follow from that:

  * corner_state: everything inside the range, with bodies on its corners, so that d, n = dx*G and the ladder's residuals reach the
    extreme exponents the guard's derivation admits (coverage() measures them);
  * OUTLIER_VALUES: one coordinate of magnitude >= 2^64.  Then dx*dx overflows and d = +inf: the reference gives n/inf = +/-0, the ladder
    gives rcp(inf) = 0, fma(-inf, 0, 1) = NaN.  The reference's result holds no NaN on such data (tests/test_guard_corners_cpu.py),
    so one NaN in the device's result is a flag some form forgot to raise.
"""
import math
import os

import numpy as np

B = 20   # the guard's upper exponent: coordinates up to 2^20


def floor_log2(x):
    m, e = math.frexp(float(np.float32(x)))   # x = m * 2^e, m in [0.5, 1)
    return e - 1


def guard(G, bias):
    """(a, b, g, c, dmax) of the guarded range {0} U [2^a, 2^b] for these constants, or None where there is none and STRICT divides
    with '/' throughout: nb_plan.h:strict_divide_guard, restated.  |G| in [2^g, 2^(g+1)), bias in [2^c, 2^(c+1)), d < 2^dmax."""
    G, bias = float(np.float32(G)), float(np.float32(bias))
    if not (math.isfinite(G) and math.isfinite(bias) and abs(G) > 0.0 and bias > 0.0):
        return None
    g, c, b = floor_log2(abs(G)), floor_log2(bias), B
    dmax = max(2 * b + 4, c + 2)
    a = max(-100 + 23 - g, -120 + 23 - g + dmax)
    if not (-100 <= g <= 100 and c >= -100 and dmax <= 100 and b + 2 + g - c <= 120 and a <= b - 1):
        return None
    return max(a, -120), b, g, c, dmax


def guard_words(G, bias):
    """(lo_bits, hi_bits, force_ieee): the words the kernels are given"""
    gd = guard(G, bias)
    if gd is None:
        return 0x3f800000, 0x3f800000, 1
    return (gd[0] + 127) << 23, (gd[1] + 127) << 23, 0


# ---- launch shapes --------------------------------------------------------------------------------------------------------------
# the eleven of test_gpu_parity.py's `lanes` fixture with the same knobs, the scalar-load form's other two launch shapes, and whatever
# the plan picks with no knob set
STRICT_FORMS = [1, "1np", 2, 4, 8, 16, "pc8", "pc14", "pc14np", "bc", "sl", "sl2", "sl3", "default"]


def form_env(form):
    if form == "default":
        return {}
    if form == "bc":
        return {"NB_STRICT_BC": "1"}
    if form in ("sl", "sl2", "sl3"):
        return {"NB_STRICT_SL": form[2:] or "1", "NB_STRICT_BC": "0"}
    if form == "1np":
        return {"NB_STRICT_PC": "0", "NB_STRICT_LANES": "1", "NB_STRICT_NO_PACKED": "1"}
    if str(form).startswith("pc"):
        env = {"NB_STRICT_NO_PACKED": "1"} if form.endswith("np") else {}
        env["NB_STRICT_PC"] = form[2:].replace("np", "")
        return env
    return {"NB_STRICT_PC": "0", "NB_STRICT_LANES": str(form)}


def form_kernel(form):
    """the kernel a pinned form must plan, whatever the shard size (None: the plan's own choice)"""
    if form == "default":
        return None
    if form == "bc":
        return "step_strict_bc_kernel"
    if str(form).startswith("sl"):
        return "step_strict_sl_kernel"
    return "step_strict_pc_kernel" if str(form).startswith("pc") else "step_strict_kernel"


def apply(monkeypatch, form, params=None, n=0, counts=()):
    """Pin the launch shape (conftest.py's monkeypatch binds the legacy library for the knobs that need it); given `params`, also
    check that steps of `counts` bodies out of `n` then plan the form's kernel."""
    for k in [k for k in os.environ if k.startswith("NB_STRICT_")]:
        monkeypatch.delenv(k)
    for k, v in form_env(form).items():
        monkeypatch.setenv(k, v)
    if params is not None and form_kernel(form):
        from nenbody_amd import _lib

        for count in counts:
            assert _lib.planned_kernels(params, n, count)[0] == form_kernel(form), (form, n, count)


# ---- family A: corners inside the guard -------------------------------------------------------------------------------------------
# (G, bias): the first eight were tried with this generator before it was written down here; the ninth sits where the range is narrowest,
# g = -72, the smallest g that leaves a <= b - 1 (a = 19: one binade of coordinates), so that q = n/d goes down to 2^-119.
CORNER_CONSTANTS = [(0.001, 1e-7), (-0.001, 1e-7), (0.001, 2.0 ** 61), (0.001, 2.0 ** -100), (0.3, 2.0 ** -100), (2.0 ** 30, 1.0), (-2.0, 3.0),
                    (2.0 ** -60, 2.0 ** -20), (2.0 ** -72, 2.0 ** -20), (2.0 ** 100, 4.0)]
# The tenth is the largest g there is (g = 100 needs c >= 2 for b+2+g-c <= 120): a is clamped to -120, differences go down to the
# subnormal 2^-143 and n up to 2^121.  Its second step is left out: the first throws bodies to ~2^95, where the reference's own n = dx*G
# and d both overflow and n/d = NaN, and a bit comparison of NaNs says nothing about the guard.
CORNER_TWO_STEPS = CORNER_CONSTANTS[:9]
CORNER_N = 1537   # more than one 1 024-record tile; ragged for every tile size and for the 64- and 256-body workgroups
CORNER_DT = 0.1


def corner_id(case):
    G, bias = case
    return f"G{G:.3g}_bias{bias:.3g}"


def corner_state(n, a, b, seed):
    """(pos, vel): every |coordinate| is 0 or in [2^a, 2^b].  Log-uniform magnitudes with random signs; then, an eighth of the bodies
    each: on the cube's corners (+/-2^b in all three), one ulp inside those, at +/-2^a in all three, one ulp above those (same signs
    body for body, so the smallest non-zero |dx| is 2^(a-23)); then a few at the origin, a few with z = 0 only and a few coincident."""
    rng = np.random.default_rng(seed)
    mag = np.exp2(rng.uniform(a, b, (n, 3)))
    pos = (mag * rng.choice([-1.0, 1.0], (n, 3))).astype(np.float32)
    lo, hi = np.float32(2.0 ** a), np.float32(2.0 ** b)
    assert (np.abs(pos) >= lo).all() and (np.abs(pos) <= hi).all()
    m = n // 8
    idx = rng.permutation(n)   # scattered over the tiles and workgroups
    signs = rng.choice([-1.0, 1.0], (m, 3)).astype(np.float32)
    signs[0], signs[1] = 1.0, -1.0   # two opposite corners: |dx| = 2^(b+1) in all three components
    pos[idx[0 * m:1 * m]] = signs * hi
    pos[idx[1 * m:2 * m]] = signs * np.nextafter(hi, np.float32(0))
    pos[idx[2 * m:3 * m]] = signs * lo
    pos[idx[3 * m:4 * m]] = signs * np.nextafter(lo, np.float32(np.inf))
    rest = idx[4 * m:]
    k = max(2, n // 64)
    pos[rest[:k]] = 0.0
    pos[rest[k:2 * k], 2] = 0.0
    pos[rest[2 * k:3 * k]] = pos[rest[3 * k:4 * k]]
    vel = rng.uniform(-0.1, 0.1, (n, 3)).astype(np.float32)
    return pos, vel


def expected_coverage(G, bias):
    """(d_lo, d_hi, n_lo, n_hi): the exponents corner_state must reach.  d from the self pairs (d = bias) to two opposite corners
    (3 * 2^(2b+2) + bias, rounded once: the three squares and their sums are exact); non-zero |n| from |dx| = 2^(a-23) to 2^(b+1)."""
    a, b, g, c, _ = guard(G, bias)
    d_top = np.float32(3.0 * 2.0 ** (2 * b + 2)) + np.float32(bias)
    return c, floor_log2(d_top), a - 23 + g, b + 1 + g


def coverage(pos, G, bias):
    """(d_lo, d_hi, n_lo, n_hi): smallest and largest binary exponent of d and of non-zero |n| over all pairs, in binary32 and in the
    reference's order: d = ((dx*dx + dy*dy) + dz*dz) + bias, n = dx*G."""
    pos = np.ascontiguousarray(pos, np.float32)
    G, bias = np.float32(G), np.float32(bias)
    d_lo = n_lo = 1 << 30
    d_hi = n_hi = -(1 << 30)
    exps = lambda x: np.frexp(x)[1] - 1
    with np.errstate(over="ignore", under="ignore"):
        for i in range(0, len(pos), 128):
            dv = pos[None, :, :] - pos[i:i + 128, None, :]
            sq = dv * dv
            d = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + bias
            nn = np.abs(dv * G)
            assert d.dtype == np.float32 and nn.dtype == np.float32
            e = exps(d[np.isfinite(d)])
            d_lo, d_hi = min(d_lo, int(e.min())), max(d_hi, int(e.max()))
            if not np.isfinite(d).all():
                d_hi = 128
            e = exps(nn[nn > 0])
            n_lo, n_hi = min(n_lo, int(e.min())), max(n_hi, int(e.max()))
    return d_lo, d_hi, n_lo, n_hi


# ---- family B: one outlier at a time ----------------------------------------------------------------------------------------------
OUTLIER_N = 2049
OUTLIER_VALUES = [2.0 ** 64, -2.0 ** 70, 2.0 ** 100]
OUTLIER_INDICES = [0, 255, 256, 1023, 1024, 2047, 2048]
OUTLIER_STEPS = 2


def outlier_state(oracle, index, value, component, planar=False, n=OUTLIER_N, seed=64):
    """Ordinary data (test_gpu_parity.state3d's; planar: the reference's own z = 0 initial state) with one coordinate of one body replaced."""
    pos, vel = oracle.init_state(n, seed)
    if not planar:
        rng = np.random.default_rng(seed)
        pos[:, 2] = rng.uniform(-100, 100, n).astype(np.float32)
        vel[:, 2] = rng.uniform(0, 0.1, n).astype(np.float32)
    pos[index, component] = np.float32(value)
    return pos, vel


def outlier_cases():
    """(index, value, component, planar) of the whole-set outlier test.  Every index meets every value once, with the component
    alternating, and the planar path gets each index with one value: 28 cases, not the 7 x 3 x 2 + 7 x 3 of the full grid.  What a
    form can forget is a flag for a *place* (its own bodies, a tile's first or last record, the ragged last tile), and every place meets
    every value; which component trips coord_oor is one OR in every form, and both components occur at every place."""
    out = []
    for ii, index in enumerate(OUTLIER_INDICES):
        for vi, value in enumerate(OUTLIER_VALUES):
            out.append((index, value, (0, 2)[(ii + vi) % 2], False))
        out.append((index, OUTLIER_VALUES[ii % 3], 0, True))
    return out


def outlier_shard_cases():
    """(name, parts, index, value, component, steps) of the sharded outlier test; the checked bodies are those of `parts`.  Parts that
    do not cover the set leave the other bodies' new positions unwritten, so those cases run one step."""
    out = []
    for vi, value in enumerate(OUTLIER_VALUES):
        comp = (0, 2)[vi % 2]
        out += [("own_and_foreign", [(0, 513), (513, 1536)], 100, value, comp, OUTLIER_STEPS),   # shard 0's own body; a foreign record for shard 1
                ("foreign_last_record", [(0, 513)], 2048, value, comp, 1),                       # only in the ragged last tile
                ("foreign_first_record", [(1024, 1025)], 0, value, comp, 1),
                ("single_body_shard", [(2048, 1)], 2048, value, comp, 1)]                        # a shard of one body that is the outlier
    return out


# ---- family C: FAST with an overflowing pair ----------------------------------------------------------------------------------------
FAST_N = 2048


def fast_overflow_state(seed=70):
    """(pos, vel, dt, G, bias): ordinary data, two bodies with a coordinate of 2^64 and -2^70.  In binary32 their r^2 overflows; in
    binary64 their terms are merely tiny, so test_gpu_fast_binary64.check_bodies' bounds apply as they stand."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-100, 100, (FAST_N, 3)).astype(np.float32)
    vel = rng.uniform(-0.1, 0.1, (FAST_N, 3)).astype(np.float32)
    pos[300, 0] = np.float32(2.0 ** 64)
    pos[1700, 2] = np.float32(-2.0 ** 70)
    return pos, vel, np.float32(0.1), np.float32(0.001), np.float32(1e-7)
