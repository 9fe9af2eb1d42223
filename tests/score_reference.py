"""A binary64 reference of the score of a scene (include/nenbody.h Q2-Q7), with a derived bound beside every
value.

TEST INFRASTRUCTURE.  The kernel (nb_scenes_score.inc) and the numpy restatement (tests/score_restatement.py) were written from one
text, the steps Q1-Q7; this module is written from what the fields MEAN and imports no restatement:

  near        the number of unordered pairs {i, j}, i != j, whose squared distance is below radius_sq
  spread      the sum over the bodies of the squared distance from the centroid, the mean position
  speed2      the sum of |v|^2;  momentum2  |sum of v|^2;  goal2  the sum of the squared distance from the goal
  nonfinite   the bodies with a component of position or velocity that is not finite;  steps  the snapshots scored
and a record is the SUM of its snapshots' terms.

BOUNDS, first order, from magnitude sums, nothing tuned (U = 2^-24):
  a sum       of n leaves by the rule's tree passes every leaf through at most D = ceil(log2 n) additions: D U (sum of |leaf|).
  a leaf      ((a a) + (b b)) + (c c) of three differences: the difference 1, squared 2, the product 1, two sums 2: 6 U leaf (5 U for
              |v|^2, taken as 6).
  centroid    c = sum / n: D U (sum of |p_c|) / n + U |c|; a leaf of `spread` moves by 2 |p - c| delta + delta^2 a component.
  momentum2   each component sum m_c carries D U (sum of |v_c|) = delta: 2 |m_c| delta + delta^2, and 3 U on (|m_c| + delta)^2.
  subnormal   2^-149 per operation (a product in the subnormal range loses up to half of that, and no relative bound holds): on
              the "tiny" kind every square is subnormal.
  near        is an interval [sure, sure + maybe]: a pair is MAYBE when |d2 - radius_sq| is within d2's bound (6 U d2 + 8 x
              2^-149).  Where every step of a d2 is exact -- each difference, each square and both partial sums are binary32
              numbers as they stand in binary64 -- the bound is 0 and the pair is decided by d2 < radius_sq itself: on an
              integer lattice every pair is, however many of them tie with the radius.
  accumulate  one addition a field a snapshot: U |sum| on top of the terms' bounds; the first, into a cleared record, is exact.
`nonfinite` and `steps` are exact.  A field whose binary64 value is not finite (a scene with a non-finite body, in the fields its
positions or velocities reach) is not held; `near` counts the pairs whose d2 is finite and is always held.

What the bounds admit: the rule's tree in any association of depth D (adjacent pairs, padding skipped or added), a binary64 sum, a
fused multiply-add in a leaf, the centroid by a reciprocal.  A SERIAL sum is not admitted at n = 1 025 -- its partial sums pass a
leaf through up to n - 1 additions, not D -- and is no arm here.

Largest observed error / bound over score_cases.make at n in {2, 5, 65, 129, 300, 1 025}, every kind (test_policy_score_reference_cpu.py
and test_gpu_policy_score_reference.py print them; on the MI355X the device's words are the restatement's, so the figures are one):
spread 0.20, speed2 0.23, momentum2 0.35, goal2 0.19; with a second snapshot accumulated 0.18, 0.21, 0.30, 0.17; over three scored
rollouts of the policy 0.05, 0.06, 0.02, 0.12.  Maybe pairs: none on the lattice, at most 2 a scene elsewhere but on the "tiny" kind, whose bound is the subnormal
term (44 of 524 800 at n = 1 025; the cap is 0.1 %).
"""
import types

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
F32 = np.float32
FLOATS = ("spread", "speed2", "momentum2", "goal2")
LEAF = 6.0


def _is32(a):
    """a binary64 value is a binary32 number as it stands"""
    with np.errstate(all="ignore"):
        return a.astype(F32).astype(np.float64) == a


def _depth(n):
    return int(np.ceil(np.log2(n))) if n > 1 else 0


def pairs(pos, radius_sq):
    """(sure, maybe, pairs): unordered pairs surely nearer than the radius, pairs within their bound of it, and all of them"""
    p = np.asarray(pos, np.float64)
    n = len(p)
    i, j = np.triu_indices(n, 1)
    sure = maybe = 0
    r = float(radius_sq)
    for a in range(0, len(i), 1 << 18):
        ii, jj = i[a:a + (1 << 18)], j[a:a + (1 << 18)]
        with np.errstate(all="ignore"):
            d = p[ii] - p[jj]
            q = d * d
            s1 = q[:, 0] + q[:, 1]
            d2 = s1 + q[:, 2]
            exact = _is32(d).all(1) & _is32(q).all(1) & _is32(s1) & _is32(d2)
            bound = np.where(exact, 0.0, LEAF * U * d2 + 8 * TINY)
            finite = np.isfinite(d2)
            open_ = finite & ~exact & (np.abs(d2 - r) <= bound)
            sure += int((finite & ~open_ & (d2 < r)).sum())
            maybe += int(open_.sum())
    return sure, maybe, len(i)


def _sum_sq(d):
    return (d * d).sum(1)


def terms(pos, vel, radius_sq, goal):
    """one snapshot's terms: a namespace of near_lo, near_hi, maybe, pairs, nonfinite, steps = 1 and, per float field, its value and
    bound (`d` + name; not finite: the field is not held)"""
    p, v, g = np.asarray(pos, np.float64), np.asarray(vel, np.float64), np.asarray(goal, np.float64)
    n = len(p)
    D = _depth(n)
    out = types.SimpleNamespace(steps=1, nonfinite=int((~np.isfinite(np.concatenate([p, v], 1))).any(1).sum()))
    sure, out.maybe, out.pairs = pairs(p, radius_sq)
    out.near_lo, out.near_hi = sure, sure + out.maybe
    with np.errstate(all="ignore"):
        c = p.sum(0) / n
        dc = D * U * np.abs(p).sum(0) / n + U * np.abs(c) + TINY
        e = _sum_sq(p - c)
        moved = (2 * np.abs(p - c) * dc + dc * dc).sum(1)
        out.spread = e.sum()
        out.dspread = moved.sum() + (D + LEAF) * U * (e + moved).sum() + 9 * n * TINY
        e = _sum_sq(v)
        out.speed2, out.dspeed2 = e.sum(), (D + LEAF) * U * e.sum() + 6 * n * TINY
        m = v.sum(0)
        dm = D * U * np.abs(v).sum(0) + n * TINY
        out.momentum2 = (m * m).sum()
        out.dmomentum2 = (2 * np.abs(m) * dm + dm * dm).sum() + 3 * U * ((np.abs(m) + dm) ** 2).sum() + 5 * TINY
        e = _sum_sq(p - g)
        out.goal2, out.dgoal2 = e.sum(), (D + LEAF) * U * e.sum() + 9 * n * TINY
    return out


def accumulate(acc, term):
    """Q7: a record's reference with one more snapshot added (acc None: the cleared record)"""
    if acc is None:
        return types.SimpleNamespace(**vars(term))
    out = types.SimpleNamespace(steps=acc.steps + term.steps, nonfinite=acc.nonfinite + term.nonfinite, near_lo=acc.near_lo + term.near_lo,
                                near_hi=acc.near_hi + term.near_hi, maybe=acc.maybe + term.maybe, pairs=acc.pairs + term.pairs)
    for f in FLOATS:
        value = getattr(acc, f) + getattr(term, f)
        bound = getattr(acc, "d" + f) + getattr(term, "d" + f)
        setattr(out, f, value)
        setattr(out, "d" + f, bound + U * (abs(value) + bound))
    return out


def batch(pos, vel, radius_sq, goal, acc=None):
    """the references of a batch (B, n, 3) after scoring one snapshot, from the references `acc` or from cleared records"""
    return [accumulate(None if acc is None else acc[s], terms(pos[s], vel[s], radius_sq, goal)) for s in range(len(pos))]


def compare(case, ref, records):
    """The records (structured: near, spread, speed2, momentum2, goal2, steps, nonfinite) against batch()'s references: `nonfinite` and
    `steps` exactly (modulo 2^32), `near` within its interval, every held float within its bound.  Raises AssertionError naming
    case, scene, field, value, reference +- bound; returns the largest error / bound per float field."""
    worst = dict.fromkeys(FLOATS, 0.0)
    assert len(records) == len(ref), f"{case}: {len(records)} records against {len(ref)}"
    for s, (got, r) in enumerate(zip(records, ref)):
        for f in ("steps", "nonfinite"):
            assert int(got[f]) == getattr(r, f) & 0xFFFFFFFF, f"{case}: scene {s}, {f}: {int(got[f])} against {getattr(r, f)}"
        assert r.near_lo <= int(got["near"]) <= r.near_hi, \
            f"{case}: scene {s}, near: {int(got['near'])} against [{r.near_lo}, {r.near_hi}] of {r.pairs} pairs"
        for f in FLOATS:
            want, bound = getattr(r, f), getattr(r, "d" + f)
            if not (np.isfinite(want) and np.isfinite(bound)):
                continue
            err = abs(float(got[f]) - want)
            assert err <= bound, f"{case}: scene {s}, {f}: {float(got[f])!r} against {want!r} +- {bound:.3g} (off by {err:.3g})"
            if bound > 0:
                worst[f] = max(worst[f], err / bound)
    return worst
