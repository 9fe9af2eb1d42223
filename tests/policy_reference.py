"""A binary64 reference of what the scene batches' neural policy computes for an eye (include/nenbody.h P1-P6, DESIGN.md section
14.4), with a derived bound beside every value.

TEST INFRASTRUCTURE.  The kernel (nb_scenes_policy.inc) and the numpy restatement (tests/policy_restatement.py) were written from one
text, the steps P1-P8; this module is written from what the steps MEAN and shares nothing with them: it sits on the geometric
reference of the eye rows (tests/vision_reference.py) and imports no restatement.

  features   an eye's row is V.eye_rows(pos, vel, eyes, W, up, 90 / W, W, near, far) over the bodies of its own scene.  Counted from
             the row's first column, bin f of F covers columns [f W/F, (f + 1) W/F) and reports how NEAR the nearest thing in it is:
             x_f = 1 - d_f, d_f the least depth a column of the bin shows, 1 (x_f = 0) where it shows nothing.  The reference gives an
             interval: d_f <= hi, the least depth + bound over the bin's decided covered columns (1 where there is none: a further
             column can only lower the minimum), and d_f >= lo, the least depth - bound over the same columns, lowered to the
             eye's least `und_lo` (the nearest anything could be in an undecided cell) where the bin holds an undecided column.
             x_f is carried as midpoint and radius, plus 2^-24 for the rule's own subtraction (a bin that surely shows nothing
             is +0 exactly).
  network    t_j = b1_j + sum_f w1[f, j] x_f, h_j = max(t_j, 0), o_k = b2_k + sum_j w2[k, j] h_j, o_k limited to [-L, L], in
             binary64.  w1[f, j] is the policy's float f H + j -- bin-major --, then b1 (H), w2[k, j] at k H + j, b2 (2).
  actuation  f = v / |v|, s = (f x up) / |f x up| as V.basis forms them; o_0 is THRUST, along f, o_1 is TURN, along s (to the eye's
             right: `up` x f points left); a = o_0 f + o_1 s; v' = v + a dt; p' = p + v' (the NEW velocity).  A body with no heading
             coasts, a = 0: a zero velocity, a velocity along `up`, a non-finite velocity.

BOUNDS, first order, from magnitude sums, nothing tuned (U = 2^-24):
  a sum      of T terms, products included, in any order: (radius of the inputs) . |weights| + (T + 2) U S + 2^-149 a term, S the sum
             of the terms' largest magnitudes (|w| (|x| + radius)); T = F + 1 for t_j and H + 1 for o_k.  Each term passes at most
             T - 1 additions and one product's rounding; the 2 cover the second-order terms for T <= 257.  The 2^-149 is there
             because a binary32 product may be subnormal, where no relative bound holds: its error is at most half of 2^-149,
             and a sum in the subnormal range is exact.
  relu, limit  are monotone and 1-Lipschitz: the interval [o - bound, o + bound] passes through them end by end, so an output that
             surely lies beyond the limit is the limit exactly, and no eye is masked at a kink.
  actuation  ROUNDINGS counts the binary32 roundings on the path as vision_reference.ROUNDINGS does: f = normalize(v): the sum of
             three products (3), square root, reciprocal, scale = 6 -- every one relative, the squares being positive: 6 U |f_c|;
             s = normalize(f x up): the cross product 2, normalize 6 = 14 behind f's, on the magnitude sum sm_c = (|f| x |up|)_c /
             |f x up| -- and, since the norm inherits the cross product's cancellation, on |s_c| |sm| as well: 14 U (sm_c + |s_c|
             |sm|); a_c = (o_0 f_c) + (o_1 s_c): a product and the sum = 2, on |o_0 f_c| + |o_1 s_c|, beside |f_c| bound(o_0) +
             |s_c| bound(o_1) + |o_0| bound(f_c) + |o_1| bound(s_c); v' = v + a dt: 2, on |v_c| + |a_c| dt; p' = p + v': 1, on
             |p_c| + |v'_c|.  The longest path, to p', has 6 + 8 + 2 + 2 + 1 = 19.  Where |f x up| does not exceed its own bound
             the heading is UNDECIDED (binary32 may see none, or any): a = 0 with bound |o_0| + |o_1| a component.  The fixed
             cases hold no such body; a body moving exactly along (0, 0, 1) has f x up = 0 in either arithmetic.
An eye is COMPARED when both of its output bounds are at most MAX_OUTPUT_BOUND = 1/32, vision_reference.MAX_COLOUR_BOUND's value
(every case keeps its outputs within +-1): `compare` holds every eye to its intervals and reports the largest error / bound over
the compared ones.

Largest observed error / bound over tests/policy_reference_cases.py's fixed and 24 random cases (test_policy_score_reference_cpu.py
and test_gpu_policy_score_reference.py print them; on the MI355X the device's words ARE the restatement's on every case, so the
figures are one).  Over the compared eyes: x 1.0000, o 1.0000, v' 1.0000, p' 0.9998 -- at 1 by construction: a bin that holds an
undecided column, or one whose winner has a second edge in reach, has its depth AT an end of its interval (the bin is empty, or
shows the other edge), and where one such bin carries an eye's bound the outputs sit at theirs.  Over the compared eyes with no
such column ("sharp"): x 0.44, o 0.078, v' 0.47, p' 0.97 (p' = p + v' is one rounding of a sum whose bound is that one rounding's).
"""
import types

import numpy as np

import vision_reference as V

U = V.U
TINY = 2.0 ** -149
ROUNDINGS = dict(forward=6, side=8, accel=2, velocity=2, position=1)
MAX_OUTPUT_BOUND = V.MAX_COLOUR_BOUND
WORDS = ("x", "o", "vel", "pos")


def unpack(policy, features, hidden):
    """one policy's floats -> w1 (F, H) bin-major, b1 (H,), w2 (2, H), b2 (2,), binary64"""
    p = np.asarray(policy, np.float64).reshape(-1)
    assert len(p) == features * hidden + hidden + 2 * hidden + 2
    a, b, c = features * hidden, features * hidden + hidden, features * hidden + 3 * hidden
    return p[:a].reshape(features, hidden), p[a:b], p[b:c].reshape(2, hidden), p[c:]


def features_of(rows, features):
    """x_f of every eye of the reference rows: (midpoint (E, F), radius (E, F), seeing (E,): a bin surely shows somebody, sharp (E,):
    no column of the eye is undecided or has a second edge of its winner in reach)"""
    e, w = rows.ids.shape
    assert w % features == 0
    per = w // features
    shown = ~rows.und & (rows.ids != V.NONE)
    hi = np.where(shown, np.minimum(rows.depth + rows.ddepth, 1.0), 1.0).reshape(e, features, per).min(2)
    lo = np.where(shown, rows.depth - rows.ddepth, 1.0).reshape(e, features, per).min(2)
    open_bin = rows.und.reshape(e, features, per).any(2)
    lo = np.where(open_bin, np.minimum(lo, rows.und_lo.min(1, initial=np.inf)[:, None]), lo)
    lo = np.clip(lo, 0.0, 1.0)
    nothing = (lo == 1.0) & (hi == 1.0)
    x = 1.0 - 0.5 * (lo + hi)
    return x, 0.5 * (hi - lo) + np.where(nothing, 0.0, U), shown.any(1), ~(rows.und | rows.und_edge).any(1)


def _layer(x, dx, w, b):
    """b + x @ w for x (E, T), w (T, J): (value, bound) (E, J)"""
    reach = (np.abs(x) + dx) @ np.abs(w) + np.abs(b)
    terms = w.shape[0] + 1
    return b + x @ w, dx @ np.abs(w) + (terms + 2) * U * reach + terms * TINY


def network(x, dx, policy, features, hidden, limit):
    """(o (E, 2), bound (E, 2), t (E, H), bound of t, free (E, 2): the output's interval lies inside the limit; held (E, 2): it lies
    at or beyond it, so that the output is the limit exactly)"""
    w1, b1, w2, b2 = unpack(policy, features, hidden)
    t, dt = _layer(x, dx, w1, b1)
    lo, hi = np.maximum(t - dt, 0.0), np.maximum(t + dt, 0.0)
    o, do = _layer(0.5 * (lo + hi), 0.5 * (hi - lo), w2.T, b2)
    limit = float(limit)
    lo, hi = np.clip(o - do, -limit, limit), np.clip(o + do, -limit, limit)
    return 0.5 * (lo + hi), 0.5 * (hi - lo), t, dt, (np.abs(o) + do < limit), (np.abs(o) - do >= limit)


def actuation(pos, vel, up, o, do, dt):
    """P5-P6 for the records (E, 3) under outputs o +- do (E, 2): (p', bound, v', bound, heading (E,): 1 it has one, 0 it has none
    and coasts, -1 undecided)"""
    pos, vel = np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    n = len(pos)
    a, da, heading = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.int64)
    R = ROUNDINGS
    for i in range(n):
        b = V.basis(vel[i], up)
        if not (np.isfinite(b.f).all() and np.isfinite(b.s).all()):
            continue
        top = np.abs(o[i]) + do[i]
        cr = V._cross(b.f, np.asarray(up, np.float64))
        crm = V._cross_mag(np.abs(b.f), np.abs(np.asarray(up, np.float64)))
        if not np.sqrt(cr @ cr) > 2 * (R["forward"] + R["side"]) * U * np.sqrt(crm @ crm):
            heading[i], da[i] = -1, top.sum()
            continue
        heading[i] = 1
        df = R["forward"] * U * np.abs(b.f)
        ds = (R["forward"] + R["side"]) * U * (b.sm + np.abs(b.s) * np.sqrt(b.sm @ b.sm))
        a[i] = o[i, 0] * b.f + o[i, 1] * b.s
        reach = top[0] * np.abs(b.f) + top[1] * np.abs(b.s)
        da[i] = do[i, 0] * np.abs(b.f) + do[i, 1] * np.abs(b.s) + top[0] * df + top[1] * ds + R["accel"] * U * reach + 3 * TINY
    with np.errstate(all="ignore"):
        v1 = vel + a * dt
        dv = da * dt + R["velocity"] * U * (np.abs(vel) + (np.abs(a) + da) * dt) + TINY
        dv = np.where(heading[:, None] == 0, 0.0, dv)                                   # v + (+0) dt is v
        p1 = pos + v1
        dp = dv + R["position"] * U * (np.abs(pos) + np.abs(v1) + dv)
    return p1, dp, v1, dv, heading


def scene(pos, vel, eyes, width, up, near, far, policy, features, hidden, limit, dt):
    """the reference of the eyes `eyes` (body indices) of one scene under one policy"""
    fovy, aspect = float(np.float32(90.0) / np.float32(width)), float(width)
    rows = V.eye_rows(pos, vel, eyes, width, up, fovy, aspect, near, far)
    x, dx, seeing, sharp = features_of(rows, features)
    o, do, t, dt_, free, held = network(x, dx, policy, features, hidden, limit)
    eyes = np.asarray(eyes, np.int64)
    p1, dp, v1, dv, heading = actuation(np.asarray(pos)[eyes], np.asarray(vel)[eyes], up, o, do, float(dt))
    return types.SimpleNamespace(eyes=eyes, x=x, dx=dx, o=o, do=do, pos=p1, dpos=dp, vel=v1, dvel=dv, heading=heading, seeing=seeing,
                                 sharp=sharp, blind=~rows.touched.any(1), compared=(do <= MAX_OUTPUT_BOUND).all(1), on=(t - dt_ > 0).any(1),
                                 off=(t + dt_ <= 0).any(1), free=free.any(1), held=held.any(1),
                                 und_cells=int((rows.und & rows.touched).sum()), touched_cells=int(rows.touched.sum()))


def batch(pos, vel, eyes, width, up, near, far, policies, features, hidden, limit, dt):
    """the reference of a batch (B, n, 3): one namespace a scene; `policies` (P, floats), P = 1 or B"""
    policies = np.asarray(policies)
    return [scene(pos[s], vel[s], eyes, width, up, near, far, policies[s if len(policies) > 1 else 0], features, hidden, limit, dt)
            for s in range(len(pos))]


def compare(case, ref, x, o, pos1, vel1):
    """The features (B, n, F), outputs (B, n, 2) and the records after one step (B, n, 3) each -- None: not compared -- against the
    reference `ref` (batch()'s list): every value of every eye of the reference within its interval.  Raises AssertionError naming
    case, scene, eye, word, value, reference +- bound; returns the largest error / bound per output over the COMPARED eyes and, as
    "sharp " + word, over those of them with no undecided column and no column whose winner has a second edge in reach (either
    puts a bin's depth at an end of its interval by construction: the ratio there says nothing about the bound's room)."""
    worst = dict.fromkeys(WORDS + tuple("sharp " + w for w in WORDS), 0.0)
    for s, r in enumerate(ref):
        for name, got, want, bound in (("x", x, r.x, r.dx), ("o", o, r.o, r.do), ("vel", vel1, r.vel, r.dvel), ("pos", pos1, r.pos, r.dpos)):
            if got is None:
                continue
            g = np.asarray(got, np.float64)[s][r.eyes]
            assert g.shape == want.shape, f"{case}: {name} has shape {g.shape} an eye set, the reference {want.shape}"
            with np.errstate(all="ignore"):
                err = np.abs(g - want)
                ok = (err <= bound) | (~np.isfinite(want) & ((g == want) | (np.isnan(g) & np.isnan(want))))
            if not ok.all():
                e, k = np.argwhere(~ok)[0]
                raise AssertionError(f"{case}: scene {s}, eye {int(r.eyes[e])}, {name}[{int(k)}]: {g[e, k]!r} against {want[e, k]!r} +- "
                                     f"{bound[e, k]:.3g} (off by {err[e, k]:.3g}); {int((~ok).sum())} values differ, eye "
                                     f"{'compared' if r.compared[e] else 'not compared'}, heading {int(r.heading[e])}")
            live = r.compared[:, None] & (bound > 0) & np.isfinite(want)
            worst[name] = max(worst[name], float((err[live] / bound[live]).max(initial=0.0)))
            live &= r.sharp[:, None]
            worst["sharp " + name] = max(worst["sharp " + name], float((err[live] / bound[live]).max(initial=0.0)))
    return worst
