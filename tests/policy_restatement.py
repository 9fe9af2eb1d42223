"""numpy restatement of DESIGN.md section 14.4: a neural policy over each body's eye row (include/nenbody.h P1-P6).

TEST INFRASTRUCTURE.  The kernel (nenbody_amd/csrc/nb_scenes_policy.inc) and this module implement the same rule independently; the
GPU tests compare every word.  Every arithmetic step is one binary32 operation on numpy float32 values, in the order the rule writes
it; the two sums are explicit sequential loops over f and over j, vectorised over the eyes only.  It sits on the rows of
eyes_restatement (P1) and on located_restatement.axes (L3, for P5); a batch is scenes_restatement's: a loop over the scenes.

``variant`` names a CONTROL ARM, a deliberate departure from the rule that tests/test_scenes_policy_cpu.py shows its data can tell
from the rule: "fma" (the product is not rounded before it is added: binary64 holds the product exactly, so the sum is rounded
once to binary64 and once to binary32), "reverse_f", "reverse_j", "max" (the farthest depth of a bin instead of the nearest),
"no_relu", "no_limit", "no_guard"."""
import numpy as np

import located_restatement as L

F32 = np.float32
NONE = 0xFFFFFFFF
ONE_BITS = np.uint32(0x3F800000)
MAX_FEATURES, MAX_HIDDEN = 256, 64


def same(got, want):
    """every word equal, a NaN met by a NaN"""
    g, w = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    return bool(((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))).all())


def policy_floats(features, hidden):
    if not (1 <= features <= MAX_FEATURES and 1 <= hidden <= MAX_HIDDEN):
        return 0
    return features * hidden + hidden + 2 * hidden + 2


def pack(w1, b1, w2, b2):
    """w1 (F, H), b1 (H,), w2 (2, H), b2 (2,) -> one policy in the library's layout"""
    return np.concatenate([np.asarray(a, F32).reshape(-1) for a in (w1, b1, w2, b2)])


def unpack(policy, features, hidden):
    p = np.ascontiguousarray(policy, F32).reshape(-1)
    assert len(p) == policy_floats(features, hidden)
    cuts = np.cumsum([features * hidden, hidden, 2 * hidden])
    w1, b1, w2, b2 = np.split(p, cuts)
    return w1.reshape(features, hidden), b1, w2.reshape(2, hidden), b2


def features_of_rows(ids, depth, features, variant=None):
    """P2 for (E, W) rows: x (E, F) float32"""
    ids = np.ascontiguousarray(ids, np.uint32)
    bits = np.ascontiguousarray(depth, F32).view(np.uint32)
    e, w = ids.shape
    assert w % features == 0
    seen = (ids != np.uint32(NONE)).reshape(e, features, w // features)
    bits = bits.reshape(e, features, w // features)
    if variant == "max":
        d = np.where(seen, bits, np.uint32(0)).max(2)
        d = np.where(seen.any(2), d, ONE_BITS)
    else:
        d = np.where(seen, bits, ONE_BITS).min(2)                                        # a candidate's bits are below 1.0f's
    return (F32(1) - d.astype(np.uint32).view(F32)).astype(F32)


def _fused(t, w, x):
    return (t.astype(np.float64) + w.astype(np.float64) * x.astype(np.float64)).astype(F32)


def hidden_of(x, w1, b1, variant=None):
    """P3 for x (E, F): h (E, H).  The sum over f is sequential."""
    e, features = x.shape
    with np.errstate(all="ignore"):
        t = np.tile(np.asarray(b1, F32), (e, 1))
        order = range(features - 1, -1, -1) if variant == "reverse_f" else range(features)
        for f in order:
            if variant == "fma":
                t = _fused(t, w1[None, f, :], x[:, f, None])
            else:
                t = t + (w1[None, f, :] * x[:, f, None])
        if variant == "no_relu":
            return t.astype(F32)
        return np.where(t > 0, t, F32(0)).astype(F32)                                    # a NaN gives +0


def outputs_of(h, w2, b2, limit, variant=None):
    """P4 for h (E, H): o (E, 2).  The sum over j is sequential."""
    e, hidden = h.shape
    limit = F32(limit)
    with np.errstate(all="ignore"):
        o = np.tile(np.asarray(b2, F32), (e, 1))
        order = range(hidden - 1, -1, -1) if variant == "reverse_j" else range(hidden)
        for j in order:
            if variant == "fma":
                o = _fused(o, w2[None, :, j], h[:, j, None])
            else:
                o = o + (w2[None, :, j] * h[:, j, None])
        if variant != "no_limit":
            o = np.where(o < -limit, -limit, np.where(o > limit, limit, o))             # a NaN passes through
    return o.astype(F32)


def observe(ids, depth, policy, features, hidden, limit, variant=None):
    """P2-P4 for the (E, W) rows of eyes that share one policy: (x (E, F), o (E, 2))"""
    w1, b1, w2, b2 = unpack(policy, features, hidden)
    x = features_of_rows(ids, depth, features, variant)
    return x, outputs_of(hidden_of(x, w1, b1, variant), w2, b2, limit, variant)


def accel(vel, up, o, variant=None):
    """P5 for velocity records (E, 3) and outputs (E, 2): a (E, 3)"""
    f, s = L.axes(vel, up)
    with np.errstate(all="ignore"):
        a = (o[:, 0, None] * f) + (o[:, 1, None] * s)
    if variant == "no_guard":
        return a.astype(F32)
    ok = np.isfinite(f).all(1) & np.isfinite(s).all(1)
    return np.where(ok[:, None], a, F32(0)).astype(F32)


def step(pos, vel, o, up, dt=F32(0.1), variant=None):
    """P5-P6 for the bodies of one scene: (positions, velocities)"""
    pos, vel = np.ascontiguousarray(pos, F32), np.ascontiguousarray(vel, F32)
    a = accel(vel, up, o, variant)
    with np.errstate(all="ignore"):
        v = vel + a * F32(dt)                                                            # main.rs:434
        p = v + pos                                                                      # main.rs:436
    return p.astype(F32), v.astype(F32)


def batch(rows_of, pos, vel, policies, features, hidden, limit, up, dt=F32(0.1), variant=None):
    """One step of a batch (B, n, 3): rows_of(s, pos_s, vel_s) gives scene s's (ids, depth) rows (P1); policies (P, floats), P = 1 or
    B.  Returns (x (B, n, F), o (B, n, 2), positions, velocities)."""
    policies = np.ascontiguousarray(policies, F32).reshape(-1, policy_floats(features, hidden))
    assert len(policies) in (1, len(pos))
    out = []
    for s in range(len(pos)):
        ids, depth = rows_of(s, pos[s], vel[s])
        x, o = observe(ids, depth, policies[s if len(policies) > 1 else 0], features, hidden, limit, variant)
        out.append((x, o) + step(pos[s], vel[s], o, up, dt, variant))
    return tuple(np.stack([r[a] for r in out]) for a in range(4))
