"""numpy restatement of DESIGN.md section 14.8: a recurrent policy with per-body memory (include/nenbody.h R1-R5, R8).

TEST INFRASTRUCTURE.  The kernel (nenbody_amd/csrc/nb_scenes_policy_recurrent.inc) and this module implement the same rule
independently; the GPU tests compare every word.  Every arithmetic step is one binary32 operation on numpy float32 values, in the
order the rule writes it; the chain of R3 is two explicit sequential loops, over f and then over r, vectorised over the eyes only.
P2 (the features), P4 (the outputs) and P5-P6 (the motion) are policy_restatement's, imported and not copied.

``variant`` names a CONTROL ARM, a deliberate departure from the rule that tests/test_scenes_policy_recurrent_cpu.py shows its data
can tell from the rule:
  "mem_first"       the memory terms of R3 in front of the feature terms
  "reverse_r"       r from H-1 down to 0
  "fma_mem"         the memory chain fused: the product is not rounded before it is added
  "wr_hidden_major" wr read as wr[j H + r]
  "no_mem_limit"    m' = h, R4's limit dropped
  "o_from_m"        the outputs from m' instead of h
  "coast_keeps"     the memory of a body that coasts under P5 is not written
  "stale"           the memory read after it was overwritten: the chain of step t runs over the m' of step t"""
import numpy as np

import located_restatement as L
import policy_restatement as P

F32 = np.float32
VARIANTS = ("mem_first", "reverse_r", "fma_mem", "wr_hidden_major", "no_mem_limit", "o_from_m", "coast_keeps", "stale")


def policy_recurrent_floats(features, hidden):
    """R1"""
    if not (1 <= features <= P.MAX_FEATURES and 1 <= hidden <= P.MAX_HIDDEN):
        return 0
    return features * hidden + hidden * hidden + hidden + 2 * hidden + 2


def pack(w1, wr, b1, w2, b2):
    """w1 (F, H), wr (H, H) source-major, b1 (H,), w2 (2, H), b2 (2,) -> one recurrent policy in the library's layout (R1)"""
    return np.concatenate([np.asarray(a, F32).reshape(-1) for a in (w1, wr, b1, w2, b2)])


def unpack(policy, features, hidden):
    p = np.ascontiguousarray(policy, F32).reshape(-1)
    assert len(p) == policy_recurrent_floats(features, hidden)
    cuts = np.cumsum([features * hidden, hidden * hidden, hidden, 2 * hidden])
    w1, wr, b1, w2, b2 = np.split(p, cuts)
    return w1.reshape(features, hidden), wr.reshape(hidden, hidden), b1, w2.reshape(2, hidden), b2


def feedforward(policy, features, hidden):
    """the P-rule policy (w1, b1, w2, b2) of a recurrent one (R6)"""
    w1, _, b1, w2, b2 = unpack(policy, features, hidden)
    return P.pack(w1, b1, w2, b2)


def _fused(t, w, x):
    return (t.astype(np.float64) + w.astype(np.float64) * x.astype(np.float64)).astype(F32)


def hidden_of(x, mem, w1, wr, b1, variant=None):
    """R3 for x (E, F) and mem (E, H): h (E, H).  Both sums are sequential."""
    e, features = x.shape
    hidden = mem.shape[1]
    mem = np.ascontiguousarray(mem, F32)
    weight = (lambda r: wr[None, :, r]) if variant == "wr_hidden_major" else (lambda r: wr[None, r, :])
    with np.errstate(all="ignore"):
        t = np.tile(np.asarray(b1, F32), (e, 1))

        def over_features(t):
            for f in range(features):
                t = t + (w1[None, f, :] * x[:, f, None])
            return t

        def over_memory(t):
            for r in (range(hidden - 1, -1, -1) if variant == "reverse_r" else range(hidden)):
                t = _fused(t, weight(r), mem[:, r, None]) if variant == "fma_mem" else t + (weight(r) * mem[:, r, None])
            return t

        t = over_features(over_memory(t)) if variant == "mem_first" else over_memory(over_features(t))
        return np.where(t > 0, t, F32(0)).astype(F32)                                    # a NaN gives +0


def memory_of(h, memory_limit, variant=None):
    """R4"""
    s = F32(memory_limit)
    if variant == "no_mem_limit":
        return h.astype(F32)
    return np.where(h > s, s, h).astype(F32)


def observe(ids, depth, mem, policy, features, hidden, limit, memory_limit, variant=None):
    """R8 for the (E, W) rows and the (E, H) memory of eyes that share one policy: (x (E, F), o (E, 2), m' (E, H))"""
    w1, wr, b1, w2, b2 = unpack(policy, features, hidden)
    x = P.features_of_rows(ids, depth, features)
    h = hidden_of(x, mem, w1, wr, b1, variant)
    if variant == "stale":
        h = hidden_of(x, memory_of(h, memory_limit), w1, wr, b1)
    m = memory_of(h, memory_limit, variant)
    return x, P.outputs_of(m if variant == "o_from_m" else h, w2, b2, limit), m


def batch(rows_of, pos, vel, mem, policies, features, hidden, limit, memory_limit, up, dt=F32(0.1), variant=None):
    """One step of a batch (B, n, 3) with memory (B, n, H): rows_of(s, pos_s, vel_s) gives scene s's (ids, depth) rows (P1); policies
    (P, floats), P = 1 or B.  Returns (x (B, n, F), o (B, n, 2), m' (B, n, H), positions, velocities)."""
    policies = np.ascontiguousarray(policies, F32).reshape(-1, policy_recurrent_floats(features, hidden))
    assert len(policies) in (1, len(pos))
    mem = np.ascontiguousarray(mem, F32)
    assert mem.shape == pos.shape[:2] + (hidden,)
    out = []
    for s in range(len(pos)):
        ids, depth = rows_of(s, pos[s], vel[s])
        x, o, m = observe(ids, depth, mem[s], policies[s if len(policies) > 1 else 0], features, hidden, limit, memory_limit, variant)
        if variant == "coast_keeps":
            f, sd = L.axes(np.ascontiguousarray(vel[s], F32), up)
            pushed = np.isfinite(f).all(1) & np.isfinite(sd).all(1)
            m = np.where(pushed[:, None], m, mem[s]).astype(F32)
        out.append((x, o, m) + P.step(pos[s], vel[s], o, up, dt))
    return tuple(np.stack([r[a] for r in out]) for a in range(5))


def rollout(rows_of, pos, vel, mem, policies, features, hidden, limit, memory_limit, up, steps, dt=F32(0.1), variant=None):
    """`steps` steps with the memory carried: the list of batch()'s tuples, one a step"""
    out = []
    for _ in range(steps):
        out.append(batch(rows_of, pos, vel, mem, policies, features, hidden, limit, memory_limit, up, dt, variant))
        mem, pos, vel = out[-1][2], out[-1][3], out[-1][4]
    return out
