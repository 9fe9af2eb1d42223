"""numpy restatement of DESIGN.md section 14.5: the score of a scene (include/nenbody.h Q1-Q7).

TEST INFRASTRUCTURE.  The kernel (nenbody_amd/csrc/nb_scenes_score.inc) and this module implement the same rule independently; the GPU
tests compare every word.  Every float step is one binary32 operation on numpy float32 values in the order the rule writes it; the
tree sum is an explicit loop over the strides, vectorised over i and over the sums that share a tree.

``variant`` names a CONTROL ARM, a deliberate departure from the rule that tests/test_scenes_score_cpu.py shows its data can tell
from the rule (or, for the last two, cannot):
  "serial"        the sums in index order
  "adjacent"      a tree of adjacent pairs, u_{2i} + u_{2i+1}
  "float64"       the sums in binary64, rounded once
  "fma"           d2 and e_i with the products not rounded before they are added (binary64 holds a product exactly, so the sum is
                  rounded once to binary64 and once to binary32)
  "le"            <= in Q2
  "ordered"       ordered pairs counted
  "recip"         the centroid by multiplication with 1/n
  "skip_padding"  Q1 with every add whose right operand is padding left out
  "workgroup"     Q1 over the leaves of the kernel's workgroup: at least 64"""
import numpy as np

F32 = np.float32
DTYPE = np.dtype([("near", np.uint64), ("spread", F32), ("speed2", F32), ("momentum2", F32), ("goal2", F32), ("steps", np.uint32),
                  ("nonfinite", np.uint32)])
FLOATS = ("spread", "speed2", "momentum2", "goal2")
ARMS = ("serial", "adjacent", "float64", "fma", "le", "ordered", "recip", "skip_padding", "workgroup")


def pow2_at_least(n):
    p = 1
    while p < n:
        p *= 2
    return p


def tree(u, variant=None):
    """Q1 for the n leaves u (n,) or, k sums at once, (n, k): float32 () or (k,)"""
    u = np.array(u, F32)
    n = len(u)
    with np.errstate(all="ignore"):
        if variant == "serial":
            acc = u[0].copy()
            for i in range(1, n):
                acc = acc + u[i]
            return acc.astype(F32)
        if variant == "float64":
            return u.astype(np.float64).sum(0).astype(F32)
        if variant == "adjacent":
            while len(u) > 1:
                if len(u) % 2:
                    u = np.concatenate([u, np.zeros_like(u[:1])])
                u = (u[0::2] + u[1::2]).astype(F32)
            return u[0]
        p = pow2_at_least(n)
        if variant == "workgroup":
            p = max(p, 64)
        u = np.concatenate([u, np.zeros((p - n,) + u.shape[1:], F32)])
        live = n                                                                         # u_i is padding for i >= live
        stride = p // 2
        while stride >= 1:
            if variant == "skip_padding":
                m = max(0, min(stride, live - stride))                                   # i + stride < live
                u[:m] = u[:m] + u[stride:stride + m]
            else:
                u[:stride] = u[:stride] + u[stride:2 * stride]
            live = min(live, stride)
            stride //= 2
        return u[0]


def _sq3(a, b, c, variant=None):
    """((a a) + (b b)) + (c c)"""
    with np.errstate(all="ignore"):
        if variant == "fma":
            a64, b64, c64 = (np.asarray(x, F32).astype(np.float64) for x in (a, b, c))
            t = (a * a).astype(F32)
            t = (b64 * b64 + t.astype(np.float64)).astype(F32)
            return (c64 * c64 + t.astype(np.float64)).astype(F32)
        return ((a * a) + (b * b)) + (c * c)


def dist2(p, o, variant=None):
    """Q3's squared distance of the records p (n, 3) from the point o (3,)"""
    with np.errstate(all="ignore"):
        return _sq3(p[:, 0] - o[0], p[:, 1] - o[1], p[:, 2] - o[2], variant)


def pair_d2(pos, variant=None):
    """Q2's d2 for every ordered pair: (n, n) float32"""
    p = np.ascontiguousarray(pos, F32)
    with np.errstate(all="ignore"):
        return _sq3(p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1], p[:, None, 2] - p[None, :, 2], variant)


def near(pos, radius_sq, variant=None):
    d2 = pair_d2(pos, "fma" if variant == "fma" else None)
    with np.errstate(all="ignore"):
        hit = d2 <= F32(radius_sq) if variant == "le" else d2 < F32(radius_sq)           # a NaN compares false
    if variant == "ordered":
        np.fill_diagonal(hit, False)
        return int(hit.sum())
    return int(np.triu(hit, 1).sum())


def terms(pos, vel, radius_sq, goal, variant=None, near_of=None):
    """Q2-Q6 for one snapshot (n, 3), (n, 3): a DTYPE record with steps = 1.  near_of: Q2's count where the caller has it"""
    p, v = np.ascontiguousarray(pos, F32), np.ascontiguousarray(vel, F32)
    n = len(p)
    goal = np.asarray(goal, F32)
    order = variant if variant in ("serial", "adjacent", "float64", "skip_padding", "workgroup") else None
    form = "fma" if variant == "fma" else None
    out = np.zeros((), DTYPE)
    with np.errstate(all="ignore"):
        one = np.concatenate([p, _sq3(v[:, 0], v[:, 1], v[:, 2])[:, None], v, dist2(p, goal, form)[:, None]], 1)   # round one's 8 sums
        t = tree(one, order)
        c = t[:3] * (F32(1) / F32(n)) if variant == "recip" else t[:3] / F32(n)
        out["spread"] = tree(dist2(p, c.astype(F32), form), order)
        out["speed2"] = t[3]
        out["momentum2"] = ((t[4] * t[4]) + (t[5] * t[5])) + (t[6] * t[6])
        out["goal2"] = t[7]
    out["near"] = near(p, radius_sq, variant) if near_of is None else near_of
    out["steps"] = 1
    out["nonfinite"] = int((~np.isfinite(np.concatenate([p, v], 1))).any(1).sum())
    return out


def accumulate(acc, term):
    """Q7: the record acc (DTYPE, ()) with one snapshot's terms added"""
    out = np.array(acc, DTYPE)
    out["near"] = np.uint64(int(acc["near"]) + int(term["near"]))
    with np.errstate(all="ignore"):
        for f in FLOATS:
            out[f] = F32(acc[f]) + F32(term[f])
    out["steps"] = np.uint32((int(acc["steps"]) + int(term["steps"])) & 0xFFFFFFFF)
    out["nonfinite"] = np.uint32((int(acc["nonfinite"]) + int(term["nonfinite"])) & 0xFFFFFFFF)
    return out


def batch(pos, vel, radius_sq, goal, variant=None, acc=None):
    """the records of a batch (B, n, 3) after scoring one snapshot, from `acc` (B,) or from cleared records"""
    acc = np.zeros(len(pos), DTYPE) if acc is None else acc
    return np.stack([accumulate(acc[s], terms(pos[s], vel[s], radius_sq, goal, variant)) for s in range(len(pos))])


def same(got, want):
    """every word of every record equal; a float field that is a NaN is met by a NaN (the rule leaves its sign and payload open)"""
    g, w = np.ascontiguousarray(got, DTYPE).reshape(-1), np.ascontiguousarray(want, DTYPE).reshape(-1)
    if g.shape != w.shape:
        return False
    ok = all((g[f] == w[f]).all() for f in ("near", "steps", "nonfinite"))
    for f in FLOATS:
        ok = ok and bool(((g[f].view(np.uint32) == w[f].view(np.uint32)) | (np.isnan(g[f]) & np.isnan(w[f]))).all())
    return ok
