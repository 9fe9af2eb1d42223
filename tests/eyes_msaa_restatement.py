"""numpy float32 restatement of the 8-sample eye rule on top of eyes_restatement.py and
eyes_colour_restatement.py: what the reference's eye targets hold when every column is rendered through 8 samples and resolved
(msaa_samples = 8, src/main.rs:652; sample_count, :263; resolve_target, :547, :611).

TEST INFRASTRUCTURE.  The kernel (nenbody_amd/csrc/nb_eyes_msaa.inc) and this module implement the same rule independently; the
GPU tests compare them bit for bit.  Every step is one binary32 operation on numpy float32 arrays, in the order the rule writes it.
"""
import numpy as np

import eyes_colour_restatement as K
import eyes_restatement as R

F = np.float32
SAMPLES = 8
# M1: the x coordinates of Vulkan's standard 8-sample pattern, in sample-index order
OFFSETS = np.array([9, 7, 13, 5, 3, 1, 11, 15], np.float32) / F(16)


def _sample_keys(cams, world, first, width, see_self, stats=None):
    """M2: steps 3-5 with xc replaced by x_k = c + o_k.  (E, width, 8) uint64 keys, R.EMPTY where no candidate covers the sample."""
    E, n = len(cams), len(world)
    keep, xs0, d0, xs1, d1 = R.segments(cams, world, width, stats)
    if not see_self:
        own = first + np.arange(E)
        ok = own < n
        keep[np.arange(E)[ok], own[ok], :] = False
    with np.errstate(all="ignore"):
        xa = np.where(xs0 <= xs1, xs0, xs1)
        xb = np.where(xs0 <= xs1, xs1, xs0)
        keep &= xa <= xb                                  # a NaN end covers nothing
        e_idx, j_idx, _ = np.nonzero(keep)
        xa, xb = xa[keep], xb[keep]
        # the columns that can hold a covered sample, a superset (c < x_k < c + 1): the exact test below decides
        lo = np.clip(np.floor(np.maximum(xa.astype(np.float64), -4.0)) - 1, 0, width).astype(np.int64)
        hi = np.clip(np.ceil(np.minimum(xb.astype(np.float64), width + 4.0)) + 1, 0, width).astype(np.int64)
    keys = np.full(E * width * SAMPLES, R.EMPTY, np.uint64)
    span = np.maximum(hi - lo, 0)
    total = int(span.sum())
    if total == 0:
        return keys.reshape(E, width, SAMPLES)
    seg = np.repeat(np.arange(len(lo)), span)
    col = np.arange(total) - np.repeat(np.cumsum(span) - span, span) + lo[seg]
    x = col.astype(np.float32)[:, None] + OFFSETS[None, :]                 # exact for c < 4096; (total, 8)
    s0, s1 = xs0[keep][seg][:, None], xs1[keep][seg][:, None]
    e0, e1 = d0[keep][seg][:, None], d1[keep][seg][:, None]
    with np.errstate(all="ignore"):
        covered = (xa[seg][:, None] <= x) & (x < xb[seg][:, None])
        t = (x - s0) / (s1 - s0)
        d = e0 + t * (e1 - e0)
        cand = covered & (d < F(1))
        far = covered & (d >= F(1))
        d = np.where(d > 0, d, F(0)).astype(np.float32)    # !(d > 0) -> +0
    if stats is not None:
        stats["rejected_far"] = stats.get("rejected_far", 0) + int(far.sum())
        stats["widest"] = max(stats.get("widest", 0), int(np.bincount(seg[cand.any(1)], minlength=1).max()))
    key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j_idx[seg].astype(np.uint64)[:, None]
    slot = ((e_idx[seg] * width + col) * SAMPLES)[:, None] + np.arange(SAMPLES)[None, :]
    np.minimum.at(keys, slot[cand], key[cand])
    return keys.reshape(E, width, SAMPLES)


def winning_fragments(cams, world, e_idx, c_idx, x, j, want, width, skin):
    """M3 and M4 for m samples: sample i of eye e_idx[i] (an index into cams) lies at x[i] in column c_idx[i] and holds body j[i]
    at depth bits want[i].  Returns (edge (m,) -- the first of the body's edges 0, 1, 2 that covers x, is a candidate and gives the
    depth bits; -1: none --, the colour (m, 4) of the fragment (c, j, edge) shaded at the column centre, and whether that centre
    lies outside the edge's span: the attribute is extrapolated)."""
    th, tw = skin.shape[:2]
    m = len(j)
    C, wv = cams[e_idx], world[j]                                              # (m, 4, 4) [k] = column k; (m, 3, 4)
    with np.errstate(all="ignore"):
        P = ((C[:, 0, None, :] * wv[:, :, 0, None] + C[:, 1, None, :] * wv[:, :, 1, None]) + C[:, 2, None, :] * wv[:, :, 2, None]) \
            + C[:, 3, None, :] * wv[:, :, 3, None]                             # step 1, (m, 3, 4)
    xc = c_idx.astype(np.float32) + F(0.5)
    edge = np.full(m, -1, np.int64)
    s = np.zeros(m, np.float32)
    extra = np.zeros(m, bool)
    for k, (a, b) in enumerate(R.EDGES):                                       # M3: the first edge in draw order
        keep, t_in, t_out, w0, w1, xs0, xs1, d0, d1 = K._clip_edge(P[:, a], P[:, b], width)
        with np.errstate(all="ignore"):
            xa, xb = np.where(xs0 <= xs1, xs0, xs1), np.where(xs0 <= xs1, xs1, xs0)
            dx = xs1 - xs0
            tk = (x - xs0) / dx
            d = d0 + tk * (d1 - d0)
            ok = keep & (xa <= x) & (x < xb) & (d < F(1))
            d = np.where(d > 0, d, F(0)).astype(np.float32)
            ok &= (d.view(np.uint32) == want) & (edge < 0)
            t = (xc - xs0) / dx                                                # M4: the fragment is shaded at the column centre
            s0 = np.where(t_in > 0, t_in, F(0))                                # step 7
            s1 = np.where(t_out < 1, t_out, F(1))
            i0, i1 = F(1) / w0, F(1) / w1
            a0, a1 = s0 * i0, s1 * i1
            num = a0 + t * (a1 - a0)
            den = i0 + t * (i1 - i0)
            sk = num / den
            sk = np.where(sk > 0, sk, F(0))
            sk = np.where(sk > 1, F(1), sk)
            centre = (xa <= xc) & (xc < xb)
        edge[ok], s[ok] = k, sk[ok]
        extra |= ok & ~centre
    out = np.empty((m, 4), np.float32)
    out[:] = K.CLEAR
    hit = edge >= 0
    one_minus = F(1) - s                                                       # step 8
    u = np.select([edge == 0, edge == 1], [np.zeros(m, np.float32), s], one_minus)
    v = np.select([edge == 0, edge == 1], [s, np.ones(m, np.float32)], one_minus)
    ix = np.minimum(tw - 1, np.floor(u * F(tw)).astype(np.int64))              # step 9
    iy = np.minimum(th - 1, np.floor(v * F(th)).astype(np.int64))
    tex = skin[iy, ix]
    du, dv = u - F(0.5), v - F(0.5)                                            # step 10
    m2 = du * du + dv * dv
    f = F(1) - m2
    out[hit, :3] = (tex[:, :3] * f[:, None])[hit]
    out[hit, 3] = 1
    return edge, out, extra


def msaa(cams, inst, first, width, see_self=False, skin=None, chunk=8, stats=None):
    """The rule M1-M5 for eyes first .. first + len(cams) - 1 over every body of `inst`; skin as eyes_colour_restatement.colour.
    Returns (ids8 uint32 (E, width, 8), depth8 float32 (E, width, 8), rgba float32 (E, width, 4), bgra8 uint32 (E, width)).
    `stats`, a dict, collects over calls: "covered_hist" (9 entries: columns by their number of covered samples), "two_bodies"
    (columns whose samples name two bodies or more), "two_bodies_full" (those of them with all eight samples covered),
    "empty_centre" (columns with a covered sample whose one-sample rule at the centre finds nothing), "extrapolated" (samples whose
    fragment is shaded outside its edge's span), "edge" (samples per winning edge), "columns", what eyes_restatement.segments
    counts, "rejected_far" (covered samples of a segment whose depth is >= 1: no candidate) and "widest" (the most columns with a
    candidate sample of one segment); and of the last call "edge8", (E, width, 8), the winning edge per sample, -1 where empty."""
    cams = np.ascontiguousarray(cams, np.float32).reshape(-1, 4, 4)
    skin = K.WHITE if skin is None else np.ascontiguousarray(skin, np.float32)
    world = R.world_vertices(inst)
    E = len(cams)
    ids8 = np.empty((E, width, SAMPLES), np.uint32)
    depth8 = np.empty((E, width, SAMPLES), np.float32)
    rgba = np.empty((E, width, 4), np.float32)
    edge8 = np.full((E, width, SAMPLES), -1, np.int8)
    extrapolated = 0
    for e0 in range(0, E, chunk):
        e1 = min(E, e0 + chunk)
        keys = _sample_keys(cams[e0:e1], world, first + e0, width, see_self, stats)
        none = keys == R.EMPTY
        ids8[e0:e1] = np.where(none, np.uint32(R.NONE), (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        depth8[e0:e1] = np.where(none, F(1), (keys >> np.uint64(32)).astype(np.uint32).view(np.float32))
        a = np.empty((e1 - e0, width, SAMPLES, 4), np.float32)                 # M5: a_k
        a[:] = K.CLEAR
        e_idx, c_idx, k_idx = np.nonzero(~none)
        if len(e_idx):
            x = c_idx.astype(np.float32) + OFFSETS[k_idx]
            j = ids8[e0:e1][e_idx, c_idx, k_idx].astype(np.int64)
            want = depth8[e0:e1][e_idx, c_idx, k_idx].view(np.uint32)
            edge, col, extra = winning_fragments(cams[e0:e1], world, e_idx, c_idx, x, j, want, width, skin)
            assert (edge >= 0).all(), "a resolved sample without a winning edge"
            a[e_idx, c_idx, k_idx] = col
            edge8[e0:e1][e_idx, c_idx, k_idx] = edge
            extrapolated += int(extra.sum())
        with np.errstate(all="ignore"):
            rgba[e0:e1] = (((a[:, :, 0] + a[:, :, 1]) + (a[:, :, 2] + a[:, :, 3])) + ((a[:, :, 4] + a[:, :, 5]) + (a[:, :, 6] + a[:, :, 7]))) * F(0.125)
    if stats is not None:
        covered = (ids8 != R.NONE)
        cnt = covered.sum(-1)
        lo = np.where(covered, ids8, np.uint32(R.NONE)).min(-1)
        hi = np.where(covered, ids8, np.uint32(0)).max(-1)
        two = (cnt > 0) & (lo != hi)
        centre_ids, _ = R.eyes(cams, inst, first, width, see_self, chunk)
        stats["covered_hist"] = stats.get("covered_hist", np.zeros(9, np.int64)) + np.bincount(cnt.ravel(), minlength=9)
        stats["two_bodies"] = stats.get("two_bodies", 0) + int(two.sum())
        stats["two_bodies_full"] = stats.get("two_bodies_full", 0) + int((two & (cnt == SAMPLES)).sum())
        stats["empty_centre"] = stats.get("empty_centre", 0) + int(((centre_ids == R.NONE) & (cnt > 0)).sum())
        stats["extrapolated"] = stats.get("extrapolated", 0) + extrapolated
        stats["edge"] = stats.get("edge", np.zeros(3, np.int64)) + np.bincount(edge8[edge8 >= 0].astype(np.int64), minlength=3)
        stats["columns"] = stats.get("columns", 0) + E * width
        stats["edge8"] = edge8
    return ids8, depth8, rgba, K.pack_bgra8(rgba)
