"""numpy float32 restatement of the 8-sample frame rule on top of frame_restatement.py and
eyes_colour_restatement.py: what the reference's display pass leaves in its W x H target when every pixel is rendered through 8
samples and resolved (msaa_samples = 8, src/main.rs:652; the display target, :685-690; its resolve, :545-548, :948-960).

TEST INFRASTRUCTURE.  The kernels (nenbody_amd/csrc/nb_frame_msaa.inc) and this module implement the same rule independently; the
GPU tests compare them bit for bit.  Every step is one binary32 operation on numpy float32 arrays, in the order the rule writes it.
"""
import numpy as np

import eyes_colour_restatement as K
import eyes_restatement as R
import frame_restatement as FR

F = np.float32
SAMPLES = 8
# FM1: Vulkan's standard 8-sample pattern in sample-index order
OX = np.array([9, 7, 13, 5, 3, 1, 11, 15], np.float32) / F(16)
OY = np.array([5, 11, 9, 3, 13, 7, 15, 1], np.float32) / F(16)


def _sample(e, idx, m, k, W, far=None):
    """FM2 for sample k of step m along the major axis of edge idx (arrays that broadcast against each other): (ok, pixel, d, t_c,
    centre) -- ok: the sample is tried, lands in a pixel and its depth is a candidate; pixel = row * W + column; d after the clamp
    to +0; t_c: FM4's parameter of the centre of step m; centre: that centre lies inside the edge's span.  far, a list, receives
    the samples that land in a pixel with a depth >= 1: no candidate."""
    with np.errstate(all="ignore"):
        xm = e["xmajor"][idx]
        oa, ob = np.where(xm, OX[k], OY[k]), np.where(xm, OY[k], OX[k])
        a0, a1, da = e["a0"][idx], e["a1"][idx], e["da"][idx]
        amin, amax = np.where(a0 <= a1, a0, a1), np.where(a0 <= a1, a1, a0)
        a = (m.astype(F) + oa).astype(F)                                                     # exact
        ok = (amin <= a) & (a < amax)
        t = (a - a0) / da
        o = e["b0"][idx] + t * e["db"][idx]
        q = (F(0.5) - ob).astype(F)                                                          # exact
        ek = o + q
        ok = ok & (ek >= 0) & (ek < e["blim"][idx])                                          # a NaN covers nothing
        d = e["d0"][idx] + t * (e["d1"][idx] - e["d0"][idx])
        if far is not None:
            far.append(ok & (d >= F(1)))
        ok = ok & (d < F(1))
        d = np.where(d > 0, d, F(0)).astype(F)                                               # !(d > 0) -> +0
        f = np.where(ok, np.floor(ek), 0).astype(np.int64)
        mc = m.astype(F) + F(0.5)
        t_c = (mc - a0) / da
        centre = (amin <= mc) & (mc < amax)
    pixel = np.where(xm, f * W + m, m * W + f)
    return ok, pixel, d, t_c, centre


def centre_edges(e, ids, depth, W):
    """F6's edge for every pixel of frame_restatement.frame's (ids, depth): (H, W) int8, -1 where the pixel is empty."""
    H = ids.shape[0]
    edge = np.full(W * H, -1, np.int8)
    p = np.nonzero(ids.ravel() != R.NONE)[0]
    j = ids.ravel()[p].astype(np.int64)
    want = depth.ravel()[p].view(np.uint32)
    row, col = p // W, p % W
    found = np.full(len(p), -1, np.int8)
    for k in range(3):
        idx = 3 * j + k
        ok, _, pixel, d = FR._steps(e, idx, np.where(e["xmajor"][idx], col, row), W)
        ok &= e["keep"][idx] & (pixel == p) & (d.view(np.uint32) == want) & (found < 0)
        found[ok] = k
    edge[p] = found
    return edge.reshape(H, W)


def frame_msaa(cam, inst, W, H, skin=None, stats=None):
    """The rule FM1-FM5 for one camera over every body of `inst`; skin: (th, tw, 4) linear float32, row 0 first (None: 1 x 1 white).
    Returns (ids8 uint32 (H, W, 8), depth8 float32 (H, W, 8), rgba float32 (H, W, 4), bgra8 uint32 (H, W)); row 0 is the top.
    `stats`, a dict, receives: sample "writes" (candidates), "covered_hist" (9 entries: pixels by their number of covered samples),
    "two_bodies" (pixels whose samples name two bodies or more), "empty_centre" (pixels with a covered sample where the one-sample
    rule F1-F6 finds nothing), "centre_only" (pixels the one-sample rule covers that have no covered sample), "extrapolated"
    (samples whose fragment is shaded at a centre outside its edge's span), "edge" (samples per winning edge), "edge8" ((H, W, 8),
    the winning edge per sample, -1 where empty), "one" ((H, W) bool: all eight samples covered by one (body, edge), which is
    also the one-sample rule's winner and edge there), "cut", "w_dropped" (as frame_restatement.frame's), "rejected_far" (samples
    that land in a pixel with a depth >= 1) and "longest_x" / "longest_y" (the most major-axis steps with a candidate sample of one
    x-major / y-major edge)."""
    inst = np.ascontiguousarray(inst, F).reshape(-1, 4, 4)
    skin = K.WHITE if skin is None else np.ascontiguousarray(skin, F)
    th, tw = skin.shape[:2]
    n = len(inst)
    e = FR.edges(cam, inst, W, H)
    keys = np.full(W * H * SAMPLES, R.EMPTY, np.uint64)
    ks = np.arange(SAMPLES)
    writes = rejected_far = longest_x = longest_y = 0
    with np.errstate(all="ignore"):
        amin, amax = np.minimum(e["a0"], e["a1"]), np.maximum(e["a0"], e["a1"])              # (a NaN end: NaN, dropped next)
        live = e["keep"] & (amin <= amax)
        alim = np.where(e["xmajor"], W, H).astype(np.float64)
        # the steps that can hold a tried sample, a superset (m < a_k < m + 1): the exact test in _sample decides
        lo = np.clip(np.floor(np.maximum(amin.astype(np.float64), -4.0)) - 1, 0, alim)
        hi = np.clip(np.ceil(np.minimum(amax.astype(np.float64), alim + 4.0)) + 1, 0, alim)
    lo, hi = np.where(live, lo, 0).astype(np.int64), np.where(live, hi, 0).astype(np.int64)
    span = np.maximum(hi - lo, 0)
    total = int(span.sum())
    if total:
        idx = np.repeat(np.arange(3 * n), span)
        m = np.arange(total) - np.repeat(np.cumsum(span) - span, span) + lo[idx]
        far = []
        ok, pixel, d, _, _ = _sample(e, idx[:, None], m[:, None], ks[None, :], W, far)       # FM2
        rejected_far = int(far[0].sum())
        per_edge = np.bincount(idx[ok.any(1)], minlength=3 * n)                              # steps with a candidate sample
        longest_x, longest_y = int(per_edge[e["xmajor"]].max(initial=0)), int(per_edge[~e["xmajor"]].max(initial=0))
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (idx // 3).astype(np.uint64)[:, None]
        slot = pixel * SAMPLES + ks[None, :]
        np.minimum.at(keys, slot[ok], key[ok])
        writes = int(ok.sum())
    none = keys == R.EMPTY
    ids8 = np.where(none, np.uint32(R.NONE), (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    depth8 = np.where(none, F(1), (keys >> np.uint64(32)).astype(np.uint32).view(F))
    edge8 = np.full(W * H * SAMPLES, -1, np.int8)
    rgba = np.empty((W * H, 4), F)
    with np.errstate(all="ignore"):
        c8 = K.CLEAR + K.CLEAR
        rgba[:] = ((c8 + c8) + (c8 + c8)) * F(0.125)                                         # FM5 of eight clear samples
    extrapolated = 0
    s_idx = np.nonzero(~none)[0]
    if len(s_idx):
        p, k = s_idx // SAMPLES, s_idx % SAMPLES
        j = ids8[s_idx].astype(np.int64)
        want = depth8[s_idx].view(np.uint32)
        row, col = p // W, p % W
        edge = np.full(len(p), -1, np.int64)
        s = np.zeros(len(p), F)
        extra = np.zeros(len(p), bool)
        for g in range(3):                                                                   # FM3: the first edge in draw order
            idx = 3 * j + g
            ok, pixel, d, t, centre = _sample(e, idx, np.where(e["xmajor"][idx], col, row), k, W)
            ok &= e["keep"][idx] & (pixel == p) & (d.view(np.uint32) == want) & (edge < 0)
            with np.errstate(all="ignore"):                                                  # FM4: at the pixel centre
                s0 = np.where(e["t_in"][idx] > 0, e["t_in"][idx], F(0))                      # step 7
                s1 = np.where(e["t_out"][idx] < 1, e["t_out"][idx], F(1))
                i0, i1 = F(1) / e["w0"][idx], F(1) / e["w1"][idx]
                a0, a1 = s0 * i0, s1 * i1
                num = a0 + t * (a1 - a0)
                den = i0 + t * (i1 - i0)
                sk = num / den
                sk = np.where(sk > 0, sk, F(0))                                              # (also a NaN)
                sk = np.where(sk > 1, F(1), sk)
            edge[ok], s[ok] = g, sk[ok]
            extra |= ok & ~centre
        assert (edge >= 0).all(), "a resolved sample without a winning edge"
        extrapolated = int(extra.sum())
        edge8[s_idx] = edge
        one_minus = F(1) - s                                                                 # step 8
        u = np.select([edge == 0, edge == 1], [np.zeros(len(p), F), s], one_minus)
        v = np.select([edge == 0, edge == 1], [s, np.ones(len(p), F)], one_minus)
        ix = np.minimum(tw - 1, np.floor(u * F(tw)).astype(np.int64))                        # step 9
        iy = np.minimum(th - 1, np.floor(v * F(th)).astype(np.int64))
        tex = skin[iy, ix]
        du, dv = u - F(0.5), v - F(0.5)                                                      # step 10
        f = F(1) - (du * du + dv * dv)
        colour = np.empty((len(p), 4), F)
        colour[:, :3] = tex[:, :3] * f[:, None]
        colour[:, 3] = 1
        touched = np.unique(p)                                                               # FM5
        a = np.empty((len(touched), SAMPLES, 4), F)
        a[:] = K.CLEAR
        a[np.searchsorted(touched, p), k] = colour
        with np.errstate(all="ignore"):
            rgba[touched] = (((a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])) + ((a[:, 4] + a[:, 5]) + (a[:, 6] + a[:, 7]))) * F(0.125)
    ids8, depth8, edge8 = ids8.reshape(H, W, SAMPLES), depth8.reshape(H, W, SAMPLES), edge8.reshape(H, W, SAMPLES)
    if stats is not None:
        covered = ids8 != R.NONE
        cnt = covered.sum(-1)
        low = np.where(covered, ids8, np.uint32(R.NONE)).min(-1)
        high = np.where(covered, ids8, np.uint32(0)).max(-1)
        ids1, depth1 = FR.frame(cam, inst, W, H)[:2]
        edge1 = centre_edges(e, ids1, depth1, W)
        stats.update(writes=writes, covered_hist=np.bincount(cnt.ravel(), minlength=9), two_bodies=int(((cnt > 0) & (low != high)).sum()),
                     empty_centre=int(((ids1 == R.NONE) & (cnt > 0)).sum()), centre_only=int(((ids1 != R.NONE) & (cnt == 0)).sum()),
                     cut=(e["cut"] & e["keep"][:, None]).sum(0).astype(np.int64), w_dropped=int(e["w_dropped"].sum()),
                     rejected_far=rejected_far, longest_x=longest_x, longest_y=longest_y,
                     extrapolated=extrapolated, edge=np.bincount(edge8[edge8 >= 0].astype(np.int64), minlength=3), edge8=edge8,
                     one=(cnt == SAMPLES) & (low == high) & (low == ids1) & (edge8.min(-1) == edge8.max(-1)) & (edge8[..., 0] == edge1))
    return ids8, depth8, rgba.reshape(H, W, 4), K.pack_bgra8(rgba).reshape(H, W)
