"""numpy restatement of DESIGN.md section 12: the seen set of an eye row (S1-S5) and the boids step restricted to what each body
sees (V1-V3).

TEST INFRASTRUCTURE.  The kernels (nenbody_amd/csrc/nb_seen.inc) and this module implement the same rule independently; the GPU
tests compare every word.  The seen set goes through np.unique; the step is np_restatement.boids_step written out again with the
one change the rule makes, `ne = (idx != i) & mask[:, i]` -- every operation one binary32 operation on numpy float32 arrays.
boids_seen_step_lists is the same step over lists as a caller may hand them to nb_launch_boids_seen_step -- in slot order, duplicates
folded again, the count clamped at the stride --; tests/test_seen_lists_cpu.py ties it to the mask form and to the C oracle.
"""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF


def seen(ids_row, depth_row=None):
    """S1-S5 for one row of W columns: (count, ids (W,) uint32, depth (W,) float32, cols (W,) uint32).  ``depth_row`` None: every
    depth bit pattern counts as 0 (what the kernel does without depth rows; its seen_depth is then not written)."""
    ids_row = np.ascontiguousarray(ids_row, np.uint32)
    w = len(ids_row)
    bits = np.zeros(w, np.uint32) if depth_row is None else np.ascontiguousarray(depth_row, np.float32).view(np.uint32)
    drawn = ids_row != np.uint32(NONE)
    members, cols = np.unique(ids_row[drawn], return_counts=True)                    # S1, S3: ascending as unsigned numbers; S4
    k = len(members)
    out_ids = np.full(w, NONE, np.uint32)
    out_bits = np.full(w, F(1).view(np.uint32), np.uint32)
    out_cols = np.zeros(w, np.uint32)
    out_ids[:k] = members
    out_cols[:k] = cols
    for slot, m in enumerate(members):
        out_bits[slot] = bits[ids_row == m].min()                                    # S5: the unsigned minimum of the bit patterns
    return k, out_ids, out_bits.view(np.float32), out_cols


def seen_rows(ids, depth=None):
    """:func:`seen` for every row of (E, W) arrays: (count (E,), ids, depth, cols (E, W))."""
    ids = np.ascontiguousarray(ids, np.uint32)
    e, w = ids.shape
    count = np.zeros(e, np.uint32)
    out_ids = np.empty((e, w), np.uint32)
    out_depth = np.empty((e, w), np.float32)
    out_cols = np.empty((e, w), np.uint32)
    for r in range(e):
        count[r], out_ids[r], out_depth[r], out_cols[r] = seen(ids[r], None if depth is None else depth[r])
    return count, out_ids, out_depth, out_cols


def mask_of_rows(ids, n, first=0):
    """mask[e, i]: eye e's row (body first + e) holds body i < n -- S(first + e) as a row of booleans, (E, n)."""
    ids = np.ascontiguousarray(ids, np.uint32)
    mask = np.zeros((len(ids), n), bool)
    e, c = np.nonzero(ids < np.uint32(n))
    mask[e, ids[e, c]] = True
    return mask


def mask_of_lists(count, lists, n):
    """the same from seen lists (count (E,), lists (E, stride)); entries >= n are outside the set and dropped (V2)"""
    lists = np.ascontiguousarray(lists, np.uint32)
    mask = np.zeros((len(lists), n), bool)
    for e in range(len(lists)):
        row = lists[e, :min(int(count[e]), lists.shape[1])]
        mask[e, row[row < n]] = True
    return mask


def lists_of_mask(mask, stride=None):
    """the ascending, duplicate-free lists of a mask (E, n): (count (E,) uint32, lists (E, stride) uint32, NONE behind count[e])"""
    mask = np.asarray(mask, bool)
    stride = mask.shape[1] if stride is None else stride
    count = mask.sum(1).astype(np.uint32)
    assert count.max(initial=0) <= stride
    lists = np.full((len(mask), stride), NONE, np.uint32)
    for e in range(len(mask)):
        lists[e, :count[e]] = np.nonzero(mask[e])[0]
    return count, lists


def boids_seen_step_lists(pos, vel, count, lists, first=0, dt=F(0.04), r1=F(1000.0), r2=F(5.0), r3=F(500.0), s1=F(0.02), s2=F(0.05),
                          s3=F(0.5)):
    """V2-V3 for lists, as include/nenbody.h states nb_launch_boids_seen_step: row e of ``lists`` (E, stride) belongs to body
    first + e of the n bodies of (pos, vel), which folds the reference's three rules over the slots k < min(count[e], stride) in slot
    order.  An entry equal to first + e, or >= n, is skipped; a duplicate folds again; what lies behind the count is never looked at.
    Vectorised over the bodies e, sequential over the slot index k; every operation one binary32 numpy operation, the radius tests
    the reference's own sqrt(d2) < r.  Returns (positions, velocities), each (E, 3), of bodies first .. first + E - 1."""
    old_p = np.ascontiguousarray(pos, np.float32)
    old_v = np.ascontiguousarray(vel, np.float32)
    lists = np.ascontiguousarray(lists, np.uint32)
    n = len(old_p)
    e, stride = lists.shape
    me = first + np.arange(e, dtype=np.int64)
    pn, vn = old_p[me], old_v[me]
    length = np.minimum(np.asarray(count, np.uint32).astype(np.int64), stride)
    c = np.zeros((e, 3), np.float32)
    r = np.zeros((e, 3), np.float32)
    m = np.zeros((e, 3), np.float32)
    cnt = np.zeros(e, np.int32)
    vcnt = np.zeros(e, np.int32)
    with np.errstate(all="ignore"):
        for k in range(stride):
            i = lists[:, k].astype(np.int64)
            live = (k < length) & (i != me) & (i < n)     # V2: inside the count, not the body itself, inside the set
            j = np.where(live, i, 0)                      # (a skipped entry is not read: any record stands in, no rule takes it)
            pi, vi = old_p[j], old_v[j]
            d = pi - pn                                   # distance2: (other - self)
            sq = d * d
            d2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
            p1 = (d2 < F(r1)) & live                      # main.rs:474-475
            c = np.where(p1[:, None], c + pi, c)
            cnt = cnt + p1
            p2 = (np.sqrt(d2) < F(r2)) & live             # main.rs:485-486
            r = np.where(p2[:, None], r - (pi - pn), r)
            dv = vi - vn
            sv = dv * dv
            d2v = (sv[:, 0] + sv[:, 1]) + sv[:, 2]
            p3 = (np.sqrt(d2v) < F(r3)) & live            # main.rs:497-498
            m = np.where(p3[:, None], m + vi, m)
            vcnt = vcnt + p3
        has = cnt > 0
        c = np.where(has[:, None], c / np.maximum(cnt, 1).astype(np.float32)[:, None], c)        # main.rs:506-508
        hasv = vcnt > 0
        m = np.where(hasv[:, None], m / np.maximum(vcnt, 1).astype(np.float32)[:, None], m)     # main.rs:510-512
        v = (c * F(s1) + r * F(s2)) + m * F(s3)           # main.rs:514
        sq = v * v
        mag = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
        big = mag > F(1.0)                                # main.rs:516-518
        scale = np.where(big, F(1.0) / np.where(big, mag, F(1.0)), F(1.0)).astype(np.float32)
        v = np.where(big[:, None], v * scale[:, None], v).astype(np.float32)
        p = (v * F(dt) + pn).astype(np.float32)           # main.rs:521
    return p, v


def boids_seen_step(pos, vel, mask, dt=F(0.04), r1=F(1000.0), r2=F(5.0), r3=F(500.0), s1=F(0.02), s2=F(0.05), s3=F(0.5)):
    """update_instance_boids (src/main.rs:443-526) with `i in S(n)` added to each of the three tests: mask[n, i] says that body n
    sees body i.  Vectorised over the bodies n, sequential over the fold index i."""
    old_p = pos.astype(np.float32).copy()        # main.rs:459
    old_v = vel.astype(np.float32).copy()        # main.rs:460
    n = len(old_p)
    idx = np.arange(n)
    c = np.zeros((n, 3), np.float32)
    r = np.zeros((n, 3), np.float32)
    m = np.zeros((n, 3), np.float32)
    cnt = np.zeros(n, np.int32)
    vcnt = np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            d = old_p[i][None, :] - old_p            # distance2: (other - self)
            sq = d * d
            d2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
            ne = (idx != i) & mask[:, i]             # V2: n != i, and n sees i
            p1 = (d2 < F(r1)) & ne                   # main.rs:474-475
            c = np.where(p1[:, None], c + old_p[i][None, :], c)
            cnt = cnt + p1
            p2 = (np.sqrt(d2) < F(r2)) & ne          # main.rs:485-486
            r = np.where(p2[:, None], r - (old_p[i][None, :] - old_p), r)
            dv = old_v[i][None, :] - old_v
            sv = dv * dv
            d2v = (sv[:, 0] + sv[:, 1]) + sv[:, 2]
            p3 = (np.sqrt(d2v) < F(r3)) & ne         # main.rs:497-498
            m = np.where(p3[:, None], m + old_v[i][None, :], m)
            vcnt = vcnt + p3
        has = cnt > 0
        c = np.where(has[:, None], c / np.maximum(cnt, 1).astype(np.float32)[:, None], c)        # main.rs:506-508
        hasv = vcnt > 0
        m = np.where(hasv[:, None], m / np.maximum(vcnt, 1).astype(np.float32)[:, None], m)     # main.rs:510-512
        v = (c * F(s1) + r * F(s2)) + m * F(s3)      # main.rs:514
        sq = v * v
        mag = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
        big = mag > F(1.0)                           # main.rs:516-518
        scale = np.where(big, F(1.0) / np.where(big, mag, F(1.0)), F(1.0)).astype(np.float32)
        v = np.where(big[:, None], v * scale[:, None], v).astype(np.float32)
        p = (v * F(dt) + old_p).astype(np.float32)   # main.rs:521
    return p, v
