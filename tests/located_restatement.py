"""numpy restatement of DESIGN.md section 13: the located seen set of an eye (L1-L6) and the gravity step over those relative
positions alone (G2-G3).

TEST INFRASTRUCTURE.  The kernels (nenbody_amd/csrc/nb_located.inc) and this module implement the same rule independently; the GPU
tests compare every word.  Every arithmetic step is one binary32 operation on numpy float32 values, in the order the rule writes it.
It sits on seen_restatement.seen_rows (the lists) and eyes_restatement (the rows).
"""
import numpy as np

import seen_restatement as S

F = np.float32
NONE = S.NONE
ZERO = (1, 2, 3, 4, 6, 7, 8, 9, 12, 13, 15)


def invertible(cp):
    """L6: the constant has the shape nb_camera_constant produces, so that L2 inverts cp * view.  None where it has, else the index
    of the first entry that does not fit, in the order the library names them (11, then the zero entries ascending, then 0, then 14)."""
    cp = np.ascontiguousarray(cp, np.float32).reshape(16)
    if not cp[11] == F(-1):
        return 11
    for i in ZERO:
        if not cp[i] == F(0):
            return i
    if not cp[0] != F(0):
        return 0
    if not cp[14] != F(0):
        return 14
    return None


def normalize(x):
    """x * (1 / sqrt((x0*x0 + x1*x1) + x2*x2)) on (..., 3) float32"""
    q = x * x
    mag = np.sqrt((q[..., 0] + q[..., 1]) + q[..., 2])
    s = F(1) / mag
    return x * s[..., None]


def axes(dirs, up):
    """L3 for (E, 3) direction records: f = normalize(Dir), s = normalize(f x up), the cross product as cameras_kernel writes it"""
    up = np.ascontiguousarray(up, np.float32).reshape(3)
    with np.errstate(all="ignore"):
        f = normalize(np.ascontiguousarray(dirs, np.float32))
        s = np.stack([f[:, 1] * up[2] - f[:, 2] * up[1], f[:, 2] * up[0] - f[:, 0] * up[2], f[:, 0] * up[1] - f[:, 1] * up[0]], 1)
        return f, normalize(s)


def located(ids_row, depth_row, count, seen_ids, seen_depth, direction, up, cp):
    """L1-L5 for one eye: (col (W,) uint32, rel (W, 4) float32).  ``count`` above W is taken as W."""
    assert invertible(cp) is None
    cp = np.ascontiguousarray(cp, np.float32).reshape(16)
    ids_row = np.ascontiguousarray(ids_row, np.uint32)
    bits_row = np.ascontiguousarray(depth_row, np.float32).view(np.uint32)
    seen_ids = np.ascontiguousarray(seen_ids, np.uint32)
    seen_bits = np.ascontiguousarray(seen_depth, np.float32).view(np.uint32)
    w = len(ids_row)
    col = np.full(w, NONE, np.uint32)                                                    # L5
    rel = np.zeros((w, 4), np.float32)
    f, s = axes(np.ascontiguousarray(direction, np.float32).reshape(1, 3), up)          # L3
    f, s = f[0], s[0]
    h = F(w) * F(0.5)
    with np.errstate(all="ignore"):
        for k in range(min(int(count), w)):
            m, dbits = seen_ids[k], seen_bits[k]
            if m == np.uint32(NONE):                                                     # NB_EYES_NONE is no member
                continue
            hit = np.nonzero((ids_row == m) & (bits_row == dbits))[0]                    # L1
            if len(hit) == 0:
                continue
            c = int(hit[0])
            col[k] = c
            xc = F(c) + F(0.5)                                                           # L2
            xn = (xc - h) / h
            d = np.uint32(dbits).view(np.float32)
            r = cp[14] / (d + cp[10])
            xv = (xn * r) / cp[0]
            rel[k, :3] = r * f + xv * s                                                  # L4: two products and one sum a component
            rel[k, 3] = r
    return col, rel


def located_rows(ids, depth, count, seen_ids, seen_depth, dirs, up, cp):
    """:func:`located` for every row of (E, W) arrays: (col (E, W), rel (E, W, 4))"""
    ids = np.ascontiguousarray(ids, np.uint32)
    e, w = ids.shape
    col = np.empty((e, w), np.uint32)
    rel = np.empty((e, w, 4), np.float32)
    for r in range(e):
        col[r], rel[r] = located(ids[r], depth[r], count[r], seen_ids[r], seen_depth[r], dirs[r], up, cp)
    return col, rel


def located_of_rows(ids, depth, dirs, up, cp):
    """the lists of the rows by seen_restatement.seen_rows, then their located sets: (count, sids, sdepth, scols, col, rel)"""
    count, sids, sdepth, scols = S.seen_rows(ids, depth)
    col, rel = located_rows(ids, depth, count, sids, sdepth, dirs, up, cp)
    return count, sids, sdepth, scols, col, rel


def nbody_located_step(pos, vel, count, rel, first=0, dt=F(0.1), g=F(0.001), bias=F(0.0000001)):
    """G2-G3: row e of ``rel`` (E, stride, >= 3) belongs to body first + e of (pos, vel), which folds update_instance_nbody's law
    (src/main.rs:425-436) over the slots k < min(count[e], stride) in slot order with vec = rel[e, k, :3].  Vectorised over the bodies,
    sequential over the slot index.  Returns (positions, velocities), each (E, 3), of bodies first .. first + E - 1."""
    rel = np.ascontiguousarray(rel, np.float32)
    e, stride = rel.shape[:2]
    me = first + np.arange(e)
    p = np.ascontiguousarray(pos, np.float32)[me]
    v = np.ascontiguousarray(vel, np.float32)[me]
    length = np.minimum(np.asarray(count, np.uint32).astype(np.int64), stride)
    dt, g, bias = F(dt), F(g), F(bias)
    total = np.zeros((e, 3), np.float32)
    with np.errstate(all="ignore"):
        for k in range(int(length.max(initial=0))):
            vec = rel[:, k, :3]
            sq = vec * vec
            dist = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + bias                             # main.rs:429
            term = (vec * g) / dist[:, None]                                             # main.rs:430
            total = np.where((k < length)[:, None], total + term, total)
        v = v + total * dt                                                               # main.rs:434
        p = v + p                                                                        # main.rs:436
    return p.astype(np.float32), v.astype(np.float32)
