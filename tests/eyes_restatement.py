"""numpy float32 restatement of the eye rule: what the reference's depth attachment holds after the eye
pass (src/main.rs:585-647, 962-998), plus which instance wrote each pixel.

TEST INFRASTRUCTURE.  The kernel (nenbody_amd/csrc/nb_eyes.inc) and this module implement the same rule independently; the GPU
tests compare them bit for bit.  Every step is one binary32 operation on numpy float32 arrays (IEEE, round to nearest, no fusion),
in the order the rule writes it.  Inputs are cameras and model matrices as (count, 4, 4) / (n, 4, 4) float32 arrays whose [k] is
column k -- what oracle.cameras / oracle.instances, Scene.cameras and Scene.instances return -- so the rule can be fed from the
oracle or from hand-made matrices.
"""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
# the model triangle, drawn as the LineStrip 0-1-2-0 (src/main.rs:130-138, 249), in homogeneous coordinates
VERTS = np.array([[-1, -1, 0, 1], [1, 0, 0, 1], [-1, 1, 0, 1]], np.float32)
EDGES = ((0, 1), (1, 2), (2, 0))


def eye_constant(oracle, width=1024, horizontal_fov_deg=90.0, near=1.0, far=10000.0):
    """The reference's eye constant formed by the oracle: camera_constant(90 / W, W / 1, 1, 10000) (CameraArray::new divides the
    angle by the aspect ratio, src/gfx.rs:379-383); near / far other than the reference's for the clipping tests."""
    return oracle.camera_constant(float(F(horizontal_fov_deg) / F(width)), float(F(width) / F(1)), near, far)


def lattice_camera():
    """A caller camera for an exact lattice: x_clip = x / 512, y_clip = y, z' = 0.5, w = 1 ((4, 4), [k] = column k), so that
    xs = x + 512 exactly (W = 1024) and every depth is 0.5."""
    cp = np.zeros((4, 4), F)
    cp[0, 0] = F(1) / F(512)
    cp[1, 1] = 1
    cp[3, 2] = 0.5
    cp[3, 3] = 1
    return cp


# four bodies heading +x: half-integer x put edge ends on column centres (the left end covered, the right end not); body 3's upper
# vertex sits at y = 1.5 and its edge a1 -> a2 is cut by B4 at y = 1; the vertices at y = +-1 lie exactly on B3 / B4 = 0 (kept)
LATTICE_POS = np.array([[0.5, 0, 0], [0.5, 0, 0], [3.5, 0, 0], [7.5, 0.5, 0]], F)
LATTICE_VEL = np.tile(F([1, 0, 0]), (4, 1))


def lattice_expectation():
    """What every eye of the lattice sees through lattice_camera() with its own body included (NB_EYES_SEE_SELF), W = 1024:
    columns 511 and 512 read body 0 (it ties with body 1), 514 and 515 body 2, 518 and 519 body 3, each at depth 0.5."""
    ids = np.full(1024, NONE, np.uint32)
    ids[[511, 512]] = 0
    ids[[514, 515]] = 2
    ids[[518, 519]] = 3
    depth = np.where(ids == NONE, F(1), F(0.5)).astype(F)
    return ids, depth


def world_vertices(inst):
    """(n, 3, 4): w_r = ((M[r]*a.x + M[4+r]*a.y) + M[8+r]*a.z) + M[12+r]*a.w for the three model vertices."""
    m = np.ascontiguousarray(inst, np.float32).reshape(-1, 4, 4)      # m[:, k, r] = row r of column k
    out = np.empty((len(m), 3, 4), np.float32)
    with np.errstate(all="ignore"):                                   # (an infinite entry times zero is a NaN, silently)
        for v, a in enumerate(VERTS):
            out[:, v, :] = ((m[:, 0, :] * a[0] + m[:, 1, :] * a[1]) + m[:, 2, :] * a[2]) + m[:, 3, :] * a[3]
    return out


def clip_vertices(cams, world):
    """(E, n, 3, 4): c_r = ((C[r]*w0 + C[4+r]*w1) + C[8+r]*w2) + C[12+r]*w3 -- C * (M * a)."""
    c = np.ascontiguousarray(cams, np.float32).reshape(-1, 4, 4)
    cc = [c[:, k, None, None, :] for k in range(4)]                  # (E, 1, 1, 4): column k, rows r
    w = [world[None, :, :, k, None] for k in range(4)]               # (1, n, 3, 1)
    with np.errstate(all="ignore"):
        return ((cc[0] * w[0] + cc[1] * w[1]) + cc[2] * w[2]) + cc[3] * w[3]


def segments(cams, world, width, stats=None):
    """Clipped, projected edges: (keep, xs0, d0, xs1, d1), each (E, n, 3).  `stats`, a dict, collects over calls: "cut" (4 entries:
    kept edges that boundary B1 .. B4 cuts -- one end outside it, the other not) and "w_dropped" (edges that pass the clip and are
    dropped for an end with w <= 0)."""
    P = clip_vertices(cams, world)
    P0 = P[:, :, [a for a, _ in EDGES], :]
    P1 = P[:, :, [b for _, b in EDGES], :]
    shape = P0.shape[:3]
    t_in = np.zeros(shape, np.float32)
    t_out = np.ones(shape, np.float32)
    keep = np.ones(shape, bool)
    with np.errstate(all="ignore"):
        def bounds(p):
            y, z, w = p[..., 1], p[..., 2], p[..., 3]
            return (z, w - z, w + y, w - y)          # near, far, y = -w, y = +w

        crossed = []
        for b0, b1 in zip(bounds(P0), bounds(P1)):
            keep &= ~((b0 < 0) & (b1 < 0))
            r = b0 / (b0 - b1)
            enter = (b0 < 0) & (b1 >= 0)
            leave = (b1 < 0) & (b0 >= 0)
            crossed.append(enter | leave)
            t_in = np.where(enter & (r > t_in), r, t_in)       # max(t_in, r); a NaN r changes nothing
            t_out = np.where(leave & (r < t_out), r, t_out)    # min(t_out, r)
        keep &= ~(t_in > t_out)
        D = P1 - P0
        Q0 = np.where((t_in > 0)[..., None], P0 + t_in[..., None] * D, P0)
        Q1 = np.where((t_out < 1)[..., None], P0 + t_out[..., None] * D, P1)
        positive = (Q0[..., 3] > 0) & (Q1[..., 3] > 0)
        if stats is not None:
            stats["w_dropped"] = stats.get("w_dropped", 0) + int((keep & ~positive).sum())
            stats["cut"] = stats.get("cut", np.zeros(4, np.int64)) + np.array([int((keep & positive & c).sum()) for c in crossed])
        keep &= positive
        h = F(width) * F(0.5)
        xs0 = (Q0[..., 0] / Q0[..., 3]) * h + h
        xs1 = (Q1[..., 0] / Q1[..., 3]) * h + h
        d0 = Q0[..., 2] / Q0[..., 3]
        d1 = Q1[..., 2] / Q1[..., 3]
    return keep, xs0, d0, xs1, d1


def eyes(cams, inst, first, width, see_self=False, chunk=8, stats=None):
    """The rule for eyes first .. first + len(cams) - 1 (eye e is body first + e) over every body of `inst`.
    Returns (ids uint32 (E, width), depth float32 (E, width)).  `stats`, a dict, collects over calls what `segments` counts and
    "rejected_far" (covered columns of a segment whose depth is >= 1: no candidate) and "widest" (the most candidate columns of one
    segment)."""
    cams = np.ascontiguousarray(cams, np.float32).reshape(-1, 4, 4)
    world = world_vertices(inst)
    E = len(cams)
    ids = np.empty((E, width), np.uint32)
    depth = np.empty((E, width), np.float32)
    for e0 in range(0, E, chunk):
        e1 = min(E, e0 + chunk)
        keys = _resolve(cams[e0:e1], world, first + e0, width, see_self, stats)
        none = keys == EMPTY
        ids[e0:e1] = np.where(none, np.uint32(NONE), (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        depth[e0:e1] = np.where(none, F(1), (keys >> np.uint64(32)).astype(np.uint32).view(np.float32))
    return ids, depth


def _resolve(cams, world, first, width, see_self, stats=None):
    E, n = len(cams), len(world)
    keep, xs0, d0, xs1, d1 = segments(cams, world, width, stats)
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
        # the columns that can be covered, a superset: the exact test below decides
        lo = np.clip(np.floor(np.maximum(xa.astype(np.float64), -4.0)) - 1, 0, width).astype(np.int64)
        hi = np.clip(np.ceil(np.minimum(xb.astype(np.float64), width + 4.0)) + 1, 0, width).astype(np.int64)
    keys = np.full(E * width, EMPTY, np.uint64)
    span = np.maximum(hi - lo, 0)
    total = int(span.sum())
    if total == 0:
        return keys.reshape(E, width)
    seg = np.repeat(np.arange(len(lo)), span)
    col = np.arange(total) - np.repeat(np.cumsum(span) - span, span) + lo[seg]
    xc = col.astype(np.float32) + F(0.5)                   # exact
    s0, s1 = xs0[keep][seg], xs1[keep][seg]
    e0, e1 = d0[keep][seg], d1[keep][seg]
    with np.errstate(all="ignore"):
        covered = (xa[seg] <= xc) & (xc < xb[seg])
        t = (xc - s0) / (s1 - s0)
        d = e0 + t * (e1 - e0)
        cand = covered & (d < F(1))
        far = covered & (d >= F(1))
        d = np.where(d > 0, d, F(0))                       # !(d > 0) -> +0
    if stats is not None:
        stats["rejected_far"] = stats.get("rejected_far", 0) + int(far.sum())
        stats["widest"] = max(stats.get("widest", 0), int(np.bincount(seg[cand], minlength=1).max()))
    key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j_idx[seg].astype(np.uint64)
    slot = e_idx[seg] * width + col
    np.minimum.at(keys, slot[cand], key[cand])
    return keys.reshape(E, width)
