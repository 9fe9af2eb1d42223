"""A binary64 geometric reference of what an eye row and the scene camera's frame show, with a derived bound beside every value.

TEST INFRASTRUCTURE.  The kernels and the numpy restatements (tests/*_restatement.py) were written from one text, the steps of
DESIGN.md sections 10 and 11; this module is written from the reference application's semantics instead and shares nothing with
them.  It takes positions, velocities, `up`, the perspective parameters and the extent, and asks geometry:

  outline   body j's outline is p_j + Rz(atan2(v.y, v.x)) a for a = (-1,-1,0), (1,0,0), (-1,1,0); its edges a0->a1, a1->a2, a2->a0 in
            that draw order carry the texture coordinates (0,0), (0,1), (1,1) at those vertices.
  camera    f = normalize(dir), s = normalize(f x up), u = s x f (look_at_dir); a point q lies at view distance w = f.(q - eye) and
            its depth is far / (far - near) * (1 - near / w).
  a column  the points that project to screen x form the plane through the eye {kx s.(q - eye) = ndc_x f.(q - eye)}, kx =
            cot(fovy / 2) / aspect.  Intersecting an edge's segment P0 + s (P1 - P0) with it gives the edge parameter s* directly:
            with g_i = kx s.(P_i - eye) - ndc_x f.(P_i - eye), s* = g0 / (g0 - g1).  A hit needs 0 <= s* <= 1, near <= w < far and
            |cot(fovy / 2) u.(q - eye)| <= w at that point.  The column shows the hit of least depth (ties: the lower body, then
            the earlier edge) over every body but the eye's own unless `see_self`.
  colour    (u, v) from s* and the edge's end coordinates, the nearest texel, the vignette 1 - |uv - 1/2|^2; the clear colour
            where nothing hits.  An 8-sample row takes winner and depth at x_k = c + o_k, the colour of a sample's (body, edge) at
            the column centre with s* clamped to [0, 1], and the mean of the eight.
  frame     the same with a second axis: the edge is cut in binary64 to near, far and |y| <= w ONLY to learn the major axis of its
            projected ends and to list the centres along it; then the UNCUT edge is intersected with the column's plane (x-major)
            or the row's plane (y-major), and the floor of the minor coordinate names the pixel.
No clip algorithm and no screen-space interpolation produces a value here.

BOUNDS.  Beside every value stands a bound on how far the binary32 rule may lie from it: first order, built from magnitude sums,
not tuned.  For each clip component (x = kx s.(q - eye), y = ky u.(q - eye), w = f.(q - eye), z = A w - A near) the sum S of the
absolute values of the products that enter it is carried -- |basis_i| (|p_i| + |rotation terms_i| + |eye_i|), the basis vectors'
own entries taken as the magnitude sums of the cross products that form them -- and the component's bound is S * 2^-24 * R, R the
number of binary32 roundings on the longest path from (pos, vel) to it.  The count (ROUNDINGS):
  camera kernel   f = normalize(dir): 2 products' sum (3), sqrt, reciprocal, scale = 6; s = normalize(f x up): cross 2, normalize 6
                  = 14; u = s x f: 2 = 16; a translation entry -eye.u: product and two sums = 19; the constant's entry (degrees to
                  radians, tan within an ulp = 2, reciprocal, / aspect, the correction's product) = 6; constant x view: a product
                  and three sums = 4; together 29.
  instance kernel atan2 within an ulp of an angle of at most pi (2 pi < 7 units of 2^-24 in the sine and cosine), sine / cosine
                  within an ulp (2) = 9; the vertex: two sums = 11.
  step 1          camera x vertex: a product and three sums = 4.
  the rule after  clip parameter 3, clipped end 3, projection 3, the column's parameter 3, the interpolation 3, one spare = 16: these
                  act on values the same magnitude sums bound, so they join the count.
R = 29 + 11 + 4 + 16 = 60.  Propagation: a plane's g_i carries dg = R 2^-24 (S_major + max(1, |ndc|) S_w), so ds* = (|g0| + |g1|)
dg / (g0 - g1)^2; a value v(s) between the ends carries its component bound plus |dv/ds| ds*; depth = z / w carries (dz + depth
dw) / w + A near |w1 - w0| / w^2 ds* + 8 * 2^-24; the vignette 2 (|u - 1/2| + |v - 1/2|) ds* + 6 * 2^-24; a colour |texel| times
that + 4 * 2^-24 |colour|; the mean of eight samples the mean of their bounds + 4 * 2^-24.

UNDECIDED CELLS.  A cell is undecided when a decision could flip within these bounds: a hit condition (0 <= s* <= 1: a span end
against a centre or sample, decided by the signs of g0 and g1 against dg; near, far = `d < 1`, and the y planes: a clip plane's
sign) whose margin is below its bound; a second hit of another body whose depth interval reaches the winner's; the frame's
major-axis comparison; the floor of the minor coordinate.  Its COLOUR is undecided (`und_colour`, per column `und_rgba`) besides
where a hit of another edge of the winner is in reach (body and depth stand, the depth's bound then spans both edges), a texel
index could flip, a centre shaded by extrapolation has a plane nearly parallel to the edge (ds* > 1/4, unless the parameter
surely lies beyond an end: it is then clamped to that end exactly) or a w not surely positive, or the colour's bound exceeds
MAX_COLOUR_BOUND = 1/32.  In eye rows the order of two certain hits on two edges of one body is settled more sharply than by
intervals (`_resolve`): both are cut from the same three binary32 clip vertices by one plane through the eye, no error of the
vertices swaps them unless it reverses the triangle's orientation in (x, w) or moves the shared vertex across the plane, and both
are excluded by their bounds; what remains is the rounding of the rule's own steps from those vertices on (`loc`).  Two bodies
with identical position and velocity give identical keys in any arithmetic: between them the lower index wins and nothing is
undecided.  The same holds between two hits on edges whose w is the camera's translation entry alone (every other product that
enters it an exact zero: a camera looking straight down on planar data): their depth words are equal, the lower index wins, then
the earlier edge.  Undecided cells are masks and are left out of comparisons; decided cells are compared in full by `compare`,
`compare_seen`.

Largest observed error / bound, restatements and device alike, over tests/vision_reference_cases.py (test_vision_reference_cpu.py
prints them): depth 0.026 (eyes, eyes_colour), 0.021 (eyes_msaa), 0.014 (frame); rgba 0.078, 0.19 (on a centre clamped to an edge's
end, bound 6 * 2^-24), 0.062; where a second edge of the winner may be the nearer one, below 1 by construction (0.9999).  Caps per
case: undecided cells at most 5 % of the cells a body touches (observed at most 2.3 %, through 8 samples 4.0 %); cells whose colour
is not compared at most 5 % as well (observed 2.9 %, 3.1 %; the positions * 30 case cannot meet this one and says so in the case
list: 55 %, 53 %); at least 200 decided covered cells and 200 columns compared in colour (W <= 3, 1 x 1, 3 x 2: one).
"""
import types

import numpy as np

U = 2.0 ** -24
ROUNDINGS = dict(camera=29, instance=11, step1=4, rule=16)
R = float(sum(ROUNDINGS.values()))
NONE = 0xFFFFFFFF
CLEAR = np.array([np.float32(0.1), np.float32(0.2), np.float32(0.3), 1.0], np.float64)
OFFSETS = np.array([9, 7, 13, 5, 3, 1, 11, 15], np.float64) / 16.0      # Vulkan's standard 8-sample pattern, x coordinates
MODEL = np.array([[-1.0, -1.0, 0.0], [1.0, 0.0, 0.0], [-1.0, 1.0, 0.0]])
WHITE = np.ones((1, 1, 4))
MAX_COLOUR_BOUND = 1.0 / 32      # a colour whose bound is wider (the vignette spans 1/2) is not compared: the cell counts as undecided


def srgb8_to_linear(img):
    """an (th, tw, 4) uint8 sRGB image as binary64 linear texels: the sRGB decode for the colours, alpha / 255"""
    e = np.asarray(img, np.float64) / 255.0
    out = np.where(e <= 0.04045, e / 12.92, ((e + 0.055) / 1.055) ** 2.4)
    out[..., 3] = e[..., 3]
    return out


def lens(fovy_deg, aspect, near=1.0, far=10000.0):
    cot = 1.0 / np.tan(np.radians(float(fovy_deg)) / 2.0)
    return types.SimpleNamespace(kx=cot / float(aspect), ky=cot, near=float(near), far=float(far), A=float(far) / (float(far) - float(near)))


def outline(pos, vel, model=MODEL):
    """world vertices (n, 3 vertices, 3) and the magnitude sums of the products that form them"""
    pos, vel = np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    th = np.arctan2(vel[:, 1], vel[:, 0])
    c, s = np.cos(th)[:, None], np.sin(th)[:, None]
    ax, ay, az = model[None, :, 0], model[None, :, 1], model[None, :, 2]
    verts = pos[:, None, :] + np.stack([c * ax - s * ay, s * ax + c * ay, az + 0 * c], -1)
    mag = np.abs(pos)[:, None, :] + np.stack([np.abs(c * ax) + np.abs(s * ay), np.abs(s * ax) + np.abs(c * ay), np.abs(az) + 0 * c], -1)
    return verts, mag


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _cross_mag(a, b):
    return np.array([a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]])


def basis(direction, up):
    d, up = np.asarray(direction, np.float64), np.asarray(up, np.float64)
    with np.errstate(all="ignore"):
        f = d / np.sqrt(d @ d)
        cr = _cross(f, up)
        n = np.sqrt(cr @ cr)
        s = cr / n
        u = _cross(s, f)
        fm = np.abs(f)
        sm = _cross_mag(fm, np.abs(up)) / n
        um = _cross_mag(sm, fm)
    return types.SimpleNamespace(f=f, s=s, u=u, fm=fm, sm=sm, um=um)


def _clip(verts, mag, eye, b, L):
    """clip components of every vertex for one camera, (n, 3) each, and their magnitude sums"""
    eye = np.asarray(eye, np.float64)
    rel = verts - eye
    reach = mag + np.abs(eye)
    return dict(X=L.kx * (rel @ b.s), Y=L.ky * (rel @ b.u), W=rel @ b.f, SX=L.kx * (reach @ b.sm), SY=L.ky * (reach @ b.um),
                SW=reach @ b.fm, SWr=mag @ b.fm)


def _visible(c, L):
    """the part [lo, hi] of each edge (n, 3) that lies within near, far and the y planes; `cut` (n, 3, 4): the plane has one end
    outside it.  Used to list candidate centres and, for the frame, to learn the major axis: never for a value."""
    i1 = [1, 2, 0]
    W0, W1, Y0, Y1 = c["W"], c["W"][:, i1], c["Y"], c["Y"][:, i1]
    lo, hi = np.zeros(W0.shape), np.ones(W0.shape)
    dead = np.zeros(W0.shape, bool)
    cut = np.zeros(W0.shape + (4,), bool)
    with np.errstate(all="ignore"):
        for p, (c0, c1) in enumerate(((W0 - L.near, W1 - L.near), (L.far - W0, L.far - W1), (W0 + Y0, W1 + Y1), (W0 - Y0, W1 - Y1))):
            r = c0 / (c0 - c1)
            enter, leave = (c0 < 0) & (c1 >= 0), (c1 < 0) & (c0 >= 0)
            lo = np.where(enter, np.maximum(lo, r), lo)
            hi = np.where(leave, np.minimum(hi, r), hi)
            dead |= ((c0 < 0) & (c1 < 0)) | ~np.isfinite(c0) | ~np.isfinite(c1)
            cut[..., p] = enter | leave
    return lo, hi, ~dead & (lo <= hi), cut


def _hits(c, L, j, k, nm, axis):
    """Edge k of body j against the plane whose normalised device coordinate along `axis` ("X" or "Y") is nm: the edge parameter,
    the point's clip components, depth, and their bounds; `certain`: every hit condition holds by more than its bound; `possible`:
    none fails by more than its bound."""
    k1 = (k + 1) % 3
    W0, W1 = c["W"][j, k], c["W"][j, k1]
    SW = np.maximum(c["SW"][j, k], c["SW"][j, k1])
    M0, M1 = c[axis][j, k], c[axis][j, k1]
    SM = np.maximum(c["S" + axis][j, k], c["S" + axis][j, k1])
    h = types.SimpleNamespace()
    with np.errstate(all="ignore"):
        g0, g1 = M0 - nm * W0, M1 - nm * W1
        den = g0 - g1
        dg = R * U * (SM + np.maximum(1.0, np.abs(nm)) * SW)
        s = g0 / den
        ds = (np.abs(g0) + np.abs(g1)) * dg / (den * den)
        bW = R * U * SW
        bZ = R * U * L.A * (SW + L.near)
        dW = W1 - W0
        w = W0 + s * dW
        dw = bW + np.abs(dW) * ds
        z = L.A * (w - L.near)
        dz = bZ + L.A * np.abs(dW) * ds
        depth = L.A * (1.0 - L.near / w)
        dd = (bZ + np.abs(depth) * bW) / w + L.A * L.near * np.abs(dW) / (w * w) * ds + 8 * U
        for name in ("X", "Y"):
            V0, V1 = c[name][j, k], c[name][j, k1]
            bV = R * U * np.maximum(c["S" + name][j, k], c["S" + name][j, k1])
            setattr(h, name, V0 + s * (V1 - V0))
            setattr(h, "d" + name, bV + np.abs(V1 - V0) * ds)
            setattr(h, "b" + name, bV)
            setattr(h, "D" + name, V1 - V0)
        ymargin = w - np.abs(h.Y)
        dym = dw + h.dY
        finite = np.isfinite(s) & np.isfinite(ds) & np.isfinite(depth) & np.isfinite(dd)
        # 0 <= s* <= 1 is the plane separating the ends: decided by the signs of g0 and g1 against their bound
        apart = ((g0 >= dg) & (g1 <= -dg)) | ((g0 <= -dg) & (g1 >= dg))
        one_side = ((g0 > dg) & (g1 > dg)) | ((g0 < -dg) & (g1 < -dg))
        certain = finite & apart & (w - dw > 0) & (z - dz >= 0) & (depth + dd < 1) & (ymargin - dym >= 0)
        possible = finite & ~one_side & (w + dw > 0) & (z + dz >= 0) & (depth - dd < 1) & (ymargin + dym >= 0)
        possible |= ~finite & ~one_side
        depth = np.where(finite, depth, 0.0)
        dd = np.where(finite, dd, 0.0)
        # the least depth a possible hit may have: over the part of the edge its parameter may lie on
        sa, sb = np.where(finite, np.clip(s - ds, 0.0, 1.0), 0.0), np.where(finite, np.clip(s + ds, 0.0, 1.0), 1.0)
        wmin = np.minimum(W0 + sa * dW, W0 + sb * dW) - bW
        lo = np.where(wmin > 0.5 * L.near, L.A * (1.0 - L.near / wmin) - (bZ + bW) / wmin - 8 * U, 0.0)
        h.lo = np.where(certain, depth - dd, np.clip(lo, 0.0, None))
    # every product that enters w but the camera's translation entry is an exact zero, in any arithmetic: both ends of the edge have
    # that entry's w and z, word for word, and so has every point the rule interpolates between them
    h.flat = (c["SWr"][j, k] == 0) & (c["SWr"][j, k1] == 0)
    h.s, h.ds, h.w, h.dw, h.bW, h.dW, h.depth, h.dd, h.certain, h.possible, h.finite = s, ds, w, dw, bW, dW, depth, dd, certain, possible, finite
    return h


def _resolve(cell, ncell, depth, dd, lo, body, edge, certain, possible, canon, flat, loc=None, firm=None):
    """Per cell the winning pair among the certain hits (least depth, then the lower body, then the earlier edge; -1: none); `und`:
    another possible hit's depth interval reaches the winner's (or, without a winner, exists at all) and it is another body's, or
    no hit of the winner's body; `und_edge`: a hit of ANOTHER EDGE OF THE WINNER does (the body stands, the colour does not, and the
    depth's bound, returned as `bound`, reaches down to that hit's least depth `lo`); `touched`: anything may hit the cell; `hidden`: a farther
    certain hit of another body lies behind a decided winner.
    `loc`, `firm` (eye rows): two certain hits on two edges of ONE body are cut from the same three binary32 clip vertices by one plane
    through the eye.  With V the shared vertex and a, b the edges from it, the hits lie at lambda_A, lambda_B along the plane's ray in
    (x, w), and lambda_A - lambda_B = cross(V, r) cross(a, b) / (cross(r, a) cross(r, b)): its sign is that of the triangle's
    orientation times the side V lies on, so no error of the vertices swaps the two unless it reverses the orientation (`firm`: it
    cannot) or moves V across the plane (a certain hit: it cannot).  What can still swap them is the rounding of the rule's own
    steps from those vertices on, `loc` per hit: the farther edge is no challenger where the depths lie more than loc + loc apart."""
    win = np.full(ncell, -1, np.int64)
    idx = np.nonzero(certain)[0]
    order = idx[np.lexsort((edge[idx], body[idx], depth[idx], cell[idx]))]
    first = np.ones(len(order), bool)
    first[1:] = cell[order][1:] != cell[order][:-1]
    w = order[first]
    win[cell[w]] = w
    hi = np.full(ncell, np.inf)
    hi[cell[w]] = depth[w] + dd[w]
    bound = np.zeros(ncell)
    bound[cell[w]] = dd[w]
    cand = np.nonzero(possible | certain)[0]
    wc = win[cell[cand]]
    same = (wc >= 0) & (canon[body[cand]] == canon[body[wc]])
    twin = same & (edge[cand] == edge[wc]) & (depth[cand] == depth[wc])
    twin |= (wc >= 0) & certain[cand] & flat[cand] & flat[wc] & (depth[cand] == depth[wc])       # equal keys but for the index
    chall = (cand != wc) & ~twin & (lo[cand] <= hi[cell[cand]])
    own = chall & same
    if loc is not None:
        own &= ~(certain[cand] & firm[cand] & (depth[cand] - depth[wc] > loc[cand] + loc[wc]))
        chall &= own | ~same
    und = np.zeros(ncell, bool)
    und[cell[cand[chall & ~own]]] = True
    und_edge = np.zeros(ncell, bool)
    und_edge[cell[cand[own]]] = True
    np.maximum.at(bound, cell[cand[own]], depth[wc[own]] - lo[cand[own]])
    touched = np.zeros(ncell, bool)
    touched[cell[cand]] = True
    hidden = np.zeros(ncell, bool)
    behind = certain[cand] & (wc >= 0) & ~same
    hidden[cell[cand[behind]]] = True
    return win, und, und_edge, bound, touched, hidden & ~und


def _shade(s, ds, edge, skin):
    """colour of edge parameter s (clamped to [0, 1]) on edge `edge`: (rgba, bound, undecided: a texel index could flip)"""
    s = np.clip(s, 0.0, 1.0)
    zero, one = np.zeros(len(s)), np.ones(len(s))
    u = np.select([edge == 0, edge == 1], [zero, s], 1.0 - s)
    v = np.select([edge == 0, edge == 1], [s, one], 1.0 - s)
    uvar, vvar = edge != 0, edge != 1
    th, tw = skin.shape[:2]
    und = np.zeros(len(s), bool)
    exact = (ds == 0) & ((s == 0) | (s == 1))            # clamped to an end: the index is the first or the last texel, surely
    if tw > 1:
        und |= uvar & ~exact & (np.abs(u * tw - np.rint(u * tw)) <= ds * tw + 4 * U * tw)
    if th > 1:
        und |= vvar & ~exact & (np.abs(v * th - np.rint(v * th)) <= ds * th + 4 * U * th)
    ix = np.minimum(tw - 1, np.floor(u * tw).astype(np.int64))
    iy = np.minimum(th - 1, np.floor(v * th).astype(np.int64))
    tex = np.asarray(skin, np.float64)[iy, ix]
    f = 1.0 - ((u - 0.5) ** 2 + (v - 0.5) ** 2)
    df = 2.0 * (np.abs(u - 0.5) * uvar + np.abs(v - 0.5) * vvar) * ds + 6 * U
    rgba = np.ones((len(s), 4))
    bound = np.zeros((len(s), 4))
    rgba[:, :3] = tex[:, :3] * f[:, None]
    bound[:, :3] = np.abs(tex[:, :3]) * df[:, None] + 4 * U * np.abs(rgba[:, :3])
    return rgba, bound, und


def _canon(pos, vel):
    """canon[j]: the lowest index whose position and velocity are body j's, word for word"""
    rec = np.ascontiguousarray(np.concatenate([np.asarray(pos, np.float32), np.asarray(vel, np.float32)], 1)).view(np.uint32)
    seen, canon = {}, np.empty(len(rec), np.int64)
    for j, r in enumerate(map(bytes, rec)):
        canon[j] = seen.setdefault(r, j)
    return canon


def _count(stats, win, j, k, c, cut, hidden):
    """what the case list's coverage conditions ask about the decided winners"""
    wj, wk = j[win], k[win]
    stats["edge"] += np.bincount(wk, minlength=3)
    stats["cut"] += cut[wj, wk].sum(0)
    w0, w1 = c["W"][wj, wk], c["W"][wj, (wk + 1) % 3]
    stats["unequal_w"] += int(((w0 > 0) & (w1 > 0) & (np.abs(w0 - w1) > 0.1 * np.maximum(w0, w1))).sum())
    stats["hidden"] += int(hidden.sum())


def new_stats():
    return dict(edge=np.zeros(3, np.int64), cut=np.zeros(4, np.int64), unequal_w=0, hidden=0, xmajor=0, ymajor=0)


def eye_rows(pos, vel, eyes, width, up, fovy_deg, aspect, near=1.0, far=10000.0, see_self=False, skin=None, samples=False,
             model=MODEL):
    """The rows of the eyes `eyes` (body indices) over every body of (pos, vel).  Returns a namespace of arrays over (eye, column)
    -- with `samples`, (eye, column, 8) for ids, depth, ddepth, und, touched --: ids, depth and its bound ddepth, und (undecided),
    touched (a body may hit the cell); rgba, drgba, und_rgba over (eye, column); without `samples` also edge, s, ds of the winner;
    per eye `hit` (n,): the body may hit some cell, and `und_lo` (n,): the least depth - bound of its possible hits in undecided
    cells; `stats`."""
    L = lens(fovy_deg, aspect, near, far)
    skin = WHITE if skin is None else np.asarray(skin, np.float64)
    verts, mag = outline(pos, vel, model)
    canon = _canon(pos, vel)
    n, E, h = len(verts), len(eyes), width / 2.0
    offs = OFFSETS if samples else np.array([0.5])
    K = len(offs)
    out = types.SimpleNamespace(ids=np.full((E, width, K), NONE, np.uint32), depth=np.ones((E, width, K)), ddepth=np.zeros((E, width, K)),
                                und=np.zeros((E, width, K), bool), und_edge=np.zeros((E, width, K), bool), und_colour=np.zeros((E, width, K), bool), touched=np.zeros((E, width, K), bool),
                                rgba=np.tile(CLEAR, (E, width, 1)), drgba=np.zeros((E, width, 4)), und_rgba=np.zeros((E, width), bool),
                                edge=np.full((E, width, K), -1, np.int64), s=np.zeros((E, width, K)), ds=np.zeros((E, width, K)),
                                hit=np.zeros((E, n), bool), und_lo=np.full((E, n), np.inf), stats=new_stats(), samples=samples)
    pos64, vel64 = np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    for ei, e in enumerate(eyes):
        b = basis(vel64[e], up)
        if not np.isfinite(b.s).all():
            continue                                                   # no heading: the camera is undefined and the row is empty
        c = _clip(verts, mag, pos64[e], b, L)
        lo, hi, vis, cut = _visible(c, L)
        if not see_self:
            vis[e] = False
        j, k = np.nonzero(vis)
        if not len(j):
            continue
        with np.errstate(all="ignore"):
            ends = []
            for t in (lo[j, k], hi[j, k]):
                xe = c["X"][j, k] + t * (c["X"][j, (k + 1) % 3] - c["X"][j, k])
                we = c["W"][j, k] + t * (c["W"][j, (k + 1) % 3] - c["W"][j, k])
                ends.append(xe / we * h + h)
            a, z = np.minimum(*ends), np.maximum(*ends)
            reach_x = np.maximum(np.abs(ends[0]), np.abs(ends[1]))               # the projected ends' |xs|; not finite: no claim below
            a, z = np.where(np.isfinite(a), a, 0.0), np.where(np.isfinite(z), z, width)
        c_lo = np.clip(np.floor(a) - 2, 0, width).astype(np.int64)
        c_hi = np.clip(np.ceil(z) + 2, 0, width).astype(np.int64)
        span = np.maximum(c_hi - c_lo, 0)
        if span.sum() == 0:
            continue
        seg = np.repeat(np.arange(len(j)), span)
        col = np.arange(span.sum()) - np.repeat(np.cumsum(span) - span, span) + c_lo[seg]
        pj, pk = np.repeat(j[seg], K), np.repeat(k[seg], K)
        pcol, psm = np.repeat(col, K), np.tile(np.arange(K), len(col))
        x = pcol + offs[psm]
        ht = _hits(c, L, pj, pk, (x - h) / h, "X")
        cell = pcol * K + psm
        # what the rule's own steps add from the binary32 clip vertices on: the quotient z / w and the last sum (3 units of 2^-24 of
        # a depth <= 1); for an edge that a plane cuts, the cut end (3 roundings on |z|, |w| of both ends, over a w >= near); the
        # interpolation along screen x (projection and parameter: 8 roundings on |xs| + W) times the depth's slope in screen x
        with np.errstate(all="ignore"):
            pk1 = (pk + 1) % 3
            ends_w = np.abs(c["W"][pj, pk]) + np.abs(c["W"][pj, pk1])
            cut_end = cut[pj, pk].any(-1) * 3 * U * (ends_w + L.A * (ends_w + 2 * L.near)) / L.near
            slope = L.A * L.near * np.abs(ht.dW) / (h * np.abs(ht.DX * ht.w - ht.X * ht.dW))
            loc = 3 * U + cut_end + slope * 8 * U * (np.repeat(reach_x[seg], K) + width)
            loc = np.where(np.isfinite(loc), loc, np.inf)
            ax, aw = c["X"][:, 1] - c["X"][:, 0], c["W"][:, 1] - c["W"][:, 0]
            bx, bw = c["X"][:, 2] - c["X"][:, 0], c["W"][:, 2] - c["W"][:, 0]
            firm = np.abs(ax * bw - aw * bx) > 2 * R * U * (c["SX"].max(1) * (np.abs(aw) + np.abs(bw)) + c["SW"].max(1) * (np.abs(ax) + np.abs(bx)))
        win, und, und_edge, bound, touched, hidden = _resolve(cell, width * K, ht.depth, ht.dd, ht.lo, pj, pk, ht.certain, ht.possible, canon, ht.flat,
                                                             loc, firm[pj])
        und, touched, win = und.reshape(width, K), touched.reshape(width, K), win.reshape(width, K)
        und_edge, bound = und_edge.reshape(width, K), bound.reshape(width, K)
        out.und[ei], out.touched[ei], out.und_edge[ei] = und, touched, und_edge
        got = (win >= 0) & ~und
        wi = win[got]
        out.ids[ei][got], out.depth[ei][got], out.ddepth[ei][got] = pj[wi], ht.depth[wi], bound[got]
        out.edge[ei][got], out.s[ei][got], out.ds[ei][got] = pk[wi], ht.s[wi], ht.ds[wi]
        _count(out.stats, wi, pj, pk, c, cut, hidden)
        maybe = ht.possible | ht.certain
        out.hit[ei][np.unique(pj[maybe])] = True
        inund = maybe & und.reshape(-1)[cell]
        np.minimum.at(out.und_lo[ei], pj[inund], ht.lo[inund])
        # colour: the winner's (body, edge) at the column centre
        cc, kk = np.nonzero(got)
        wj, wk = pj[win[cc, kk]], pk[win[cc, kk]]
        if samples:
            hc = _hits(c, L, wj, wk, (cc + 0.5 - h) / h, "X")
            # a centre whose parameter surely lies beyond an end is clamped to that end exactly, however badly it is conditioned
            beyond = hc.finite & ((hc.s - hc.ds >= 1) | (hc.s + hc.ds <= 0))
            cu = ~hc.finite | ~(hc.w - hc.dw > 0) | (~(hc.ds <= 0.25) & ~beyond)
            s_c, ds_c = np.where(hc.finite, hc.s, 0.0), np.where(hc.finite & ~beyond, hc.ds, 0.0)
        else:
            s_c, ds_c, cu = ht.s[win[cc, kk]], ht.ds[win[cc, kk]], np.zeros(len(cc), bool)
        rgba, bound, tu = _shade(s_c, ds_c, wk, skin)
        a_k = np.tile(CLEAR, (width, K, 1))
        b_k = np.zeros((width, K, 4))
        a_k[cc, kk], b_k[cc, kk] = rgba, bound
        bad = und | und_edge
        bad[cc, kk] |= cu | tu | (bound.max(1) > MAX_COLOUR_BOUND)
        out.und_colour[ei] = bad
        out.rgba[ei] = a_k.mean(1)
        out.drgba[ei] = b_k.mean(1) + (4 * U * np.abs(a_k).max(1) if samples else 0.0)
        out.drgba[ei][..., 3] = 0.0
        out.und_rgba[ei] = bad.any(1)
    if not samples:
        for name in ("ids", "depth", "ddepth", "und", "und_edge", "und_colour", "touched", "edge", "s", "ds"):
            setattr(out, name, getattr(out, name)[..., 0])
    return out


def frame(pos, vel, eye, direction, up, fovy_deg, aspect, extent, near=1.0, far=10000.0, skin=None):
    """The frame of extent (W, H) through the camera at `eye` looking along `direction`.  Returns a namespace of (H, W) arrays, row 0
    the top: ids, depth, ddepth, und, touched, rgba, drgba, und_rgba, edge, xmajor (the winner's edge is x-major); `stats`."""
    L = lens(fovy_deg, aspect, near, far)
    skin = WHITE if skin is None else np.asarray(skin, np.float64)
    W, H = extent
    hw, hh = W / 2.0, H / 2.0
    verts, mag = outline(pos, vel)
    canon = _canon(pos, vel)
    b = basis(direction, up)
    c = _clip(verts, mag, eye, b, L)
    lo, hi, vis, cut = _visible(c, L)
    i1 = np.array([1, 2, 0])
    with np.errstate(all="ignore"):
        end = []
        for t in (lo, hi):
            xe, ye, we = (c[a] + t * (c[a][:, i1] - c[a]) for a in ("X", "Y", "W"))
            bx = hw * R * U * (c["SX"] + np.abs(xe / we) * c["SW"]) / we
            by = hh * R * U * (c["SY"] + np.abs(ye / we) * c["SW"]) / we
            end.append((xe / we * hw + hw, hh - ye / we * hh, np.maximum(bx, bx[:, i1]), np.maximum(by, by[:, i1])))
        dx, dy = np.abs(end[1][0] - end[0][0]), np.abs(end[1][1] - end[0][1])
        xmajor = dx >= dy
        und_major = ~(np.abs(dx - dy) > end[0][2] + end[1][2] + end[0][3] + end[1][3] + 8 * U * (W + H))
    parts = []
    for axis, lim, half, blim in (("X", W, hw, H), ("Y", H, hh, W)):
        sel = vis & ((xmajor if axis == "X" else ~xmajor) | und_major)
        j, k = np.nonzero(sel)
        if not len(j):
            continue
        a0, a1 = (end[0][0], end[1][0]) if axis == "X" else (end[0][1], end[1][1])
        a, z = np.minimum(a0, a1)[j, k], np.maximum(a0, a1)[j, k]
        a, z = np.where(np.isfinite(a), a, 0.0), np.where(np.isfinite(z), z, lim)
        m_lo = np.clip(np.floor(a) - 2, 0, lim).astype(np.int64)
        m_hi = np.clip(np.ceil(z) + 2, 0, lim).astype(np.int64)
        span = np.maximum(m_hi - m_lo, 0)
        if span.sum() == 0:
            continue
        seg = np.repeat(np.arange(len(j)), span)
        m = np.arange(span.sum()) - np.repeat(np.cumsum(span) - span, span) + m_lo[seg]
        pj, pk = j[seg], k[seg]
        mc = m + 0.5
        nm = (mc - hw) / hw if axis == "X" else (hh - mc) / hh
        ht = _hits(c, L, pj, pk, nm, axis)
        with np.errstate(all="ignore"):
            if axis == "X":       # the minor coordinate is the row
                q, bq, Dq, half_m = ht.Y, ht.bY, ht.DY, hh
                minor = hh - q / ht.w * hh
            else:
                q, bq, Dq, half_m = ht.X, ht.bX, ht.DX, hw
                minor = q / ht.w * hw + hw
            dminor = half_m * ((bq + np.abs(q / ht.w) * ht.bW) / ht.w + np.abs(Dq * ht.w - q * ht.dW) / (ht.w * ht.w) * ht.ds) + 4 * U * blim
            ok = np.isfinite(minor) & np.isfinite(dminor)
            minor, dminor = np.where(ok, minor, -1.0), np.where(ok, dminor, 0.0)
            inside = ok & (minor - dminor >= 0) & (minor + dminor < blim)
            near_in = ok & (minor + dminor >= 0) & (minor - dminor < blim)
            f0, fa, fb = np.floor(minor), np.floor(minor - dminor), np.floor(minor + dminor)
            sure = inside & (fa == f0) & (fb == f0) & ~und_major[pj, pk]
        certain, possible = ht.certain & sure, (ht.possible | ht.certain) & near_in
        is_x = np.full(len(m), axis == "X")
        # the pixel the floor names holds the hit; where the floor could fall either way, the neighbours hold a possible hit too
        for f, cert in ((f0, certain), (fa, None), (fb, None)):
            keep = possible & (f >= 0) & (f < blim) if cert is not None else possible & (f != f0) & (f >= 0) & (f < blim)
            fi = np.where(keep, f, 0).astype(np.int64)
            pixel = fi * W + m if axis == "X" else m * W + fi
            cert = certain if cert is not None else np.zeros(len(m), bool)
            parts.append([a[keep] for a in (pixel, ht.depth, ht.dd, ht.lo, pj, pk, cert, possible, ht.s, ht.ds, is_x, ht.flat)])
    out = types.SimpleNamespace(ids=np.full(W * H, NONE, np.uint32), depth=np.ones(W * H), ddepth=np.zeros(W * H), und=np.zeros(W * H, bool),
                                touched=np.zeros(W * H, bool), und_edge=np.zeros(W * H, bool), rgba=np.tile(CLEAR, (W * H, 1)), drgba=np.zeros((W * H, 4)),
                                und_rgba=np.zeros(W * H, bool), edge=np.full(W * H, -1, np.int64), xmajor=np.zeros(W * H, bool),
                                stats=new_stats())
    if parts:
        pixel, depth, dd, lo, pj, pk, certain, possible, s, ds, is_x, flat = (np.concatenate([p[i] for p in parts]) for i in range(12))
        win, und, und_edge, bound, touched, hidden = _resolve(pixel, W * H, depth, dd, lo, pj, pk, certain, possible, canon, flat)
        out.und, out.touched, out.und_edge = und, touched, und_edge
        got = (win >= 0) & ~und
        wi = win[got]
        out.ids[got], out.depth[got], out.ddepth[got], out.edge[got], out.xmajor[got] = pj[wi], depth[wi], bound[got], pk[wi], is_x[wi]
        _count(out.stats, wi, pj, pk, c, cut, hidden)
        out.stats["xmajor"], out.stats["ymajor"] = int(is_x[wi].sum()), int((~is_x[wi]).sum())
        rgba, bound, tu = _shade(s[wi], ds[wi], pk[wi], skin)
        out.rgba[got], out.drgba[got] = rgba, bound
        out.und_rgba = und | und_edge
        out.und_rgba[np.nonzero(got)[0][tu | (bound.max(1) > MAX_COLOUR_BOUND)]] = True
    for name in ("ids", "depth", "ddepth", "und", "und_edge", "touched", "und_rgba", "edge", "xmajor"):
        setattr(out, name, getattr(out, name).reshape(H, W))
    out.und_colour = out.und_rgba
    out.rgba, out.drgba = out.rgba.reshape(H, W, 4), out.drgba.reshape(H, W, 4)
    return out


# -- comparisons ------------------------------------------------------------------------------------------------------------------------
def _where(axes, index, labels=None):
    parts = []
    for a, i in zip(axes, index):
        parts.append(f"{a} {labels[int(i)] if labels is not None and a == axes[0] else int(i)}")
    return ", ".join(parts)


def compare(case, ref, ids, depth, rgba=None, axes=("eye", "column"), labels=None):
    """Decided cells in full: ids exactly, depth and rgba within their bounds, empty cells exactly (NONE, 1.0, the clear colour).
    `labels`: the first axis' names (the eyes' body indices).  Returns the largest error / bound per output; raises AssertionError
    naming the case, the cell, the body and the value against reference +- bound."""
    ids, depth = np.asarray(ids), np.asarray(depth, np.float64)
    assert ids.shape == ref.ids.shape and depth.shape == ref.depth.shape, f"{case}: shapes {ids.shape}, {depth.shape} against {ref.ids.shape}"
    ax = axes + ("sample",) if ids.ndim == len(axes) + 1 else axes
    decided = ~ref.und
    bad = decided & (ids != ref.ids)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{case}: {_where(ax, i, labels)}: body {int(ids[i])} (depth {depth[i]:.9g}) against the reference's "
                             f"{int(ref.ids[i])} (depth {ref.depth[i]:.9g} +- {ref.ddepth[i]:.3g}); {int(bad.sum())} decided cells differ")
    covered = decided & (ref.ids != NONE)
    err = np.abs(depth - ref.depth)
    bad = (covered & ~(err <= ref.ddepth)) | (decided & ~covered & (depth != 1.0))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{case}: {_where(ax, i, labels)}: body {int(ids[i])}: depth {depth[i]:.9g} against {ref.depth[i]:.9g} +- "
                             f"{ref.ddepth[i]:.3g} (off by {err[i]:.3g}); {int(bad.sum())} decided cells differ")
    # (where another edge of the winner may be the nearer one the bound spans both edges: those cells' ratio is kept apart)
    one, two = covered & ~ref.und_edge, covered & ref.und_edge
    ratios = dict(depth=float((err[one] / ref.ddepth[one]).max(initial=0.0)), depth_two_edges=float((err[two] / ref.ddepth[two]).max(initial=0.0)))
    if rgba is not None:
        rgba32 = np.ascontiguousarray(rgba, np.float32)
        rgba = rgba32.astype(np.float64)
        assert rgba.shape == ref.rgba.shape, f"{case}: rgba {rgba.shape} against {ref.rgba.shape}"
        ok = ~ref.und_rgba
        empty = ok & ~(ref.touched.any(-1) if ref.touched.ndim > ref.und_rgba.ndim else ref.touched)
        cerr = np.abs(rgba - ref.rgba)
        bad = ok[..., None] & ~(cerr <= ref.drgba)
        bad |= empty[..., None] & (rgba32.view(np.uint32) != CLEAR.astype(np.float32).view(np.uint32))
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            body = ids[i[:-1]]
            raise AssertionError(f"{case}: {_where(axes, i[:-1], labels)}, channel {i[-1]}: body {body.tolist()}: colour {rgba[i]:.9g} against "
                                 f"{ref.rgba[i]:.9g} +- {ref.drgba[i]:.3g} (off by {cerr[i]:.3g}); {int(bad.sum())} decided values differ")
        live = ok[..., None] & (ref.drgba > 0)
        ratios["rgba"] = float((cerr[live] / ref.drgba[live]).max(initial=0.0))
    return ratios


def compare_seen(case, ref, count, ids, depth, labels=None):
    """The seen sets of the device against the one-sample rows `ref`: every body that wins a decided column is a member; a member's
    nearest depth is within bound of the reference's least over decided columns, or nearer by way of an undecided column; every
    member may hit at least one column.  Returns the largest error / bound (the bound: from that least to the limit on its side)."""
    worst = 0.0
    for e in range(len(ref.ids)):
        who = f"{case}: eye {labels[e] if labels is not None else e}"
        k = int(count[e])
        members, mdepth = np.asarray(ids[e][:k]).astype(np.int64), np.asarray(depth[e][:k], np.float64)
        assert (np.diff(members) > 0).all(), f"{who}: the seen set is not ascending"
        won = ~ref.und[e] & (ref.ids[e] != NONE)
        winners = np.unique(ref.ids[e][won]).astype(np.int64)
        missing = np.setdiff1d(winners, members)
        assert not len(missing), f"{who}: body {int(missing[0])} wins decided column {int(np.nonzero(won & (ref.ids[e] == missing[0]))[0][0])} and is not in the seen set"
        for m, d in zip(members, mdepth):
            assert m < ref.hit.shape[1] and ref.hit[e, m], f"{who}: member {int(m)} hits no column of the reference row"
            cols = won & (ref.ids[e] == m)
            least = lo_lim = hi_lim = np.inf
            if cols.any():        # the least over decided columns, each with its own bound (a two-edge cell's reaches down to the other edge)
                least = ref.depth[e][cols].min()
                lo_lim, hi_lim = (ref.depth[e] - ref.ddepth[e])[cols].min(), (ref.depth[e] + ref.ddepth[e])[cols].min()
            assert d <= hi_lim, f"{who}: member {int(m)}: nearest depth {d!r} against the reference's {least!r}, at most {hi_lim!r}"
            assert d >= min(lo_lim, ref.und_lo[e, m]), \
                f"{who}: member {int(m)}: nearest depth {d!r} is nearer than the reference's {least!r}, at least {lo_lim!r}, and than every undecided column ({ref.und_lo[e, m]!r})"
            if cols.any() and d >= lo_lim:
                worst = max(worst, (d - least) / (hi_lim - least) if d >= least else (least - d) / (least - lo_lim))
    return float(worst)
