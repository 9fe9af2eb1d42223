"""numpy float32 restatement of the frame rule on top of eyes_restatement.py and eyes_colour_restatement.py:
what the reference's display pass leaves in its W x H target (src/main.rs:948-960) -- per pixel the instance that wrote it, the
depth attachment's value, the linear colour the fragment shader writes and the byte an sRGB target stores.

TEST INFRASTRUCTURE.  The kernels (nenbody_amd/csrc/nb_frame.inc) and this module implement the same rule independently; the GPU
tests compare them bit for bit.  Every step is one binary32 operation on numpy float32 arrays (IEEE, round to nearest, no fusion),
in the order the rule writes it.  The camera is one (4, 4) float32 array and the model matrices an (n, 4, 4) one whose [k] is
column k, as for the eyes.
"""
import numpy as np

import eyes_colour_restatement as K
import eyes_restatement as R

F = np.float32


def ortho_camera(W, H, sx=1, sy=1):
    """A caller camera for hand checks: columns (2 sx/W, 0, 0, 0), (0, 2 sy/H, 0, 0), (0, 0, 0, 0), (0, 0, 0.5, 1), so that with W,
    H, sx and sy powers of two xs = sx x + W/2 and ys = H/2 - sy y exactly, and every depth is 0.5."""
    c = np.zeros((4, 4), F)
    c[0, 0] = F(2 * sx) / F(W)
    c[1, 1] = F(2 * sy) / F(H)
    c[3, 2] = 0.5
    c[3, 3] = 1
    return c


def edges(cam, inst, W, H):
    """F1-F3 for the 3n edges of n bodies, edge 3 j + k = edge k of body j: a dict of (3n,) arrays -- keep, the clip parameters and
    the clipped ends' w (section 10 step 7 needs them), the projected ends (xs, ys, d), `outside`: an end lies outside a plane,
    `cut` ((3n, 4): boundary B1 .. B4 has one end outside it and the other not) and `w_dropped` (the edge passes the clip and is
    dropped for an end with w <= 0)."""
    world = R.world_vertices(inst)
    P = R.clip_vertices(np.ascontiguousarray(cam, F).reshape(1, 4, 4), world)[0]            # F1: (n, 3, 4)
    P0 = P[:, [a for a, _ in R.EDGES], :].reshape(-1, 4)
    P1 = P[:, [b for _, b in R.EDGES], :].reshape(-1, 4)
    m = len(P0)
    t_in, t_out, keep, outside = np.zeros(m, F), np.ones(m, F), np.ones(m, bool), np.zeros(m, bool)
    cut = np.zeros((m, 4), bool)
    with np.errstate(all="ignore"):
        def bounds(p):
            y, z, w = p[:, 1], p[:, 2], p[:, 3]
            return (z, w - z, w + y, w - y)                                                  # B1 .. B4

        for k, (b0, b1) in enumerate(zip(bounds(P0), bounds(P1))):                           # F2
            keep &= ~((b0 < 0) & (b1 < 0))
            outside |= (b0 < 0) | (b1 < 0)
            cut[:, k] = ((b0 < 0) & (b1 >= 0)) | ((b1 < 0) & (b0 >= 0))
            r = b0 / (b0 - b1)
            t_in = np.where((b0 < 0) & (b1 >= 0) & (r > t_in), r, t_in)
            t_out = np.where((b1 < 0) & (b0 >= 0) & (r < t_out), r, t_out)
        keep &= ~(t_in > t_out)
        D = P1 - P0
        Q0 = np.where((t_in > 0)[:, None], P0 + t_in[:, None] * D, P0)
        Q1 = np.where((t_out < 1)[:, None], P0 + t_out[:, None] * D, P1)
        positive = (Q0[:, 3] > 0) & (Q1[:, 3] > 0)
        w_dropped = keep & ~positive
        keep &= positive
        h, g = F(W) * F(0.5), F(H) * F(0.5)                                                  # F3
        e = dict(keep=keep, outside=outside, cut=cut, w_dropped=w_dropped, t_in=t_in, t_out=t_out, w0=Q0[:, 3], w1=Q1[:, 3])
        e["xs0"] = (Q0[:, 0] / Q0[:, 3]) * h + h
        e["xs1"] = (Q1[:, 0] / Q1[:, 3]) * h + h
        e["ys0"] = g - (Q0[:, 1] / Q0[:, 3]) * g
        e["ys1"] = g - (Q1[:, 1] / Q1[:, 3]) * g
        e["d0"] = Q0[:, 2] / Q0[:, 3]
        e["d1"] = Q1[:, 2] / Q1[:, 3]
        dx, dy = e["xs1"] - e["xs0"], e["ys1"] - e["ys0"]                                    # F4: the major axis
        xm = np.abs(dx) >= np.abs(dy)                                                        # a NaN: False, the y-major way
        e["xmajor"] = xm
        e["a0"], e["a1"], e["da"] = np.where(xm, e["xs0"], e["ys0"]), np.where(xm, e["xs1"], e["ys1"]), np.where(xm, dx, dy)
        e["b0"], e["db"] = np.where(xm, e["ys0"], e["xs0"]), np.where(xm, dy, dx)
        e["blim"] = np.where(xm, F(H), F(W)).astype(F)
    return e


def _steps(e, idx, m, W, far=None):
    """F4 and F5 for step m[i] along the major axis of edge idx[i]: (ok, t, pixel, d) -- ok: the step yields a pixel and its depth
    is a candidate; pixel = row * W + column; d after the clamp to +0.  far, a list, receives the steps that yield a pixel whose
    depth is >= 1: no candidate."""
    with np.errstate(all="ignore"):
        a0, a1 = e["a0"][idx], e["a1"][idx]
        amin, amax = np.where(a0 <= a1, a0, a1), np.where(a0 <= a1, a1, a0)
        mc = m.astype(F) + F(0.5)                                                            # exact
        ok = (amin <= mc) & (mc < amax)
        t = (mc - a0) / e["da"][idx]
        o = e["b0"][idx] + t * e["db"][idx]
        ok &= (o >= 0) & (o < e["blim"][idx])
        d = e["d0"][idx] + t * (e["d1"][idx] - e["d0"][idx])
        if far is not None:
            far.append(ok & (d >= F(1)))
        ok &= d < F(1)
        d = np.where(d > 0, d, F(0)).astype(F)                                               # !(d > 0) -> +0
        f = np.where(ok, np.floor(o), 0).astype(np.int64)
    pixel = np.where(e["xmajor"][idx], f * W + m, m * W + f)
    return ok, t, pixel, d


def frame(cam, inst, W, H, skin=None, stats=None):
    """The rule F1-F6 for one camera over every body of `inst`; skin: (th, tw, 4) linear float32, row 0 first (None: 1 x 1 white).
    Returns (ids uint32 (H, W), depth float32 (H, W), rgba float32 (H, W, 4), bgra8 uint32 (H, W)); row 0 is the top.
    `stats`, a dict, receives: "kept" edges (after F2), "clipped" (kept with an end outside a plane), "xmajor" / "ymajor" (kept
    edges with a step to try), pixel "writes" (candidates), "covered" pixels, distinct "depths" among them, visible "bodies", the
    "longest" edge in pixel writes ("longest_x", "longest_y": among the x-major and the y-major edges), "edge": how many pixels
    each edge index wins, "cut" (4 entries: kept edges that boundary B1 .. B4 cuts), "w_dropped" (edges that pass the clip and are
    dropped for an end with w <= 0) and "rejected_far" (steps that yield a pixel whose depth is >= 1)."""
    inst = np.ascontiguousarray(inst, F).reshape(-1, 4, 4)
    skin = K.WHITE if skin is None else np.ascontiguousarray(skin, F)
    th, tw = skin.shape[:2]
    n = len(inst)
    e = edges(cam, inst, W, H)
    keys = np.full(W * H, R.EMPTY, np.uint64)
    st = dict(kept=int(e["keep"].sum()), clipped=int((e["keep"] & e["outside"]).sum()), xmajor=0, ymajor=0, writes=0, longest=0,
              longest_x=0, longest_y=0, rejected_far=0, w_dropped=int(e["w_dropped"].sum()),
              cut=(e["cut"] & e["keep"][:, None]).sum(0).astype(np.int64))
    with np.errstate(all="ignore"):
        amin, amax = np.minimum(e["a0"], e["a1"]), np.maximum(e["a0"], e["a1"])              # (a NaN end: NaN, dropped next)
        live = e["keep"] & (amin <= amax)
        alim = np.where(e["xmajor"], W, H).astype(np.float64)
        # the steps that can be covered, a superset: the exact test in _steps decides
        lo = np.clip(np.floor(np.maximum(amin.astype(np.float64), -4.0)) - 1, 0, alim)
        hi = np.clip(np.ceil(np.minimum(amax.astype(np.float64), alim + 4.0)) + 1, 0, alim)
    lo, hi = np.where(live, lo, 0).astype(np.int64), np.where(live, hi, 0).astype(np.int64)
    span = np.maximum(hi - lo, 0)
    st["xmajor"], st["ymajor"] = int(((span > 0) & e["xmajor"]).sum()), int(((span > 0) & ~e["xmajor"]).sum())
    total = int(span.sum())
    if total:
        idx = np.repeat(np.arange(3 * n), span)
        m = np.arange(total) - np.repeat(np.cumsum(span) - span, span) + lo[idx]
        far = []
        ok, _, pixel, d = _steps(e, idx, m, W, far)
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (idx // 3).astype(np.uint64)   # F5
        np.minimum.at(keys, pixel[ok], key[ok])
        st["writes"] = int(ok.sum())
        per_edge = np.bincount(idx[ok], minlength=3 * n)
        st["longest"] = int(per_edge.max()) if ok.any() else 0
        st["longest_x"], st["longest_y"] = int(per_edge[e["xmajor"]].max(initial=0)), int(per_edge[~e["xmajor"]].max(initial=0))
        st["rejected_far"] = int(far[0].sum())
    none = keys == R.EMPTY
    ids = np.where(none, np.uint32(R.NONE), (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    depth = np.where(none, F(1), (keys >> np.uint64(32)).astype(np.uint32).view(F))
    rgba = np.empty((W * H, 4), F)
    rgba[:] = K.CLEAR                                                                        # step 11
    p = np.nonzero(~none)[0]
    won = np.zeros(3, np.int64)
    if len(p):                                                                               # F6
        j = ids[p].astype(np.int64)
        want = depth[p].view(np.uint32)
        row, col = p // W, p % W
        edge = np.full(len(p), -1, np.int64)
        s = np.zeros(len(p), F)
        for k in range(3):                                                                   # step 6: the first edge in draw order
            idx = 3 * j + k
            ok, t, pixel, d = _steps(e, idx, np.where(e["xmajor"][idx], col, row), W)
            ok &= e["keep"][idx] & (pixel == p) & (d.view(np.uint32) == want) & (edge < 0)
            with np.errstate(all="ignore"):
                s0 = np.where(e["t_in"][idx] > 0, e["t_in"][idx], F(0))                      # step 7
                s1 = np.where(e["t_out"][idx] < 1, e["t_out"][idx], F(1))
                i0, i1 = F(1) / e["w0"][idx], F(1) / e["w1"][idx]
                a0, a1 = s0 * i0, s1 * i1
                num = a0 + t * (a1 - a0)
                den = i0 + t * (i1 - i0)
                sk = num / den
                sk = np.where(sk > 0, sk, F(0))
                sk = np.where(sk > 1, F(1), sk)
            edge[ok], s[ok] = k, sk[ok]
        assert (edge >= 0).all(), "a resolved pixel without a winning edge"
        one_minus = F(1) - s                                                                 # step 8
        u = np.select([edge == 0, edge == 1], [np.zeros(len(p), F), s], one_minus)
        v = np.select([edge == 0, edge == 1], [s, np.ones(len(p), F)], one_minus)
        ix = np.minimum(tw - 1, np.floor(u * F(tw)).astype(np.int64))                        # step 9
        iy = np.minimum(th - 1, np.floor(v * F(th)).astype(np.int64))
        tex = skin[iy, ix]
        du, dv = u - F(0.5), v - F(0.5)                                                      # step 10
        f = F(1) - (du * du + dv * dv)
        rgba[p, :3] = tex[:, :3] * f[:, None]
        rgba[p, 3] = 1
        won = np.bincount(edge, minlength=3)
    if stats is not None:
        st.update(covered=len(p), depths=len(np.unique(depth[p].view(np.uint32))), bodies=len(np.unique(ids[p])), edge=won)
        stats.update(st)
    bgra8 = np.full(W * H, K.pack_bgra8(K.CLEAR), np.uint32)                                 # (one encoding for the empty pixels)
    bgra8[p] = K.pack_bgra8(rgba[p])
    return ids.reshape(H, W), depth.reshape(H, W), rgba.reshape(H, W, 4), bgra8.reshape(H, W)


# -- the scenes the CPU and the GPU tests share ------------------------------------------------------------------------------------
def frame_constant(oracle, extent, horizontal_fov_deg=90.0):
    """The reference's scene constant formed by the oracle: camera_constant(90 / a, a, 1, 10000), a = (float)W / (float)H."""
    a = F(extent[0]) / F(extent[1])
    return oracle.camera_constant(float(F(horizontal_fov_deg) / a), float(a), 1.0, 10000.0)


def camera(oracle, eye, direction, up, cp):
    return oracle.cameras(np.array([eye], F), np.array([direction], F), np.array(up, F), cp)[0]


def scene_camera(oracle, pos, extent, height=990.0, follow=0):
    """The reference's scene camera (src/main.rs:753-762, 940-942): above body `follow`, looking down, +x up."""
    return camera(oracle, [pos[follow, 0], pos[follow, 1], height], [0, 0, -1], [1, 0, 0], frame_constant(oracle, extent))


def spread_state(oracle, n, seed, spread):
    """init_state(n, seed) lifted off the plane: z uniform in +-spread, vz uniform in +-0.05, from default_rng(seed)."""
    pos, vel = oracle.init_state(n, seed)
    rng = np.random.default_rng(seed)
    pos[:, 2] = rng.uniform(-spread, spread, n).astype(F)
    vel[:, 2] = rng.uniform(-0.05, 0.05, n).astype(F)
    return pos, vel


def scene(oracle, name):
    """The scenes of the issue's table and the three-body scene: (pos, vel, camera, (W, H))."""
    if name == "reference":
        pos, vel = oracle.init_state(100, 1100)
        return pos, vel, scene_camera(oracle, pos, (1920, 1080)), (1920, 1080)
    if name == "side":
        pos, vel = spread_state(oracle, 300, 9, 30)
        return pos, vel, camera(oracle, [-150, 0, 40], [1, 0, -0.25], [0, 0, 1], frame_constant(oracle, (96, 64))), (96, 64)
    if name == "inside":
        pos, vel = spread_state(oracle, 2048, 5, 3)
        return pos, vel, camera(oracle, [pos[0, 0], pos[0, 1], 0.5], vel[0], [0, 0, 1], frame_constant(oracle, (96, 64))), (96, 64)
    if name == "top":
        pos, vel = spread_state(oracle, 257, 31, 30)
        return pos, vel, camera(oracle, [0, 0, 150], [0, 0, -1], [1, 0, 0], frame_constant(oracle, (128, 72))), (128, 72)
    if name == "three":
        pos = np.array([[0, 0, 0], [1.5, 0.5, 0], [-1, 2, 0]], F)
        vel = np.array([[1, 0, 0], [0.3, 1, 0], [-1, -0.2, 0]], F)
        cp = oracle.camera_constant(60.0, float(F(320) / F(180)), 1.0, 10000.0)
        return pos, vel, camera(oracle, [0, 0, 3], [0, 0, -1], [1, 0, 0], cp), (320, 180)
    raise KeyError(name)
