"""numpy float32 restatement of the colour row of the eye rule on top of eyes_restatement.py:
what the reference's colour attachment holds after the eye pass (src/main.rs:585-647, 962-998; shaders/scene.vert, scene.frag) --
per column the winning fragment's texture coordinate, one texel of the skin, the vignette, and the byte an sRGB target stores.

TEST INFRASTRUCTURE.  The kernel (nenbody_amd/csrc/nb_eyes.inc, eye_shade) and this module implement the same rule independently;
the GPU tests compare them bit for bit.  Every step is one binary32 operation on numpy float32 arrays, in the order the rule
writes it.  The two sRGB tables are computed here with `decimal` (50 digits) and rounded to binary32 by exact comparison of
fractions; the library commits its own as constants and the CPU tests compare the two.
"""
import decimal
import functools
from fractions import Fraction

import numpy as np

import eyes_restatement as R

F = np.float32
CLEAR = np.array([0.1, 0.2, 0.3, 1.0], np.float32)
WHITE = np.ones((1, 1, 4), np.float32)


# -- the sRGB tables ---------------------------------------------------------------------------------------------------------------
def srgb_eotf(e: Fraction) -> Fraction:
    """decode: e / 12.92 for e <= 0.04045, else ((e + 0.055) / 1.055) ^ 2.4 -- to 50 digits"""
    if e <= Fraction(4045, 100000):
        return e * Fraction(100, 1292)
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        x = (decimal.Decimal(e.numerator) / decimal.Decimal(e.denominator) + decimal.Decimal("0.055")) / decimal.Decimal("1.055")
        # x ^ 2.4 = x ^ 2 * (x ^ 2) ^ (1 / 5): a fifth root by Newton's iteration, no ln / exp
        sq = x * x
        r = decimal.Decimal(float(sq) ** 0.2)
        for _ in range(8):
            r = (4 * r + sq / (r * r * r * r)) / 5
        return Fraction(sq * r)


def to_binary32(v: Fraction) -> np.float32:
    """the binary32 nearest to v >= 0"""
    f = F(float(v))
    cands = [f, np.nextafter(f, F(np.inf)), np.nextafter(f, F(-np.inf))]
    return min(cands, key=lambda c: abs(Fraction(float(c)) - v))


@functools.lru_cache(None)
def _tables():
    d = np.array([to_binary32(srgb_eotf(Fraction(b, 255))) for b in range(256)], np.float32)
    t = np.array([F(0)] + [to_binary32(srgb_eotf(Fraction(2 * b - 1, 510))) for b in range(1, 256)], np.float32)
    return d, t


def decode_table():
    """D[b] = binary32(decode(b / 255))"""
    return _tables()[0].copy()


def encode_thresholds():
    """T[b] = binary32(decode((b - 0.5) / 255)) for b = 1 .. 255; T[0] = 0 is not a threshold"""
    return _tables()[1].copy()


def encode(linear):
    """the number of thresholds T[1..255] that are <= c; a NaN gives 0"""
    c = np.asarray(linear, np.float32)
    t = _tables()[1][1:]
    out = np.zeros(c.shape, np.int64)
    for th in t:                      # the definition, literally
        out += (th <= c)
    return out.astype(np.uint8)


def pack_bgra8(rgba):
    """(..., 4) linear floats -> uint32 whose bytes in memory are B, G, R, A (alpha gives 255)"""
    b = encode(rgba[..., :3]).astype(np.uint32)
    return b[..., 2] | (b[..., 1] << np.uint32(8)) | (b[..., 0] << np.uint32(16)) | np.uint32(0xFF000000)


def skin_from_srgb8(img):
    """an (th, tw, 4) uint8 Rgba8UnormSrgb image as linear float texels: colour through D, alpha / 255"""
    img = np.asarray(img, np.uint8)
    out = np.empty(img.shape, np.float32)
    out[..., :3] = _tables()[0][img[..., :3]]
    out[..., 3] = img[..., 3].astype(np.float32) / F(255)
    return out


# -- steps 6-11 --------------------------------------------------------------------------------------------------------------------
def _clip_edge(P0, P1, width):
    """steps 2 and 3 for m edges ((m, 4) clip vertices each), as eyes_restatement.segments states them, keeping what step 7 needs"""
    m = len(P0)
    t_in, t_out, keep = np.zeros(m, np.float32), np.ones(m, np.float32), np.ones(m, bool)
    with np.errstate(all="ignore"):
        def bounds(p):
            y, z, w = p[:, 1], p[:, 2], p[:, 3]
            return (z, w - z, w + y, w - y)                # near, far, y = -w, y = +w

        for b0, b1 in zip(bounds(P0), bounds(P1)):
            keep &= ~((b0 < 0) & (b1 < 0))
            r = b0 / (b0 - b1)
            t_in = np.where((b0 < 0) & (b1 >= 0) & (r > t_in), r, t_in)
            t_out = np.where((b1 < 0) & (b0 >= 0) & (r < t_out), r, t_out)
        keep &= ~(t_in > t_out)
        D = P1 - P0
        Q0 = np.where((t_in > 0)[:, None], P0 + t_in[:, None] * D, P0)
        Q1 = np.where((t_out < 1)[:, None], P0 + t_out[:, None] * D, P1)
        keep &= (Q0[:, 3] > 0) & (Q1[:, 3] > 0)
        h = F(width) * F(0.5)
        xs0 = (Q0[:, 0] / Q0[:, 3]) * h + h
        xs1 = (Q1[:, 0] / Q1[:, 3]) * h + h
        d0 = Q0[:, 2] / Q0[:, 3]
        d1 = Q1[:, 2] / Q1[:, 3]
    return keep, t_in, t_out, Q0[:, 3], Q1[:, 3], xs0, xs1, d0, d1


def colour(cams, inst, first, width, see_self=False, skin=None, chunk=8, stats=None):
    """The rule, steps 1-11, for eyes first .. first + len(cams) - 1 over every body of `inst`; skin: (th, tw, 4) linear float32,
    row 0 first (None: 1 x 1 white).  Returns (ids, depth, rgba float32 (E, width, 4), bgra8 uint32 (E, width)).
    `stats`, a dict, collects over calls: columns won by each edge ("edge"), winning columns whose edge has unequal end w
    ("unequal_w"), whose edge was cut where it enters ("s0>0"), and the columns that see a body ("covered") of "columns"; and what
    eyes_restatement.eyes counts."""
    cams = np.ascontiguousarray(cams, np.float32).reshape(-1, 4, 4)
    skin = WHITE if skin is None else np.ascontiguousarray(skin, np.float32)
    th, tw = skin.shape[:2]
    ids, depth = R.eyes(cams, inst, first, width, see_self, chunk, stats)
    E = len(cams)
    rgba = np.empty((E, width, 4), np.float32)
    rgba[:] = CLEAR                                                            # step 11
    world = R.world_vertices(inst)
    e_idx, c_idx = np.nonzero(ids != R.NONE)
    if len(e_idx):
        j = ids[e_idx, c_idx].astype(np.int64)
        want = depth[e_idx, c_idx].view(np.uint32)
        C, wv = cams[e_idx], world[j]                                          # (m, 4, 4) [k] = column k; (m, 3, 4)
        with np.errstate(all="ignore"):
            P = ((C[:, 0, None, :] * wv[:, :, 0, None] + C[:, 1, None, :] * wv[:, :, 1, None]) + C[:, 2, None, :] * wv[:, :, 2, None]) \
                + C[:, 3, None, :] * wv[:, :, 3, None]                         # step 1, (m, 3, 4)
        xc = c_idx.astype(np.float32) + F(0.5)
        m = len(j)
        edge = np.full(m, -1, np.int64)
        s = np.zeros(m, np.float32)
        uneq = np.zeros(m, bool)
        cut = np.zeros(m, bool)
        for k, (a, b) in enumerate(R.EDGES):                                   # step 6: the first edge in draw order
            keep, t_in, t_out, w0, w1, xs0, xs1, d0, d1 = _clip_edge(P[:, a], P[:, b], width)
            with np.errstate(all="ignore"):
                xa, xb = np.where(xs0 <= xs1, xs0, xs1), np.where(xs0 <= xs1, xs1, xs0)
                t = (xc - xs0) / (xs1 - xs0)
                d = d0 + t * (d1 - d0)
                ok = keep & (xa <= xc) & (xc < xb) & (d < F(1))
                d = np.where(d > 0, d, F(0))
                ok &= (d.view(np.uint32) == want) & (edge < 0)
                s0 = np.where(t_in > 0, t_in, F(0))                            # step 7
                s1 = np.where(t_out < 1, t_out, F(1))
                i0, i1 = F(1) / w0, F(1) / w1
                a0, a1 = s0 * i0, s1 * i1
                num = a0 + t * (a1 - a0)
                den = i0 + t * (i1 - i0)
                sk = num / den
                sk = np.where(sk > 0, sk, F(0))
                sk = np.where(sk > 1, F(1), sk)
            edge[ok], s[ok] = k, sk[ok]
            uneq |= ok & (w0 != w1)
            cut |= ok & (s0 > 0)
        assert (edge >= 0).all(), "a resolved column without a winning edge"
        one_minus = F(1) - s                                                   # step 8
        u = np.select([edge == 0, edge == 1], [np.zeros(m, np.float32), s], one_minus)
        v = np.select([edge == 0, edge == 1], [s, np.ones(m, np.float32)], one_minus)
        ix = np.minimum(tw - 1, np.floor(u * F(tw)).astype(np.int64))          # step 9
        iy = np.minimum(th - 1, np.floor(v * F(th)).astype(np.int64))
        tex = skin[iy, ix]
        du, dv = u - F(0.5), v - F(0.5)                                        # step 10
        m2 = du * du + dv * dv
        f = F(1) - m2
        rgba[e_idx, c_idx, :3] = tex[:, :3] * f[:, None]
        rgba[e_idx, c_idx, 3] = 1
        if stats is not None:
            stats["edge"] = stats.get("edge", np.zeros(3, np.int64)) + np.bincount(edge, minlength=3)
            stats["unequal_w"] = stats.get("unequal_w", 0) + int(uneq.sum())
            stats["s0>0"] = stats.get("s0>0", 0) + int(cut.sum())
    if stats is not None:
        stats["covered"] = stats.get("covered", 0) + len(e_idx)
        stats["columns"] = stats.get("columns", 0) + E * width
    return ids, depth, rgba, pack_bgra8(rgba)
