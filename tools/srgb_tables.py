"""Prints nenbody_amd/csrc/nb_srgb_tables.h: the two sRGB tables of the eye view's colour row (DESIGN.md section 10, step 11 on).

    D[b] = binary32(decode(b / 255))            an 8-bit sRGB skin byte -> the linear texel
    T[b] = binary32(decode((b - 0.5) / 255))    the least linear value that encodes to byte b (b = 1 .. 255; T[0] = 0, unused)

decode is the sRGB EOTF, e / 12.92 for e <= 0.04045, else ((e + 0.055) / 1.055) ^ 2.4, evaluated with `decimal` to 60 digits and
rounded to the nearest binary32 by exact comparison of fractions.  tests/test_eyes_colour_cpu.py recomputes both on its own.

    python tools/srgb_tables.py > nenbody_amd/csrc/nb_srgb_tables.h
"""
import decimal
import re
import struct
from fractions import Fraction

decimal.getcontext().prec = 60
Dec = decimal.Decimal


def decode(e: Fraction) -> Fraction:
    if e <= Fraction(4045, 100000):
        return e / Fraction(1292, 100)
    x = Dec(e.numerator) / Dec(e.denominator)
    y = (((x + Dec("0.055")) / Dec("1.055")).ln() * Dec("2.4")).exp()
    return Fraction(y)


def f32_bits(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


def bits_f32(b: int) -> float:
    return struct.unpack("<f", struct.pack("<I", b))[0]


def nearest_binary32(v: Fraction) -> float:
    """the binary32 nearest to v >= 0 (positive floats order as their bit patterns)"""
    b = f32_bits(float(v))
    return min((bits_f32(c) for c in (b - 1, b, b + 1) if c >= 0), key=lambda f: abs(Fraction(f) - v))


def tables():
    d = [nearest_binary32(decode(Fraction(b, 255))) for b in range(256)]
    t = [0.0] + [nearest_binary32(decode(Fraction(2 * b - 1, 510))) for b in range(1, 256)]
    return d, t


def rows(vals):
    out = []
    for i in range(0, 256, 8):
        out.append("    " + " ".join(re.sub(r"\.?0*p", "p", float(v).hex()) + "f," for v in vals[i:i + 8]))
    return "\n".join(out)


if __name__ == "__main__":
    d, t = tables()
    print(f"""// nb_srgb_tables.h -- the sRGB tables of the eye view's colour row (DESIGN.md section 10), written by tools/srgb_tables.py from
// 60-digit decimal arithmetic: constants, not a pow() at load time.  decode = the sRGB EOTF (e / 12.92 for e <= 0.04045, else
// ((e + 0.055) / 1.055) ^ 2.4).  The includer defines NB_SRGB_TABLE to the storage it wants (`static const`, or
// `static __device__ const` for the kernel's copy of T).
#pragma once

#ifdef NB_SRGB_WANT_DECODE
// D[b] = binary32(decode(b / 255)): an 8-bit sRGB byte as the linear value a Rgba8UnormSrgb texture hands the shader
NB_SRGB_TABLE float kSrgbDecode[256] = {{
{rows(d)}
}};
#endif

// T[b] = binary32(decode((b - 0.5) / 255)), b = 1 .. 255: the byte of a linear value c is the number of T[1..255] that are <= c
// (strictly increasing; a NaN gives 0).  T[0] = 0 is never compared.
NB_SRGB_TABLE float kSrgbEncodeT[256] = {{
{rows(t)}
}};""")
