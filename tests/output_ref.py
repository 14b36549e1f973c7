"""Decoded pictures pulled on the device (include/jmhip_output.h) restated in numpy
from the formulas of the definition: the reference of tests/test_output_gpu.py and
tests/test_output_core.py.  Nothing here comes from jmhip.py, the library or csrc/jmh_output.h.

Coefficients: the exact rationals times 2^14 by fractions.Fraction, rounded half away from zero.
Conversion in int64, chroma by replication (every pixel of a 2x2 block takes the block's U and V):
  R = clamp((iy d + irv f + 2^13) >> 14), G = clamp((iy d + igu e + igv f + 2^13) >> 14),
  B = clamp((iy d + ibu e + 2^13) >> 14) with d = Y - Yo, e = U - Co, f = V - Co.
Dequantisation: q for U8 / U16; float32(q) / float32(M) in numpy float32 (IEEE division), then
astype(float16), or round-to-nearest-even on the float32 bits for bfloat16."""
from fractions import Fraction

import numpy as np

I420, NV12, I010, P010 = 0, 1, 2, 3
BGRA8, RGBA8, RGB10A2, BGR10A2 = 16, 17, 18, 19
BT709, FULL_RANGE = 1 << 8, 1 << 9
FLAGS = (0, BT709, FULL_RANGE, BT709 | FULL_RANGE)
YUV_FORMATS = {8: (I420, NV12), 9: (I010,), 10: (I010, P010)}
RGB_FORMATS = {8: (BGRA8, RGBA8), 10: (RGB10A2, BGR10A2)}
NAMES = {I420: "I420", NV12: "NV12", I010: "I010", P010: "P010", BGRA8: "BGRA8", RGBA8: "RGBA8", RGB10A2: "RGB10A2", BGR10A2: "BGR10A2"}
U8, U16, F16, BF16, F32 = 0, 1, 2, 3, 4

# the table of the definition, copied by hand: (matrix709, bit depth, full) -> iy irv igu igv ibu
TABLE = {
    (0, 8, 0): [19077, 26149, -6419, -13320, 33050],
    (0, 10, 0): [19133, 26226, -6438, -13359, 33148],
    (0, 8, 1): [16384, 22970, -5638, -11700, 29032],
    (0, 10, 1): [16384, 22970, -5638, -11700, 29032],
    (1, 8, 0): [19077, 29372, -3494, -8731, 34610],
    (1, 10, 0): [19133, 29459, -3504, -8757, 34711],
    (1, 8, 1): [16384, 25802, -3069, -7670, 30402],
    (1, 10, 1): [16384, 25802, -3069, -7670, 30402],
}


def _rint(fr):
    """a Fraction rounded half away from zero"""
    n = int((abs(fr) * 2 + 1) // 2)
    return n if fr >= 0 else -n


def coefficients(flags, bd):
    """iy, irv, igu, igv, ibu, Yo, Co, M from the exact rationals"""
    kr, kb = (Fraction(2126, 10000), Fraction(722, 10000)) if flags & BT709 else (Fraction(299, 1000), Fraction(114, 1000))
    kg = 1 - kr - kb
    m = (1 << bd) - 1
    ys, cs, yo = (m, m, 0) if flags & FULL_RANGE else (219 << (bd - 8), 224 << (bd - 8), 16 << (bd - 8))
    q = 1 << 14
    return [_rint(Fraction(m, ys) * q), _rint(2 * (1 - kr) * Fraction(m, cs) * q), _rint(-2 * kb * (1 - kb) / kg * Fraction(m, cs) * q),
            _rint(-2 * kr * (1 - kr) / kg * Fraction(m, cs) * q), _rint(2 * (1 - kb) * Fraction(m, cs) * q), yo, 1 << (bd - 1), m]


def to_rgb(y, u, v, flags, bd, counts=None):
    """R, G, B (int64, the size of y) of planes y (h x w) and u, v (h/2 x w/2); counts, a dict, is given
    the number of samples the clamp caught at 0 ("lo") and at M ("hi") per component"""
    iy, irv, igu, igv, ibu, yo, co, m = coefficients(flags, bd)
    up = lambda a: np.repeat(np.repeat(np.asarray(a, np.int64), 2, axis=0), 2, axis=1)
    d, e, f = np.asarray(y, np.int64) - yo, up(u) - co, up(v) - co
    raw = [(iy * d + irv * f + (1 << 13)) >> 14, (iy * d + igu * e + igv * f + (1 << 13)) >> 14, (iy * d + ibu * e + (1 << 13)) >> 14]
    if counts is not None:
        counts["lo"] = [int((a < 0).sum()) for a in raw]
        counts["hi"] = [int((a > m).sum()) for a in raw]
    return [np.clip(a, 0, m) for a in raw]


def crop(pics, w, h):
    y, u, v = pics
    return y[:h, :w], u[:h // 2, :w // 2], v[:h // 2, :w // 2]


def bf16_bits(x32):
    """float32 values to bfloat16 bits, round to nearest even (finite values)"""
    b = np.asarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + (b >> 16 & 1)) >> 16).astype(np.uint16)


def dequantise(q, dtype, bd):
    """the elements that hold q: uint8, uint16, float16, bfloat16 bits as uint16, float32"""
    q = np.asarray(q)
    if dtype == U8:
        return q.astype(np.uint8)
    if dtype == U16:
        return q.astype(np.uint16)
    x = q.astype(np.float32) / np.float32((1 << bd) - 1)
    assert x.dtype == np.float32
    return x.astype(np.float16) if dtype == F16 else bf16_bits(x) if dtype == BF16 else x


def tensor(pics, w, h, dtype, flags, bd, counts=None):
    """R, G, B element arrays (h x w) of the w x h crop of the coded-size planes pics"""
    return [dequantise(a, dtype, bd) for a in to_rgb(*crop(pics, w, h), flags, bd, counts)]


def picture(pics, w, h, format, bd, counts=None):
    """the planes of the w x h crop in a picture format: [y, u, v], [y, uv] of NV12 / P010 (uint8 or
    uint16), or [(h, w) uint32 words] of an RGB format"""
    lay = format & 0xff
    y, u, v = crop(pics, w, h)
    if lay >= BGRA8:
        r, g, b = (a.astype(np.uint32) for a in to_rgb(y, u, v, format & (BT709 | FULL_RANGE), bd, counts))
        sh, alpha = (10, 3 << 30) if lay >= RGB10A2 else (8, 0xff << 24)
        lo, hi = (r, b) if lay in (RGBA8, RGB10A2) else (b, r)
        return [(lo | g << sh | hi << 2 * sh | np.uint32(alpha)).astype(np.uint32)]
    dt = np.uint16 if lay >= I010 else np.uint8
    y, u, v = (np.asarray(a).astype(dt) << (6 if lay == P010 else 0) for a in (y, u, v))
    if lay in (NV12, P010):
        uv = np.empty((h // 2, w), dt)
        uv[:, 0::2], uv[:, 1::2] = u, v
        return [y.astype(dt), uv]
    return [y.astype(dt), u.astype(dt), v.astype(dt)]


def clamps_everywhere(counts):
    """the condition on the RGB cases: a sample clamped at 0 and one clamped at M in each of R, G, B"""
    return all(n > 0 for n in counts["lo"] + counts["hi"])


def random_yuv(rng, cw, ch, bd):
    """uniform planes over the whole code range [0, M], of the coded size, with three planted 2x2 blocks
    of luma M M / 0 0: the top-left one under U = V = 0 (R and B leave the range below, G above), its
    right and lower neighbours under U = V = M (R and B above, G below), with both matrices and both
    ranges: every crop of two blocks or more clamps every component on both sides"""
    m, dt = (1 << bd) - 1, np.uint16 if bd > 8 else np.uint8
    y, u, v = (rng.integers(0, m + 1, s).astype(dt) for s in ((ch, cw), (ch // 2, cw // 2), (ch // 2, cw // 2)))
    y[0:4:2, 0:4], y[1:4:2, 0:4] = m, 0
    u[0:2, 0:2] = v[0:2, 0:2] = m
    u[0, 0] = v[0, 0] = 0
    return y, u, v
