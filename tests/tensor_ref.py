"""RGB device tensors (include/jmhip_tensor.h) restated in numpy from the definition:
the reference of tests/test_tensor_gpu.py.  Nothing here comes from jmhip.py or the library.

An element becomes an integer component q in [0, M], M = 2^bd - 1: the byte of U8, min(v, M) of U16,
floor(x M + 1/2) of a float after x is clamped to [0, 1] (NaN and everything <= 0 give 0, everything
>= 1 gives M; F16 and BF16 widened exactly first).  quantise() evaluates that in numpy float64, which
is exact for every float32 (the argument is in csrc/jmh_tensor.h); quantise_exact() does it in integer
arithmetic on the decoded mantissa and exponent, and the tests hold the one against the other.

The conversion is not restated: convert() packs the quantised components into RGBA8 / RGB10A2 words and
hands them to rgb_ref.to_yuv, so a tensor answers to the reference the RGB pictures answer to."""
import numpy as np

import rgb_ref

U8, U16, F16, BF16, F32 = 0, 1, 2, 3, 4
DTYPES = (U8, U16, F16, BF16, F32)
NAMES = {U8: "U8", U16: "U16", F16: "F16", BF16: "BF16", F32: "F32"}
ES = {U8: 1, U16: 2, F16: 2, BF16: 2, F32: 4}
FLOATS = (F16, BF16, F32)
BT709, FULL_RANGE = rgb_ref.BT709, rgb_ref.FULL_RANGE
FLAGS = (0, BT709, FULL_RANGE, BT709 | FULL_RANGE)
# every valid (dtype, context bit depth) pair
PAIRS = ((U8, 8), (F16, 8), (BF16, 8), (F32, 8), (U16, 10), (F16, 10), (BF16, 10), (F32, 10))


def storage(dtype):
    """the numpy type an array of this dtype travels as (bfloat16: its uint16 bits)"""
    return {U8: np.uint8, U16: np.uint16, F16: np.float16, BF16: np.uint16, F32: np.float32}[dtype]


def as_float32(a, dtype):
    """the elements of a float dtype (values, or their bits as uint16 / uint32) widened exactly to float32"""
    a = np.asarray(a)
    if dtype == F16:
        return (a.view(np.float16) if a.dtype == np.uint16 else a).astype(np.float32)
    if dtype == BF16:
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.view(np.float32) if a.dtype == np.uint32 else a.astype(np.float32)


def quantise(a, dtype, bd):
    """q of every element, int32: numpy float64 floor(x * M + 0.5) after the clamp"""
    m = (1 << bd) - 1
    a = np.asarray(a)
    if dtype == U8:
        return a.astype(np.int32)
    if dtype == U16:
        return np.minimum(a.astype(np.int32), m)
    with np.errstate(invalid="ignore"):
        x = as_float32(a, dtype).astype(np.float64)
        inside = (x > 0.0) & (x < 1.0)                          # NaN compares false
        q = np.floor(np.where(inside, x, 0.0) * m + 0.5)
        q = np.where(x >= 1.0, float(m), q)
    return q.astype(np.int32)


def quantise_exact(bits32, bd):
    """the same from the bits of float32 values, in Python integers: x = mant * 2^exp exactly, and
    floor(x M + 1/2) = (2 mant M + 2^s) >> (s + 1) with s = -exp"""
    m = (1 << bd) - 1
    out = []
    for b in np.asarray(bits32, np.uint32).tolist():
        e, mant, neg = b >> 23 & 0xff, b & 0x7fffff, b >> 31
        if e == 0xff:
            out.append(0 if mant or neg else m)                 # NaN, -inf: 0; +inf: M
            continue
        if neg or (e == 0 and mant == 0):
            out.append(0)                                       # negatives, -0, +0
            continue
        mant, exp = (mant, -149) if e == 0 else (mant | 1 << 23, e - 150)
        if exp >= 0 or mant >> -exp >= 1:                       # x >= 1
            out.append(m)
            continue
        s = -exp
        out.append((2 * mant * m + (1 << s)) >> (s + 1))
    return np.array(out, np.int32)


def bits32(a, dtype):
    """the float32 bit patterns of the elements of a float dtype"""
    return as_float32(a, dtype).view(np.uint32)


def convert(chans, dtype, flags, bd, cw, ch):
    """(y, u, v) of the coded size from the R, G, B element arrays (h, w) of a tensor"""
    r, g, b = (quantise(c, dtype, bd).astype(np.uint32) for c in chans)
    sh, layout = (10, rgb_ref.RGB10A2) if bd == 10 else (8, rgb_ref.RGBA8)
    words = r | g << sh | b << 2 * sh
    return rgb_ref.to_yuv(words, layout | flags, bd, cw, ch)


def convert_source_size(chans, dtype, flags, bd):
    """the same at the source size (what a .yuv file of the picture holds)"""
    r, g, b = (quantise(c, dtype, bd).astype(np.uint32) for c in chans)
    sh, layout = (10, rgb_ref.RGB10A2) if bd == 10 else (8, rgb_ref.RGBA8)
    return rgb_ref.convert(r | g << sh | b << 2 * sh, layout | flags, bd)


def grey_luma(q, flags, bd):
    """Y of the grey pixels R = G = B = q; asserts that the map is injective over [0, M], so that a
    wrong q cannot hide behind a right Y (true at full range, where Y = q; not at limited range)"""
    c = rgb_ref.coefficients(rgb_ref.RGBA8 | flags if bd == 8 else rgb_ref.RGB10A2 | flags, bd)
    yo, m = c[9], c[11]
    luma = lambda v: np.minimum(m, yo + (((c[0] + c[1] + c[2]) * v + (1 << 13)) >> 14))
    every = luma(np.arange(m + 1, dtype=np.int64))
    assert len(set(every.tolist())) == m + 1 and (np.diff(every) > 0).all(), "grey luma is not injective with these flags"
    return luma(np.asarray(q, np.int64))


# ---- test content ----
def float_specials(dtype):
    """elements every float test picture holds: a NaN, a negative value, a value above 1, the exact tie
    1/2 (x M = k + 1/2 with k = (M - 1) / 2: the only tie in (0, 1), M being odd), then -0, +inf, -inf"""
    vals = np.array([np.nan, -0.25, 1.5, 0.5, -0.0, np.inf, -np.inf], np.float32)
    return from_float32(vals, dtype)


def from_float32(x, dtype):
    """float32 values as elements of a float dtype (BF16 by truncation: any bits will do for content)"""
    x = np.asarray(x, np.float32)
    if dtype == F16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16)
    if dtype == BF16:
        return (x.view(np.uint32) >> 16).astype(np.uint16)
    return x


def holds_condition(chans, dtype):
    """the condition on every float test picture: a NaN, a negative value, a value > 1 and the tie 1/2"""
    x = np.concatenate([as_float32(c, dtype).ravel() for c in chans])
    return bool(np.isnan(x).any() and (x < 0).any() and (x > 1).any() and (x == 0.5).any())


def random_chans(rng, w, h, dtype):
    """R, G, B element arrays (h, w): uniform content that leaves the nominal range on both sides; the
    float dtypes get the first four specials planted in the first row pair (and the rest where there
    is room), so that holds_condition is true for every size from 2x2 up"""
    if dtype == U8:
        return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3)]
    if dtype == U16:
        a = [rng.integers(0, 1024, (h, w)).astype(np.uint16) for _ in range(3)]
        a[0][0, 0], a[1][-1, -1], a[2][0, -1] = 1024, 65535, 1023          # min(v, M) is live
        return a
    chans = [from_float32(rng.uniform(-0.125, 1.125, (h, w)).astype(np.float32), dtype) for _ in range(3)]
    sp = float_specials(dtype)
    flat = [(c, y, x) for y in range(2) for x in range(2) for c in range(3)]   # 12 places in the first 2x2 block
    for (c, y, x), v in zip(flat, sp):
        chans[c][y, x] = v
    assert holds_condition(chans, dtype)
    return chans


def f32_edge_bits(bd):
    """the float32 edge set of a bit depth, as bit patterns: for every k in [0, M] the floats nearest
    k / M and (k + 1/2) / M with two neighbours on each side; +-0, denormals, +-inf, NaNs, the values
    just outside [0, 1]"""
    m = (1 << bd) - 1
    k = np.arange(m + 1, dtype=np.float64)
    centres = np.concatenate([k / m, (k + 0.5) / m]).astype(np.float32).view(np.uint32).astype(np.int64)
    near = np.concatenate([centres + d for d in (-2, -1, 0, 1, 2)])
    near = near[(near >= 0) & (near < 0x7f800000)]
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x007fffff, 0x00800000, 0x80000001, 0x807fffff,   # +-0, denormals
                        0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x7fffffff,   # inf, NaNs
                        0x3f800000, 0x3f800001, 0x3f7fffff, 0x3f7ffffe, 0xbf800000, 0x3f000000, 0x3effffff, 0x3f000001,
                        0x40000000, 0x7f7fffff, 0xff7fffff, 0x33800000, 0x34000000], np.int64)
    return np.concatenate([near, special]).astype(np.uint32)
