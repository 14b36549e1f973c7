"""The scaler of device pushes (include/jmhip_scale.h) restated in numpy from the
header's text; shares no code with csrc/jmh_scale.h (TEST INFRASTRUCTURE).

Two separate things:
  - tables(): the tap tables of an axis recomputed in float64,
  - scale_picture(): the two integer passes and the padding applied to tables that are handed in (the
    library's own, from jmh_scale_taps, where the result is to be compared byte for byte: a tap may
    legitimately differ by one between two float64 evaluations of a weight, see test_scale_core).
"""
import numpy as np

OFF, BILINEAR, BICUBIC, LANCZOS3 = 0, 1, 2, 3
CHROMA_LEFT = 1
TAPS_MAX, SRC_MAX, ONE = 24, 8192, 16384
SUPPORT = {BILINEAR: 1, BICUBIC: 2, LANCZOS3: 3}
NAMES = {BILINEAR: "bilinear", BICUBIC: "bicubic", LANCZOS3: "lanczos3"}


def kernel(filter, t):
    """k(t) of the three filters on a float64 array"""
    a = np.abs(np.asarray(t, np.float64))
    if filter == BILINEAR:
        return np.where(a < 1, 1 - a, 0.0)
    if filter == BICUBIC:                                      # Catmull-Rom, a = -0.5
        near = 1.5 * a ** 3 - 2.5 * a ** 2 + 1
        far = -0.5 * a ** 3 + 2.5 * a ** 2 - 4 * a + 2
        return np.where(a <= 1, near, np.where(a < 2, far, 0.0))
    return np.where(a < 3, np.sinc(a) * np.sinc(a / 3), 0.0)   # np.sinc(x) = sin(pi x) / (pi x)


def ntaps(n_src, n_dst, filter):
    """T = 2 ceil(S s), the ceiling of the exact rational"""
    S = SUPPORT[filter]
    return 2 * S if n_src <= n_dst else 2 * -((-S * n_src) // n_dst)


def tables(n_src, n_dst, filter, chroma_left=False):
    """(first[n_dst] int64, taps[n_dst, T] int64, real[n_dst, T] float64: the normalised weights times 16384)"""
    T = ntaps(n_src, n_dst, filter)
    r = n_src / n_dst
    s = max(1.0, r)
    phi = 0.25 if chroma_left else 0.5
    c = (np.arange(n_dst, dtype=np.float64) + phi) * r - phi
    first = np.floor(c - T // 2).astype(np.int64) + 1
    j = first[:, None] + np.arange(T)[None, :]
    w = kernel(filter, (j - c[:, None]) / s)
    real = w / w.sum(axis=1, keepdims=True) * ONE
    q = np.floor(real + 0.5).astype(np.int64)
    rows = np.arange(n_dst)
    q[rows, q.argmax(axis=1)] += ONE - q.sum(axis=1)           # argmax: the first of the largest
    return first, q, real


def scale_plane(src, first_h, taps_h, first_v, taps_v, bd):
    """the two passes on one plane: (the dh x dw result, the largest |h|)"""
    src = np.asarray(src).astype(np.int64)
    sh, sw = src.shape
    P = 14 - bd
    maxv = (1 << bd) - 1
    fh, th = np.asarray(first_h, np.int64), np.asarray(taps_h, np.int64)
    fv, tv = np.asarray(first_v, np.int64), np.asarray(taps_v, np.int64)
    ix = np.clip(fh[:, None] + np.arange(th.shape[1])[None, :], 0, sw - 1)          # (dw, T)
    h = ((src[:, ix] * th[None, :, :]).sum(axis=2) + (1 << (13 - P))) >> (14 - P)     # (sh, dw)
    peak = int(np.abs(h).max())
    iy = np.clip(fv[:, None] + np.arange(tv.shape[1])[None, :], 0, sh - 1)          # (dh, T)
    v = ((h[iy, :] * tv[:, :, None]).sum(axis=1) + (1 << (13 + P))) >> (14 + P)       # (dh, dw)
    return np.clip(v, 0, maxv), peak


def pad(plane, W, H):
    """the last column to the right, the last row downwards"""
    h, w = plane.shape
    return np.pad(plane, ((0, H - h), (0, W - w)), mode="edge")


def scale_picture(pics, ow, oh, W, H, filter, chroma_left, bd, taps_fn):
    """pics = (y, u, v) of the source size resampled to ow x oh and padded to W x H with the tables of
    taps_fn(n_src, n_dst, filter, chroma_left) -> (first, taps).  Returns ((y, u, v), largest |h|)."""
    dt = np.uint16 if bd > 8 else np.uint8
    out, peak = [], 0
    for pl, a in enumerate(pics):
        sh, sw = a.shape
        dw, dh = (ow // 2, oh // 2) if pl else (ow, oh)
        PW, PH = (W // 2, H // 2) if pl else (W, H)
        fh, th = taps_fn(sw, dw, filter, bool(pl) and chroma_left)
        fv, tv = taps_fn(sh, dh, filter, False)
        res, pk = scale_plane(a, fh, th, fv, tv, bd)
        peak = max(peak, pk)
        out.append(pad(res, PW, PH).astype(dt))
    return tuple(out), peak


def random_yuv(rng, w, h, bd):
    dt = np.uint16 if bd > 8 else np.uint8
    return tuple(rng.integers(0, 1 << bd, s, dtype=np.int64).astype(dt) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


# (coded W, H, source w, h, output w, h, filter, chroma_left): the cases of tests/test_scale_gpu.py, which
# tests/test_scale_core.py also runs through the C walk (jms_scale) under the sanitizers
def _cases():
    out = []
    for src, dst in (((2, 2), (64, 48)), ((256, 192), (64, 48)), ((250, 130), (62, 34))):      # every filter
        for f in (BILINEAR, BICUBIC, LANCZOS3):
            if ntaps(src[0], dst[0], f) <= TAPS_MAX:           # 250 -> 62 is above 4:1: Lanczos3 would need 26 taps (REFUSED)
                out.append((64, 48, *src, *dst, f, False))
    out.append((64, 48, 256, 192, 64, 48, LANCZOS3, True))
    out.append((64, 48, 250, 130, 62, 34, BICUBIC, True))
    out.append((64, 48, 130, 98, 48, 34, LANCZOS3, False))
    out.append((176, 144, 352, 288, 176, 144, LANCZOS3, False))
    out.append((176, 144, 120, 90, 176, 144, LANCZOS3, False))
    out.append((64, 48, 64, 48, 64, 48, LANCZOS3, False))
    return out


CASES = _cases()
# the same form: what a push answers JMH_E_UNSUPPORTED_CFG for (more than TAPS_MAX taps on an axis)
REFUSED = [(64, 48, 250, 130, 62, 34, LANCZOS3, False), (64, 48, 288, 48, 64, 48, LANCZOS3, False)]


def case_id(c):
    return f"{c[2]}x{c[3]}_to_{c[4]}x{c[5]}_in_{c[0]}x{c[1]}_{NAMES[c[6]]}" + ("_left" if c[7] else "")
