"""RGB device pictures (include/jmhip_rgb.h) restated in numpy from the formulas of the
definition: the reference of tests/test_rgb_gpu.py.  Nothing here comes from jmhip.py or the library.

Formats 16..19 (BGRA8, RGBA8, RGB10A2, BGR10A2), OR-ed with BT709 = 1 << 8 and FULL_RANGE = 1 << 9.
Q14 integer arithmetic in int32; numpy's >> of a negative int32 is an arithmetic shift (it floors)."""
import numpy as np

BGRA8, RGBA8, RGB10A2, BGR10A2 = 16, 17, 18, 19
BT709, FULL_RANGE = 1 << 8, 1 << 9
LAYOUTS = (BGRA8, RGBA8, RGB10A2, BGR10A2)
NAMES = {BGRA8: "BGRA8", RGBA8: "RGBA8", RGB10A2: "RGB10A2", BGR10A2: "BGR10A2"}

# the table of DESIGN.md §5.8, copied by hand: (matrix709, bit depth, full) -> cyr cyg cyb | cur cug cub | cvr cvg cvb
TABLE = {
    (0, 8, 0): [4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170],
    (0, 10, 0): [4195, 8236, 1599, -2421, -4754, 7175, 7175, -6008, -1167],
    (0, 8, 1): [4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332],
    (0, 10, 1): [4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332],
    (1, 8, 0): [2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660],
    (1, 10, 0): [2983, 10034, 1013, -1644, -5531, 7175, 7175, -6517, -658],
    (1, 8, 1): [3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751],
    (1, 10, 1): [3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751],
}


def depth_of(format):
    return 10 if (format & 0xff) >= RGB10A2 else 8


def gains(format, bd):
    """the real-valued gains kyr kyg kyb | kur kug kub | kvr kvg kvb and (Yo, Co, M)"""
    kr, kb = (0.2126, 0.0722) if format & BT709 else (0.299, 0.114)
    m = (1 << bd) - 1
    if format & FULL_RANGE:
        ys, cs, yo = float(m), float(m), 0
    else:
        ys, cs, yo = 219.0 * 2 ** (bd - 8), 224.0 * 2 ** (bd - 8), 16 << (bd - 8)
    kg = 1.0 - kr - kb
    y = [kr * ys / m, kg * ys / m, kb * ys / m]
    u = [-kr / (2 * (1 - kb)) * cs / m, -kg / (2 * (1 - kb)) * cs / m, 0.5 * cs / m]
    v = [0.5 * cs / m, -kg / (2 * (1 - kr)) * cs / m, -kb / (2 * (1 - kr)) * cs / m]
    return y + u + v, (yo, 1 << (bd - 1), m)


def coefficients(format, bd):
    """the 12 ints of the definition: c = rint(k 2^14), the green terms closing the sums; Yo, Co, M"""
    k, (yo, co, m) = gains(format, bd)
    ys = m if format & FULL_RANGE else 219 * 2 ** (bd - 8)
    q = lambda x: int(np.rint(np.float64(x) * 16384.0))
    cyr, cyb, cur, cub, cvr, cvb = q(k[0]), q(k[2]), q(k[3]), q(k[5]), q(k[6]), q(k[8])
    cyg = q(ys / m) - cyr - cyb
    return [cyr, cyg, cyb, cur, -cur - cub, cub, cvr, -cvr - cvb, cvb, yo, co, m]


def unpack(words, format):
    """(h, w) uint32 little-endian words -> R, G, B as int32"""
    layout = format & 0xff
    words = words.astype(np.uint32)
    sh, m = (10, 1023) if layout >= RGB10A2 else (8, 255)
    lo, g, hi = (words & m).astype(np.int32), (words >> sh & m).astype(np.int32), (words >> 2 * sh & m).astype(np.int32)
    return (lo, g, hi) if layout in (RGBA8, RGB10A2) else (hi, g, lo)


def convert(words, format, bd):
    """(y, u, v) at the source size, in the sample type of a bd-bit context"""
    c = coefficients(format, bd)
    yo, co, m = c[9:]
    r, g, b = unpack(words, format)
    y = np.minimum(m, yo + ((c[0] * r + c[1] * g + c[2] * b + (1 << 13)) >> 14))
    box = lambda a: a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
    rs, gs, bs = box(r), box(g), box(b)
    u = np.clip(co + ((c[3] * rs + c[4] * gs + c[5] * bs + (1 << 15)) >> 16), 0, m)
    v = np.clip(co + ((c[6] * rs + c[7] * gs + c[8] * bs + (1 << 15)) >> 16), 0, m)
    dt = np.uint16 if bd > 8 else np.uint8
    return tuple(np.ascontiguousarray(a.astype(dt)) for a in (y, u, v))


def pad(pics, cw, ch):
    """jm_pad_picture: the last column to the right, the last row downwards, chroma at half size"""
    out = []
    for a, (H, W) in zip(pics, ((ch, cw), (ch // 2, cw // 2), (ch // 2, cw // 2))):
        out.append(np.ascontiguousarray(np.pad(a, ((0, H - a.shape[0]), (0, W - a.shape[1])), mode="edge")))
    return tuple(out)


def to_yuv(words, format, bd, cw, ch):
    return pad(convert(words, format, bd), cw, ch)


def corners(format):
    """the eight RGB corners as words of the layout (alpha set), forwards and backwards"""
    layout = format & 0xff
    top, sh, a = (1023, 10, 3 << 30) if layout >= RGB10A2 else (255, 8, 0xff << 24)
    out = []
    for i in range(8):
        c = [top if i >> k & 1 else 0 for k in range(3)]
        out.append(c[0] | c[1] << sh | c[2] << 2 * sh | a)
    return np.array([out, out[::-1]], np.uint32)


def random_words(rng, w, h, format):
    """uniform words (alpha noise included) with the eight corners as 2 x 2 blocks: along the first row
    pair where 16 pixels fit, else down the first column pair where 16 rows fit, else the one block of
    the pure high component (blue of RGBA8 / RGB10A2, red of the BGR layouts): full range clamps it"""
    a = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    c = corners(format)[0]
    if w >= 16:
        a[0:2, 0:16] = np.repeat(c, 2)[None, :]
    elif h >= 16:
        a[0:16, 0:2] = np.repeat(c, 2)[:, None]
    else:
        a[0:2, 0:2] = c[4]
    return a
