"""Directed pictures: content that makes every intra prediction mode win, and a census that proves it.

A whole-picture comparison sees only the winning decision of every block; the prediction of a
mode that never wins is computed and never reaches an assertion.  The families here are built so
that the oracle chooses every Intra4x4 / Intra8x8 / Intra16x16 / chroma mode, with and without
its neighbours, in I and in P pictures; census() counts what was chosen from the macroblock
results alone, and table_misses() holds the counts against the table of DESIGN.md §6.1.

Everything is 64x48 (4 x 3 macroblocks: corners, edges and two interior macroblocks) and comes
from seeds.  CPU only: nothing here imports the device library.  Run as a script to print the
census of the oracle for every configuration of CONFIGS.
"""
from collections import Counter

import numpy as np

W, H = 64, 48
P_SLICE, I_SLICE = 0, 2
I4MB, I16MB, I8MB = 9, 10, 13

# f(a x + b y) is constant along (b, -a): the direction each Intra4x4 / Intra8x8 mode predicts along.
# (a, b) -> the mode (H.264 tables 8-2 / 8-3) whose direction that is
DIRECTIONS = [((1, 0), 0), ((0, 1), 1), ((1, 1), 3), ((1, -1), 4), ((2, -1), 5), ((1, -2), 6), ((2, 1), 7), ((1, 2), 8)]


# ---------------------------------------------------------------- generators
def _walk(rng, n, sigma, lo=16.0, hi=240.0):
    """A random walk of n steps of the given sigma, folded into [lo, hi] (a fold keeps it continuous)."""
    v = 128.0 + np.cumsum(rng.normal(0.0, sigma, n))
    span = hi - lo
    v = np.mod(v - lo, 2 * span)
    return lo + np.where(v > span, 2 * span - v, v)


def _oriented_plane(rng, w, h, ab, scale, sigma, noise, step=1):
    """f((a x + b y) / scale) on a w x h plane whose samples sit step luma samples apart: f a random
    walk interpolated linearly, plus uniform noise of +-noise."""
    a, b = ab
    y, x = np.mgrid[0:h, 0:w] * step
    t = (a * x + b * y).astype(np.float64)
    t = (t - t.min()) / scale
    f = _walk(rng, int(t.max()) + 2, sigma)
    i = t.astype(np.int64)
    v = f[i] + (t - i) * (f[i + 1] - f[i])
    if noise:
        v = v + rng.integers(-noise, noise + 1, (h, w))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def oriented(seed, ab, scale=1, sigma=14.0, noise=0, w=W, h=H):
    """One picture varying along (a, b) only; chroma carries the same orientation with walks of its own."""
    rng = np.random.default_rng(seed)
    y = _oriented_plane(rng, w, h, ab, scale, sigma, noise)
    u = _oriented_plane(rng, w // 2, h // 2, ab, scale, sigma / 2, noise // 2, step=2)
    v = _oriented_plane(rng, w // 2, h // 2, ab, scale, sigma / 2, noise // 2, step=2)
    return y, u, v


def flat_noise(seed, amp, spread, base=None, camp=2, w=W, h=H):
    """Flat macroblocks of mean base +-spread (base None: one random base per plane) with +-amp
    noise; chroma flat per macroblock with +-camp."""
    rng = np.random.default_rng(seed)
    mbh, mbw = h // 16, w // 16

    def plane(sub, a):
        b = rng.integers(60, 196) if base is None else base
        mean = b + rng.integers(-spread, spread + 1, (mbh, mbw))
        p = np.kron(mean, np.ones((sub, sub), np.int64)) + rng.integers(-a, a + 1, (mbh * sub, mbw * sub))
        return np.clip(p, 0, 255).astype(np.uint8)
    return plane(16, amp), plane(8, camp), plane(8, camp)


def global_plane(seed, w=W, h=H):
    """128 + 3 (x - w/2) + 2 (y - h/2) +- 1: Intra16x16 plane prediction; chroma planes likewise."""
    rng = np.random.default_rng(seed)

    def plane(w, h, gx, gy):
        y, x = np.mgrid[0:h, 0:w]
        return np.clip(128 + gx * (x - w // 2) + gy * (y - h // 2) + rng.integers(-1, 2, (h, w)), 0, 255).astype(np.uint8)
    return plane(w, h, 3, 2), plane(w // 2, h // 2, -4, 3), plane(w // 2, h // 2, 2, -5)


def bands(seed, vertical, w=W, h=H):
    """Macroblock-wide smooth ramps across (vertical) or down the picture, flat along the other axis,
    +-1 noise: Intra16x16 vertical / horizontal prediction."""
    rng = np.random.default_rng(seed)

    def plane(w, h, sigma):
        n = w if vertical else h
        f = _walk(rng, n, sigma)
        p = np.tile(f, (h, 1)) if vertical else np.tile(f[:, None], (1, w))
        return np.clip(np.rint(p + rng.integers(-1, 2, (h, w))), 0, 255).astype(np.uint8)
    return plane(w, h, 5.0), plane(w // 2, h // 2, 4.0), plane(w // 2, h // 2, 4.0)


def checker(ref, other, phase):
    """The P family's current picture: macroblocks with (mbx + mby + phase) even copy ref (inter wins),
    the others carry other (unrelated content: intra wins) -- intra macroblocks with inter neighbours."""
    out = []
    for r, o in zip(ref, other):
        sub = r.shape[1] // (W // 16)
        p = o.copy()
        for my in range(H // 16):
            for mx in range(W // 16):
                if (mx + my + phase) % 2 == 0:
                    p[my * sub:(my + 1) * sub, mx * sub:(mx + 1) * sub] = r[my * sub:(my + 1) * sub, mx * sub:(mx + 1) * sub]
        out.append(p)
    return tuple(out)


def widen(pic, seed):
    """The 10-bit variant: 4 y + (random 0..3)."""
    rng = np.random.default_rng(seed)
    return tuple((p.astype(np.uint16) * 4 + rng.integers(0, 4, p.shape).astype(np.uint16)) for p in pic)


class PictureSet:
    """Pictures coded alike: slice type, QP, and for P pictures the reference of each."""

    def __init__(self, name, slice_type, qp, pics, refs=None, direction=None):
        self.name, self.slice_type, self.qp, self.pics, self.refs, self.direction = name, slice_type, qp, pics, refs, direction


def intra_sets():
    """The I-picture families, 8 bits."""
    sets = []
    for k, (ab, mode) in enumerate(DIRECTIONS):
        # sharp: one walk step per sample -- Intra4x4
        sets.append(PictureSet(f"sharp{mode}", I_SLICE, 12, [oriented(100 + k, ab, 1, 14.0)]))
        sets.append(PictureSet(f"sharp{mode}q", I_SLICE, 28, [oriented(120 + k, ab, 1, 14.0)]))
        # smooth: the walk interpolated at scale 2 and 4 -- Intra8x8
        sets.append(PictureSet(f"smooth{mode}", I_SLICE, 32, [oriented(200 + k, ab, 2, 14.0), oriented(220 + k, ab, 4, 14.0)],
                               direction=mode))
    sets.append(PictureSet("smooth6n", I_SLICE, 32, [oriented(300, (1, -2), 2, 14.0, 3), oriented(301, (1, -2), 4, 14.0, 3)]))
    # Intra16x16: heavy noise on one mean (RDO off: DC prediction, all 16 AC blocks, DC levels >= 128),
    # exact flats of distant means (RDO on: the DC level alone), fine noise that survives QP 20 (DC
    # prediction from one neighbour) and that QP 28 removes (ties: vertical / horizontal, cbp 0)
    sets.append(PictureSet("heavy", I_SLICE, 0, [flat_noise(400, 90, 0, 128), flat_noise(401, 90, 0, 128)]))
    sets.append(PictureSet("exact", I_SLICE, 0, [flat_noise(410, 0, 60, 128, 0)]))
    sets.append(PictureSet("fine", I_SLICE, 20, [flat_noise(420, 6, 0, 128), flat_noise(421, 6, 0, 128)]))
    sets.append(PictureSet("fineq", I_SLICE, 28, [flat_noise(430, 3, 1, 128)]))
    sets.append(PictureSet("plane", I_SLICE, 28, [global_plane(500)]))
    sets.append(PictureSet("bands", I_SLICE, 36, [bands(600, True), bands(601, False)]))
    return sets


def p_sets():
    """The P family: the current picture copies its reference in a checkerboard of macroblocks (inter
    wins there) and carries unrelated content in the others (intra wins, between inter neighbours).
    The reference is one oriented picture; for the Intra16x16 set it is fine noise on the same mean as
    the intra macroblocks' own, so that their DC prediction from the inter neighbours fits."""
    sets = []
    others = [(lambda s: oriented(s, (1, -1), 1, 14.0), None, 20),                        # Intra4x4
              (lambda s: oriented(s, (1, 2), 4, 14.0), None, 32),                         # Intra8x8
              (lambda s: flat_noise(s, 3, 1, 128), lambda s: flat_noise(s, 3, 1, 128), 28),  # Intra16x16
              (lambda s: oriented(s, (1, -1), 4, 14.0), None, 32)]                        # Intra8x8, down-right
    for k, (gen, refgen, qp) in enumerate(others):
        pics, refs = [], []
        for phase in (0, 1):
            seed = 700 + 2 * k + phase
            ref = refgen(seed) if refgen else oriented(seed, DIRECTIONS[(3 * k + phase) % 8][0], 4, 6.0)
            refs.append(ref)
            pics.append(checker(ref, gen(seed + 20), phase))
        sets.append(PictureSet(f"checker{k}", P_SLICE, qp, pics, refs))
    return sets


def for_depth(sets, bit_depth):
    if bit_depth == 8:
        return sets
    out = []
    for k, s in enumerate(sets):
        pics = [widen(p, 1000 + 10 * k + i) for i, p in enumerate(s.pics)]
        refs = [widen(p, 2000 + 10 * k + i) for i, p in enumerate(s.refs)] if s.refs else None
        out.append(PictureSet(s.name, s.slice_type, s.qp, pics, refs, s.direction))
    return out


# ---------------------------------------------------------------- census
# decoding order of the 4x4 blocks of a macroblock (6.4.3), by raster position
_ORDER4 = {(2 * (k % 2) + j % 2, 2 * (k // 2) + j // 2): 4 * k + j for k in range(4) for j in range(4)}


def _which(left, top):
    return "both" if left and top else "left" if left else "top" if top else "none"


def census(results, slice_type, w, slice_mbs):
    """Count what one picture's macroblock results chose.  Neighbour availability is derived here from
    the macroblock's position, the block's index and slice_mbs (raster runs of slice_mbs macroblocks;
    6.4.8 - 6.4.11), never taken from the encoder.  Cells (a Counter):

        ("i4", m) / ("i8", m)       4x4 / 8x8 blocks of Intra4x4 / Intra8x8 macroblocks predicted by mode m
        ("i16", m) / ("chroma", m)  Intra16x16 macroblocks / intra macroblocks by mode m
        ("i16cbp", c)               Intra16x16 macroblocks by luma cbp (0 or 15)
        ("i16dc128",)               Intra16x16 macroblocks with a |luma_dc| level >= 128
        ("i4ur", m, 0 / 1), ("i8ur", m, 0 / 1)    blocks of mode m with the above-right block un/available
        (kind + "dc", "left" / "top" / "none" / "both")   DC predictions by the neighbours they had
        ("sliceedge", what)         "unavailable" cases whose missing neighbour is inside the picture
    In a P picture the mode cells carry a leading "p", and there are
        ("pmb", mb_type)            intra macroblocks by type
        ("pintra_inter_la",)        intra macroblocks whose left and above neighbours (same slice) are inter
    """
    c = Counter()
    mbw = w // 16
    p = "p" if slice_type == P_SLICE else ""
    for a in range(len(results)):
        r = results[a]
        t = int(r["mb_type"])
        if t not in (I4MB, I16MB, I8MB):
            continue
        mx, my = a % mbw, a // mbw
        first = (a // slice_mbs) * slice_mbs if slice_mbs > 0 else 0
        A = mx > 0 and a - 1 >= first
        B = my > 0 and a - mbw >= first
        C = my > 0 and mx < mbw - 1 and a - mbw + 1 >= first
        B_edge = my > 0 and not B                       # the missing neighbour lies in another slice
        C_edge = my > 0 and mx < mbw - 1 and not C
        ipred = r["ipred"]
        if slice_type == P_SLICE:
            c[("pmb", t)] += 1
            inter = lambda b: int(results[b]["mb_type"]) not in (I4MB, I16MB, I8MB)
            if A and B and inter(a - 1) and inter(a - mbw):
                c[("pintra_inter_la",)] += 1
        cm = int(r["c_ipred_mode"])
        c[(p + "chroma", cm)] += 1
        if cm == 0:
            c[(p + "chromadc", _which(A, B))] += 1
            if B_edge:
                c[(p + "sliceedge", "chromadc")] += 1
        if t == I16MB:
            m = int(r["i16mode"])
            c[(p + "i16", m)] += 1
            c[(p + "i16cbp", int(r["cbp"]) & 15)] += 1
            if np.abs(r["luma_dc"].astype(np.int32)).max() >= 128:
                c[(p + "i16dc128",)] += 1
            if m == 2:
                c[(p + "i16dc", _which(A, B))] += 1
                if B_edge:
                    c[(p + "sliceedge", "i16dc")] += 1
        elif t == I4MB:
            for by in range(4):
                for bx in range(4):
                    m = int(ipred[4 * by + bx])
                    c[(p + "i4", m)] += 1
                    left, top = bx > 0 or A, by > 0 or B
                    if by == 0:
                        ur, ur_edge = (B, B_edge) if bx < 3 else (C, C_edge)
                    else:
                        ur, ur_edge = bx < 3 and _ORDER4[(bx + 1, by - 1)] < _ORDER4[(bx, by)], False
                    if m in (3, 7):
                        c[(p + "i4ur", m, int(ur))] += 1
                        if ur_edge:
                            c[(p + "sliceedge", "i4ur")] += 1
                    if m == 2:
                        c[(p + "i4dc", _which(left, top))] += 1
                        if by == 0 and B_edge:
                            c[(p + "sliceedge", "i4dc")] += 1
        else:
            for by in range(2):
                for bx in range(2):
                    m = int(ipred[8 * by + 2 * bx])
                    c[(p + "i8", m)] += 1
                    left, top = bx > 0 or A, by > 0 or B
                    if by == 0:
                        ur, ur_edge = (B, B_edge) if bx == 0 else (C, C_edge)
                    else:
                        ur, ur_edge = bx == 0, False
                    if m in (0, 2, 3, 7):
                        c[(p + "i8ur", m, int(ur))] += 1
                        if ur_edge:
                            c[(p + "sliceedge", "i8ur")] += 1
                    if m == 2:
                        c[(p + "i8dc", _which(left, top))] += 1
                        if by == 0 and B_edge:
                            c[(p + "sliceedge", "i8dc")] += 1
    return c


def table(transform_8x8, slice_mbs, div=1):
    """What an I-picture census must hold: {cell: minimum}.  div: 4 for the configurations whose
    thresholds are a quarter (RDO on, 10 bits), never below 1."""
    n = lambda v: max(1, v // div)
    t = {}
    for m in range(9):
        t[("i4", m)] = n(16)
        if transform_8x8:
            t[("i8", m)] = n(8)
    for m in range(4):
        t[("i16", m)] = n(2)
        t[("chroma", m)] = n(4)
    t[("i16cbp", 0)] = t[("i16cbp", 15)] = t[("i16dc128",)] = 1
    for m in (3, 7):
        t[("i4ur", m, 0)] = t[("i4ur", m, 1)] = 1
    kinds = ["i4", "i16", "chroma"]
    if transform_8x8:
        kinds.append("i8")
        for m in (0, 2, 3, 7):
            t[("i8ur", m, 0)] = t[("i8ur", m, 1)] = 1
    for k in kinds:
        for nb in ("left", "top", "none"):
            t[(k + "dc", nb)] = 1
    if slice_mbs:
        # the missing neighbour of a DC prediction lies in another slice, not outside the picture.  (A mode
        # that needs the above-right block needs the above one too, which in a raster run comes earlier:
        # a slice edge never takes the first alone.)
        for k in kinds:
            t[("sliceedge", k + "dc")] = 1
        if slice_mbs < W // 16 + 2:
            # plane prediction needs the above-left macroblock, W / 16 + 1 macroblocks back: no run this
            # short holds it together with the current one.  The one-slice configurations carry these cells.
            del t[("i16", 3)], t[("chroma", 3)]
    return t


def p_table(transform_8x8, constrained, div=1):
    n = lambda v: max(1, v // div)
    t = {("pmb", I4MB): n(8), ("pmb", I16MB): n(8)}
    if transform_8x8:
        t[("pmb", I8MB)] = n(8)
    if constrained:
        t[("pintra_inter_la",)] = n(4)
    return t


def table_misses(c, t):
    """The cells of table t that census c misses: [(cell, count, minimum)]."""
    return [(k, c[k], v) for k, v in t.items() if c[k] < v]


def dominant_mode(c):
    """The most frequent non-DC Intra8x8 mode of a census."""
    return max((m for m in range(9) if m != 2), key=lambda m: c[("i8", m)])


# ---------------------------------------------------------------- configurations
class Config:
    def __init__(self, name, kw, div=1):
        self.name, self.kw, self.div = name, kw, div
        self.bit_depth = kw.get("bit_depth", 8)
        self.t8 = kw.get("transform_8x8_mode", 0)


# Every configuration runs with slice_mbs 0 and 5, its P family with constrained_intra_pred 0 and 1.  The
# search modes matter on the device, where each has intra kernels of its own (test_directed_gpu.py);
# div 4: the thresholds of the configurations the table was not measured for beforehand.
CONFIGS = [
    Config("ffs_t4", dict(search_mode=0, transform_8x8_mode=0)),
    Config("ffs_t8", dict(search_mode=0, transform_8x8_mode=1)),
    Config("epzs_t4", dict(search_mode=3, transform_8x8_mode=0)),
    Config("epzs_t8", dict(search_mode=3, transform_8x8_mode=1)),
    Config("full_t4", dict(search_mode=-1, transform_8x8_mode=0)),
    Config("full_t8", dict(search_mode=-1, transform_8x8_mode=1)),
    Config("rdo_cavlc", dict(search_mode=3, transform_8x8_mode=1, rdo=1, symbol_mode=0), 4),
    Config("rdo_cabac", dict(search_mode=3, transform_8x8_mode=1, rdo=1, symbol_mode=1), 4),
    Config("bits10", dict(search_mode=3, transform_8x8_mode=1, bit_depth=10), 4),
]


def run_sets(enc, sets, slice_mbs, each=None):
    """Encode every picture of sets with enc (an OracleEncoder or an Encoder); returns the summed census
    and {set name: census}.  each(set, index, results, recon) sees every picture."""
    total, per = Counter(), {}
    for s in sets:
        cs = Counter()
        for i, pic in enumerate(s.pics):
            if s.refs:
                enc.set_reference(*s.refs[i])
            res, rec = enc.encode(*pic, s.slice_type, s.qp)
            cs += census(res, s.slice_type, W, slice_mbs)
            if each:
                each(s, i, res, rec)
        per[s.name] = cs
        total += cs
    return total, per


def _fmt(c, keys):
    return " ".join(f"{c[k]:4d}" for k in keys)


def print_census(title, c, t):
    print(f"## {title}")
    pre = "p" if any(k[0] == "pmb" for k in c) else ""
    print(f"  {pre}i4 modes 0..8     {_fmt(c, [(pre + 'i4', m) for m in range(9)])}")
    print(f"  {pre}i8 modes 0..8     {_fmt(c, [(pre + 'i8', m) for m in range(9)])}")
    print(f"  {pre}i16 modes 0..3    {_fmt(c, [(pre + 'i16', m) for m in range(4)])}    cbp 0 / 15: {c[(pre + 'i16cbp', 0)]} / "
          f"{c[(pre + 'i16cbp', 15)]}    |dc| >= 128: {c[(pre + 'i16dc128',)]}")
    print(f"  {pre}chroma modes 0..3 {_fmt(c, [(pre + 'chroma', m) for m in range(4)])}")
    if pre:
        print(f"  intra MBs I4 / I8 / I16: {c[('pmb', I4MB)]} / {c[('pmb', I8MB)]} / {c[('pmb', I16MB)]}    "
              f"inter left and above: {c[('pintra_inter_la',)]}")
    else:
        print("  above-right un/available: " + "  ".join(f"{k}{m}: {c[(k + 'ur', m, 0)]}/{c[(k + 'ur', m, 1)]}"
                                                          for k, ms in (("i4", (3, 7)), ("i8", (0, 2, 3, 7))) for m in ms))
        print("  DC left / top / none / both: " + "  ".join(f"{k}: " + "/".join(str(c[(k + 'dc', nb)]) for nb in ("left", "top", "none", "both"))
                                                             for k in ("i4", "i8", "i16", "chroma")))
        print("  below a slice edge: " + "  ".join(f"{k[1]}: {v}" for k, v in sorted(c.items()) if k[0] == "sliceedge"))
    miss = table_misses(c, t)
    print("  table: " + ("met" if not miss else "MISSED " + ", ".join(f"{k} {n} < {v}" for k, n, v in miss)))
    return not miss


def main():
    import oracle_lib
    ok = True
    for cfg in CONFIGS:
        isets, psets = for_depth(intra_sets(), cfg.bit_depth), for_depth(p_sets(), cfg.bit_depth)
        for slice_mbs in (0, 5):
            o = oracle_lib.OracleEncoder(W, H, search_range=8, slice_mbs=slice_mbs, **cfg.kw)
            c, per = run_sets(o, isets, slice_mbs)
            ok &= print_census(f"{cfg.name} slice_mbs={slice_mbs}: I pictures ({sum(len(s.pics) for s in isets)})", c,
                               table(cfg.t8, slice_mbs, cfg.div))
            if cfg.t8 and cfg.name == "ffs_t8" and not slice_mbs:
                print("  smooth families, most frequent non-DC Intra8x8 mode: " +
                      " ".join(f"{s.direction}:{dominant_mode(per[s.name])}" for s in isets if s.direction is not None))
            o.close()
        for slice_mbs, cip in ((0, 0), (5, 0), (0, 1), (5, 1)):
            o = oracle_lib.OracleEncoder(W, H, search_range=8, slice_mbs=slice_mbs, constrained_intra_pred=cip, **cfg.kw)
            c, _ = run_sets(o, psets, slice_mbs)
            ok &= print_census(f"{cfg.name} slice_mbs={slice_mbs} constrained_intra_pred={cip}: P pictures "
                               f"({sum(len(s.pics) for s in psets)})", c, p_table(cfg.t8, cip, cfg.div))
            o.close()
    return 0 if ok else 1


if __name__ == "__main__":
    import sys
    sys.exit(main())
