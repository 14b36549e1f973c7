"""k_mb_flow's macroblock chain on small pictures: dataflow == ticks == oracle, bit for bit.

Three things of the dataflow macroblock are aimed at here:
  * the half-pel planes b, h and j of the search window: sources that
    alternate 0 and 255 in 1-, 2- and 3-pixel checkerboards and stripes and in period-3 stripes
    (255 0 255 255 0 255 and 0 255 0 0 255 0 are the two ends of a 6-tap sum, 10710 and -2550),
    shifted by odd offsets from picture to picture;
  * the Intra16x16 and chroma intra-mode decisions of a P macroblock, which run on a wave that
    has no search in two of the search stages: a 32x32 picture has the four left / top availability
    combinations, and in every P picture one macroblock is the extension of the row above it (or
    of the column to its left), which makes Intra16x16 win there;
  * windows clamped at all four picture edges (32x32 at SearchRange 32).

The oracle chain is the CPU oracle's encode plus the loop filter written from 8.7
(deblock_ref.py), each P picture referencing the previous deblocked picture -- what run_chain does
on the device.  test_sequences_exercise_the_paths checks on the CPU that the sequences really give
what the GPU tests rely on.
"""
import functools

import numpy as np
import pytest

import deblock_ref as dr
import oracle_lib
from jmpaths import ensure_built, load_jmhip
from test_flow_gpu import env
from test_gpu_parity import assert_same, rand_picture, run_chain

jmhip = load_jmhip()
I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE
QP = 24
TAP_MIN, TAP_MAX = -2550, 10710               # a - 5b + 20c + 20d - 5e + f over bytes

# (kind, p): 0 checkerboard of p x p cells, 1 / 2 vertical / horizontal stripes p wide,
# 3 / 4 columns / rows with p of every 3 samples on, 5 the two of them XORed
KINDS = [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (4, 1), (4, 2), (5, 1), (5, 2)]


def pattern(kind, X, Y):
    k, p = kind
    if k == 0:
        v = ((X // p) + (Y // p)) & 1
    elif k == 1:
        v = (X // p) & 1
    elif k == 2:
        v = (Y // p) & 1
    elif k == 3:
        v = (X % 3) < p
    elif k == 4:
        v = (Y % 3) < p
    else:
        v = ((X % 3) < p) ^ ((Y % 3) < p)
    return np.where(v, 255, 0).astype(np.uint8)


def with_chroma(y):
    return np.ascontiguousarray(y), np.ascontiguousarray(y[::2, ::2] // 2 + 40), np.ascontiguousarray(255 - y[1::2, 1::2])


def extend_mb(y, i, w, h):
    """Picture i > 0: one macroblock (another one in every picture) becomes the extension of the row
    above it (of the column to its left in the top row, flat 128 at the origin) -- nothing in the
    reference predicts that, one Intra16x16 mode does, for fewer bits than sixteen Intra4x4 modes."""
    k = (7 * i) % ((w // 16) * (h // 16))
    x, yy = 16 * (k % (w // 16)), 16 * (k // (w // 16))
    if yy:
        y[yy:yy + 16, x:x + 16] = y[yy - 1, x:x + 16][None, :]
    elif x:
        y[yy:yy + 16, x:x + 16] = y[yy:yy + 16, x - 1][:, None]
    else:
        y[yy:yy + 16, x:x + 16] = 128


def checker_seq(w, h, n, seed, blend=False):
    """Tiles of the 0 / 255 patterns, the picture a window that moves by odd offsets.  blend: odd
    pictures are the rounded mean of the window and its diagonal neighbour, a half-sample shift in
    both directions (without the Hadamard transform a sub-pel position has to beat the full-pel SAD
    to win, which it never does where a full-pel position matches exactly)."""
    rng = np.random.default_rng(seed)
    bw, bh = w + 64, h + 64
    Y, X = np.mgrid[0:bh, 0:bw]
    big = np.zeros((bh, bw), np.uint8)
    order = rng.permutation(len(KINDS))
    for t, (ty, tx) in enumerate((ty, tx) for ty in range(0, bh, 16) for tx in range(0, bw, 16)):
        big[ty:ty + 16, tx:tx + 16] = pattern(KINDS[order[t % len(KINDS)]], X[ty:ty + 16, tx:tx + 16], Y[ty:ty + 16, tx:tx + 16])
    pics, x0, y0 = [], 32, 32
    for i in range(n):
        y = big[y0:y0 + h, x0:x0 + w].copy()
        if blend and i & 1:
            y = ((y.astype(np.int16) + big[y0 + 1:y0 + 1 + h, x0 + 1:x0 + 1 + w] + 1) >> 1).astype(np.uint8)
        if i:
            extend_mb(y, i, w, h)
        pics.append(with_chroma(y))
        x0 += int(rng.choice([-7, -5, -3, -1, 1, 3, 5, 7]))
        y0 += int(rng.choice([-5, -3, -1, 1, 3, 5]))
    return pics


def texture_seq(w, h, n, seed):
    """Smooth texture that moves by a few samples per picture, plus noise."""
    rng = np.random.default_rng(seed)
    big = rand_picture(rng, w + 64, h + 64)[0]
    pics = []
    for i in range(n):
        y = big[32 - 3 * i:32 - 3 * i + h, 32 + 5 * i:32 + 5 * i + w].copy()
        y = np.clip(y.astype(np.int16) + rng.integers(-4, 5, y.shape), 0, 255).astype(np.uint8)
        if i:
            extend_mb(y, i, w, h)
        pics.append(with_chroma(y))
    return pics


# name -> (width, height, pictures, encoder settings); the seeds are the first for which
# test_sequences_exercise_the_paths holds
CASES = {
    "texture32": (32, 32, lambda: texture_seq(32, 32, 4, 1), dict(search_range=32)),
    "checker80": (80, 48, lambda: checker_seq(80, 48, 4, 0), dict(search_range=32)),
    "checker80_sad": (80, 48, lambda: checker_seq(80, 48, 4, 0, blend=True), dict(search_range=32, use_hadamard=0)),
    "checker80_rsr0": (80, 48, lambda: checker_seq(80, 48, 4, 0), dict(search_range=32, restrict_search_range=0)),
}


@functools.lru_cache(maxsize=None)
def oracle_chain(name):
    """[(results, reconstruction, deblocked)] of the case's I P P P chain (computed once)."""
    ensure_built()
    w, h, pics, kw = CASES[name]
    o = oracle_lib.OracleEncoder(w, h, **kw)
    out = []
    for i, pic in enumerate(pics()):
        res, rec = o.encode(*pic, P if i else I, QP)
        dbk, _ = dr.deblock(rec, res, w // 16, h // 16, QP, 0, 0, 0, 8)
        dbk = tuple(np.asarray(p, np.uint8) for p in dbk)
        out.append((res, rec, dbk))
        o.set_reference(*dbk)
    o.close()
    return out


def tap_range(p):
    p = p.astype(np.int64)
    t = lambda a, b, c, d, e, f: a - 5 * b + 20 * c + 20 * d - 5 * e + f
    hz = t(p[:, :-5], p[:, 1:-4], p[:, 2:-3], p[:, 3:-2], p[:, 4:-1], p[:, 5:])
    vt = t(p[:-5], p[1:-4], p[2:-3], p[3:-2], p[4:-1], p[5:])
    return min(hz.min(), vt.min()), max(hz.max(), vt.max())


@pytest.mark.parametrize("name", list(CASES))
def test_sequences_exercise_the_paths(name):
    """CPU: the oracle's results for the sequence have an Intra16x16 macroblock in a P picture, an
    inter macroblock whose MV is fractional in both components, and sub-pel winners on each
    half-pel plane: (fx, fy) = (2, 0) is a b sample alone, (0, 2) an h sample alone, and (2, 2) --
    or, in the 32x32 sequence, a quarter position beside it, fx = 2 with fy odd or fy = 2 with fx
    odd -- reads j.  The checkerboard references reach both ends of the 6-tap range."""
    out = oracle_chain(name)
    i16 = frac = 0
    seen = set()
    for res, _, _ in out[1:]:
        mt = res["mb_type"]
        i16 += int((mt == 10).sum())
        for k in np.flatnonzero((mt >= 1) & (mt <= 8)):
            mv = res["mv"][k]
            frac += int((((mv[:, 0] & 3) != 0) & ((mv[:, 1] & 3) != 0)).any())
            seen |= {(int(x) & 3, int(y) & 3) for x, y in mv}
    assert i16 >= 1, "no Intra16x16 macroblock in a P picture"
    assert frac >= 1, "no inter macroblock with an MV fractional in both components"
    assert (2, 0) in seen and (0, 2) in seen, f"no winner on a b sample or on an h sample: {sorted(seen)}"
    reads_j = {(2, 2)} if name.startswith("checker") else {(2, 2), (2, 1), (2, 3), (1, 2), (3, 2)}
    assert seen & reads_j, f"no winner that reads a j sample: {sorted(seen)}"
    if name.startswith("checker"):
        refs = [tap_range(dbk[0]) for _, _, dbk in out[:-1]]
        assert min(r[0] for r in refs) == TAP_MIN and max(r[1] for r in refs) == TAP_MAX, refs


def device_chain(name, flow):
    w, h, pics, kw = CASES[name]
    with env(JMH_FLOW=flow):
        enc = jmhip.Encoder(w, h, **kw)
    out = run_chain(enc, pics(), QP, (0, 0, 0), True)
    assert (enc.timing().flow_launches > 0) == bool(flow)     # the path under test ran
    enc.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_flow_ticks_oracle(name):
    """dataflow == ticks == oracle: every result field, every reconstruction and deblocked plane."""
    ensure_built()
    jmhip.load()
    w = CASES[name][0]
    want = oracle_chain(name)
    for flow in (1, 0):
        got = device_chain(name, flow)
        assert len(got) == len(want)
        for i, ((gres, grec, gdbk), (ores, orec, odbk)) in enumerate(zip(got, want)):
            assert_same(gres, grec, ores, orec, w // 16)
            for pl, (x, y) in enumerate(zip(gdbk, odbk)):
                assert np.array_equal(x, y), f"JMH_FLOW={flow} picture {i}: deblocked plane {pl} differs from the oracle chain"
