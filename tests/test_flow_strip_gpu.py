"""The 4x4 SAD strip of the next 8x8 block, computed under the last 4x4 sub-pel search of the block
before it: dataflow == ticks == oracle, bit for bit, on macroblocks whose 8x8 quadrants move apart.

The motion search keeps, per thread, the four 4x4 SADs of ONE 8x8 block at every search position.
The strip of block b + 1 overwrites them while block b's last search (4x4 bottom-right) is in its
sub-pel phase, and writes block b + 1's half of the 8x8 SAD table that the 16x16 / 16x8 / 8x16
searches read in block 3's stages.  What can go wrong there shows only where the blocks differ:

  * a strip taken for the wrong 8x8 block: that block's searches find another block's motion;
  * the SADs overwritten before block b's last full-pel argmin has read them: its bottom-right 4x4
    gets the next block's vector;
  * the table half written for the wrong block: the 16x8 / 8x16 searches see swapped halves.

So the pictures are I P P chains of 32x32 and 48x32 samples (deblocking on, SearchRange 32) of a
texture cut into 4x4 cells, each cell displaced by a vector of its own per picture: in a "quads"
macroblock the four 8x8 quadrants have a vector each and one of quadrants 1..3 four of them (one per
4x4 block), in a "halves" macroblock (the 48x32 chain) the upper and the lower half, or the left and
the right one, have one each.  The chains go through test_flow_chain_gpu's helpers;
test_quadrants_move_apart holds the oracle's results for them to a census on the CPU.
"""
import numpy as np
import pytest

import test_flow_chain_gpu as fc
from jmpaths import ensure_built, load_jmhip
from test_gpu_parity import assert_same

jmhip = load_jmhip()
P8X8, SUB4X4 = 8, 7


def texture(rng, w, h):
    """Texture with detail at the scale of a 4x4 block: a coarse random field, upsampled, plus noise."""
    coarse = rng.integers(30, 226, ((h + 3) // 4 + 1, (w + 3) // 4 + 1)).astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w] / 4.0
    y0, x0 = yy.astype(int), xx.astype(int)
    fy, fx = yy - y0, xx - x0
    v = (coarse[y0, x0] * (1 - fy) * (1 - fx) + coarse[y0, x0 + 1] * (1 - fy) * fx
         + coarse[y0 + 1, x0] * fy * (1 - fx) + coarse[y0 + 1, x0 + 1] * fy * fx)
    return np.clip(v + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint8)


def cell_vectors(w, h, seed):
    """(h/4, w/4, 2) full-pel (x, y) displacement per picture of every 4x4 cell.  Macroblocks
    alternate quads / halves in raster order where the picture is wider than 32, else all are quads."""
    rng = np.random.default_rng(seed)
    pool = [(x, y) for x in range(-3, 4) for y in range(-3, 4)]
    vec = np.zeros((h // 4, w // 4, 2), np.int64)
    for k, (my, mx) in enumerate((my, mx) for my in range(h // 16) for mx in range(w // 16)):
        v = [pool[j] for j in rng.permutation(len(pool))[:8]]
        mb = vec[4 * my:4 * my + 4, 4 * mx:4 * mx + 4]
        if w > 32 and k % 2:      # halves: 16x8 (upper / lower) or 8x16 (left / right)
            if k % 4 == 1:
                mb[:2], mb[2:] = v[0], v[1]
            else:
                mb[:, :2], mb[:, 2:] = v[0], v[1]
            continue
        for q in range(4):
            mb[2 * (q >> 1):2 * (q >> 1) + 2, 2 * (q & 1):2 * (q & 1) + 2] = v[q]
        q = 1 + k % 3             # this quadrant's 4x4 blocks go four ways
        for b in range(4):
            mb[2 * (q >> 1) + (b >> 1), 2 * (q & 1) + (b & 1)] = v[4 + b]
    return vec


def quad_seq(w, h, n, seed):
    rng = np.random.default_rng(seed)
    big = texture(rng, w + 64, h + 64)
    vec = cell_vectors(w, h, seed + 1000)
    pics = []
    for i in range(n):
        y = np.empty((h, w), np.uint8)
        for by in range(h // 4):
            for bx in range(w // 4):
                sx, sy = 32 + 4 * bx + i * vec[by, bx, 0], 32 + 4 * by + i * vec[by, bx, 1]
                y[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = big[sy:sy + 4, sx:sx + 4]
        pics.append(fc.with_chroma(y))
    return pics


# name -> (width, height, pictures, encoder settings): cases of test_flow_chain_gpu's helpers; the
# seeds are the first for which test_quadrants_move_apart holds
SEED32, SEED48 = 0, 0
STRIP_CASES = {}
for _had in (1, 0):
    for _rsr in (2, 0):
        _kw = dict(search_range=32, use_hadamard=_had, restrict_search_range=_rsr)
        STRIP_CASES[f"strip32_had{_had}_rsr{_rsr}"] = (32, 32, lambda: quad_seq(32, 32, 3, SEED32), _kw)
        STRIP_CASES[f"strip48_had{_had}_rsr{_rsr}"] = (48, 32, lambda: quad_seq(48, 32, 3, SEED48), _kw)
fc.CASES.update(STRIP_CASES)


def block_mvs(mv):
    """the MVs of a macroblock's four 8x8 blocks, each as the tuple of its four 4x4 MVs"""
    m = np.asarray(mv).reshape(4, 4, 2)
    return [tuple(m[2 * (q >> 1):2 * (q >> 1) + 2, 2 * (q & 1):2 * (q & 1) + 2].reshape(-1).tolist()) for q in range(4)]


@pytest.mark.parametrize("name", list(STRIP_CASES))
def test_quadrants_move_apart(name):
    """CPU: in some P picture of the oracle's chain one macroblock is P8x8 with different MVs in at
    least three of its 8x8 blocks and sub-mode 4x4 in one of blocks 1..3; in the 48x32 chains some
    macroblock of a P picture is 16x8 or 8x16 with a non-zero MV (block 3's searches read the 8x8
    table for it)."""
    w = STRIP_CASES[name][0]
    quads = halves = 0
    for i, (res, _, _) in enumerate(fc.oracle_chain(name)[1:], 1):
        print(f"picture {i}: mb_type {res['mb_type'].tolist()} b8mode {res['b8mode'].tolist()}")
        for k in range(len(res)):
            mt, mv = int(res["mb_type"][k]), res["mv"][k]
            if mt == P8X8 and len(set(block_mvs(mv))) >= 3 and (res["b8mode"][k][1:] == SUB4X4).any():
                quads += 1
            if mt in (2, 3) and mv.any():
                halves += 1
    assert quads >= 1, "no P8x8 macroblock with three different block MVs and a 4x4 sub-mode in blocks 1..3"
    if w == 48:
        assert halves >= 1, "no 16x8 / 8x16 macroblock with a non-zero MV"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STRIP_CASES))
def test_strip_flow_ticks_oracle(name):
    """dataflow == ticks == oracle: every result field, every reconstruction and deblocked plane."""
    ensure_built()
    jmhip.load()
    w = STRIP_CASES[name][0]
    want = fc.oracle_chain(name)
    for flow in (1, 0):
        got = fc.device_chain(name, flow)
        assert len(got) == len(want)
        for i, ((gres, grec, gdbk), (ores, orec, odbk)) in enumerate(zip(got, want)):
            assert_same(gres, grec, ores, orec, w // 16)
            for pl, (x, y) in enumerate(zip(gdbk, odbk)):
                assert np.array_equal(x, y), f"JMH_FLOW={flow} picture {i}: deblocked plane {pl} differs from the oracle chain"
