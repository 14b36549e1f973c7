"""The sub-pel searches of k_mb_flow and k_mb_analyse after their spiral decode moved into registers
and their motion-vector rate into the LDS table: dataflow == ticks == oracle, bit for bit, on pictures
whose winners sit where those two can go wrong.

A full-pel winner reaches the sub-pel search as its index in JM's spiral order and is decoded there
(csrc/jmh_spiral.h): an error in the ring number or at the switch from a ring's top / bottom entries to
its left / right ones moves the winner.  The candidates' rate lambda * (mvbits(dx) + mvbits(dy)) is read
from the table s.mvc: an index error shows where the difference to the predictor is large or
negative, a table error where lambda changes.  So the pictures are I P P chains of 48x48 and 64x48
samples of test_flow_strip_gpu's texture, cut into 4x4 cells that move by vectors of their own:

  * macroblock (1, 1): its neighbours A, B and C stand still, so its window centre is (0, 0), and (search
    ranges 4 and 8) its four 8x8 blocks move to the four corners (+-sr, +-sr) of the window -- (-sr, -sr)
    is a ring's first left / right entry, (sr, sr) its last entry; at search range 32 two of them move
    20 samples apart;
  * the macroblocks of the top row and of the left column stand still;
  * every other macroblock: an 8x8 quadrant on a ring's first entry (-l+1, -l), one on its last top /
    bottom entry (l-1, l), and eight 4x4 cells with vectors drawn from +-3.

Picture 0 is the texture undisplaced, so in picture 1 every cell has an exact full-pel match at its
vector; picture 2 references picture 1's displaced cells and brings the fractional winners.  Runs:
search ranges 4, 8 and 32, UseHadamard 1 / 0, RestrictSearchRange 2 / 0, QP 12 / 28 / 44 (lambda 1, 6 and 40).
test_census holds the oracle's results to what the GPU test relies on, on the CPU.
"""
import functools

import numpy as np
import pytest

import deblock_ref as dr
import oracle_lib
import test_flow_strip_gpu as fs
from jmpaths import ensure_built, load_jmhip
from test_flow_chain_gpu import with_chroma
from test_flow_gpu import env
from test_gpu_parity import assert_same, run_chain
from test_spiral_gpu import jm_spiral

jmhip = load_jmhip()
I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE
SKIP, P8X8, I4, I16 = 0, 8, 9, 10


def cell_vectors(w, h, sr, seed):
    """(h/4, w/4, 2) full-pel (x, y) displacement per picture of every 4x4 cell (see the module text)"""
    rng = np.random.default_rng(seed)
    pool = [(x, y) for x in range(-3, 4) for y in range(-3, 4)]
    vec = np.zeros((h // 4, w // 4, 2), np.int64)
    for my in range(1, h // 16):
        for mx in range(1, w // 16):
            mb = vec[4 * my:4 * my + 4, 4 * mx:4 * mx + 4]
            if (mx, my) == (1, 1):
                c = sr if sr <= 8 else 10
                quads = [(-c, -c), (c, -c), (-c, c), (c, c)] if sr <= 8 else [(-c, 0), (c, 0), (0, -c), (0, c)]
                for q in range(4):
                    mb[2 * (q >> 1):2 * (q >> 1) + 2, 2 * (q & 1):2 * (q & 1) + 2] = quads[q]
                continue
            l = 1 + int(rng.integers(0, min(sr, 3)))
            mb[:2, :2] = (-l + 1, -l)               # a ring's first entry
            mb[2:, 2:] = (l - 1, l)                 # its last top / bottom entry
            for b, j in enumerate(rng.permutation(len(pool))[:8]):
                q, k = (1, b) if b < 4 else (2, b - 4)
                mb[2 * (q >> 1) + (k >> 1), 2 * (q & 1) + (k & 1)] = pool[j]
    return vec


def cell_seq(w, h, n, sr, seed):
    rng = np.random.default_rng(seed)
    big = fs.texture(rng, w + 64, h + 64)
    vec = cell_vectors(w, h, sr, seed + 1000)
    pics = []
    for i in range(n):
        y = np.empty((h, w), np.uint8)
        for by in range(h // 4):
            for bx in range(w // 4):
                sx, sy = 32 + 4 * bx + i * vec[by, bx, 0], 32 + 4 * by + i * vec[by, bx, 1]
                y[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = big[sy:sy + 4, sx:sx + 4]
        pics.append(with_chroma(y))
    return pics


# name -> (width, height, QP, seed, encoder settings); the seeds are the first for which test_census holds
CASES = {
    "sr4_had1_rsr2_qp12": (48, 48, 12, 0, dict(search_range=4, use_hadamard=1, restrict_search_range=2)),
    "sr8_had0_rsr2_qp28": (64, 48, 28, 0, dict(search_range=8, use_hadamard=0, restrict_search_range=2)),
    "sr8_had1_rsr2_qp12": (48, 48, 12, 0, dict(search_range=8, use_hadamard=1, restrict_search_range=2)),
    "sr4_had0_rsr0_qp44": (64, 48, 44, 0, dict(search_range=4, use_hadamard=0, restrict_search_range=0)),
    "sr32_had1_rsr0_qp44": (64, 48, 44, 0, dict(search_range=32, use_hadamard=1, restrict_search_range=0)),
}


def pictures(name):
    w, h, _, seed, kw = CASES[name]
    return cell_seq(w, h, 3, kw["search_range"], seed)


@functools.lru_cache(maxsize=None)
def oracle_chain(name):
    """[(results, reconstruction, deblocked)] of the case's I P P chain (computed once)."""
    ensure_built()
    w, h, qp, _, kw = CASES[name]
    o = oracle_lib.OracleEncoder(w, h, **kw)
    out = []
    for i, pic in enumerate(pictures(name)):
        res, rec = o.encode(*pic, P if i else I, qp)
        dbk, _ = dr.deblock(rec, res, w // 16, h // 16, qp, 0, 0, 0, 8)
        dbk = tuple(np.asarray(p, np.uint8) for p in dbk)
        out.append((res, rec, dbk))
        o.set_reference(*dbk)
    o.close()
    return out


def device_chain(name, flow):
    w, h, qp, _, kw = CASES[name]
    with env(JMH_FLOW=flow):
        enc = jmhip.Encoder(w, h, **kw)
    out = run_chain(enc, pictures(name), qp, (0, 0, 0), True)
    assert (enc.timing().flow_launches > 0) == bool(flow)     # the path under test ran
    enc.close()
    return out


# ---- the census: where the oracle's winners sit -------------------------------------------------
def median3(a, b, c):
    return a + b + c - min(a, b, c) - max(a, b, c)


def mvp16(res, mbw, k):
    """SetMotionVectorPredictor of macroblock k's 16x16 block, one reference: neighbours A (left), B
    (above), C (above right, else D above left); an intra neighbour has reference -1 and MV 0"""
    mx, my = k % mbw, k // mbw

    def nb(x, y, blk):
        if x < 0 or y < 0 or x >= mbw:
            return None
        j = y * mbw + x
        if int(res["mb_type"][j]) in (I4, I16):
            return (-1, 0, 0)
        return (0, int(res["mv"][j][blk][0]), int(res["mv"][j][blk][1]))

    a, b, c = nb(mx - 1, my, 3), nb(mx, my - 1, 12), nb(mx + 1, my - 1, 12)
    if c is None:
        c = nb(mx - 1, my - 1, 15)
    if a is not None and b is None and c is None:
        return a[1], a[2]
    cand = [n if n is not None else (-1, 0, 0) for n in (a, b, c)]
    same = [n for n in cand if n[0] == 0]
    if len(same) == 1:
        return same[0][1], same[0][2]
    return median3(*(n[1] for n in cand)), median3(*(n[2] for n in cand))


def census(name):
    """counts over the P pictures of the oracle's chain: winners by their place in the window (full-pel
    MVs only, whose place is certain), fractional MVs, and MV differences to the left neighbour"""
    w, _, _, _, kw = CASES[name]
    sr, mbw = kw["search_range"], w // 16
    index = {(int(x), int(y)): n for n, (x, y) in enumerate(jm_spiral(sr))}
    seen = dict(corners=set(), ring_first=0, ring_last_tb=0, ring_first_side=0, ring_last=0, frac_both=0, far_left=0, skips=0)
    for res, _, _ in oracle_chain(name)[1:]:
        for k in range(len(res)):
            mt = int(res["mb_type"][k])
            if mt in (I4, I16):
                continue
            px, py = mvp16(res, mbw, k)
            mv = res["mv"][k].astype(int)
            if mt == SKIP:      # the restatement above, held against the oracle: a skipped macroblock's MV is its 16x16 predictor or zero
                assert tuple(mv[0]) in ((px, py), (0, 0)), (name, k, mv[0], px, py)
                seen["skips"] += 1
                continue
            cx, cy = (int(np.clip(int(p / 4), -sr, sr)) for p in (px, py))      # int(): toward zero, as the C division
            for b in range(16):
                x, y = mv[b]
                seen["frac_both"] += int(x & 3 != 0 and y & 3 != 0)
                if b & 3:
                    seen["far_left"] += int(max(abs(x - mv[b - 1][0]), abs(y - mv[b - 1][1])) > 64)
                rx, ry = x - 4 * cx, y - 4 * cy
                if rx & 3 or ry & 3 or (rx // 4, ry // 4) not in index:
                    continue
                rx, ry = rx // 4, ry // 4
                l = max(abs(rx), abs(ry))
                if l == 0:
                    continue
                n = index[(rx, ry)]
                if l == sr and abs(rx) == abs(ry):
                    seen["corners"].add((rx, ry))
                seen["ring_first"] += int(n == (2 * l - 1) ** 2)
                seen["ring_last_tb"] += int(n == (2 * l - 1) ** 2 + 2 * (2 * l - 1) - 1)
                seen["ring_first_side"] += int(n == (2 * l - 1) ** 2 + 2 * (2 * l - 1))
                seen["ring_last"] += int(n == (2 * l + 1) ** 2 - 1)
    return seen


@pytest.mark.parametrize("name", list(CASES))
def test_census(name):
    """CPU, on the oracle's results.  Search ranges 4 and 8 with RestrictSearchRange 2 (with 0 a sub-block
    searches half the range, and at QP 44 the cells' exact matches no longer all win): a block MV at
    each of the four corners of its macroblock's window, and a winner on a ring's first entry, on its
    last top / bottom entry, on its first left / right entry and on its last entry.  Every run: an MV
    fractional in both components.  Search range 32: a block whose MV differs from its left
    neighbour's by more than 64 quarter-pels."""
    kw = CASES[name][4]
    sr = kw["search_range"]
    seen = census(name)
    print(name, seen)
    if sr <= 8 and kw["restrict_search_range"]:
        assert seen["corners"] == {(-sr, -sr), (sr, -sr), (-sr, sr), (sr, sr)}, seen
        for key in ("ring_first", "ring_last_tb", "ring_first_side", "ring_last"):
            assert seen[key] >= 1, (key, seen)
    assert seen["frac_both"] >= 1 and seen["skips"] >= 1, seen
    if sr == 32:
        assert seen["far_left"] >= 1, seen


def test_the_runs_cover_the_settings():
    kws = [c[4] for c in CASES.values()]
    assert {k["search_range"] for k in kws} == {4, 8, 32}
    assert {k["use_hadamard"] for k in kws} == {0, 1} and {k["restrict_search_range"] for k in kws} == {0, 2}
    assert {c[2] for c in CASES.values()} == {12, 28, 44}
    assert [jmhip.QP2QUANT[max(0, q - 12)] for q in (12, 28, 44)] == [1, 6, 40]
    assert {(c[0], c[1]) for c in CASES.values()} == {(48, 48), (64, 48)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_subpel_flow_ticks_oracle(name):
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
