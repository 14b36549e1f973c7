"""k_mb_flow hands a macroblock's analysis to its final in LDS: dataflow == ticks == oracle on chains
whose finals take every branch that reads the handed-over results.

The final (final_core) reads the analysis through a view: the tick kernels' view reads MbScratch in
HBM, k_mb_flow's reads the workgroup's LDS.  What it reads depends on the mode it decides on, so the
chains below are chosen for the census of P-picture macroblocks that test_census asserts on the CPU,
from the oracle's results alone:

  I4MB           the Intra4x4 levels, reconstruction, modes, cbp and block mask
  I16MB          the Intra16x16 cost and mode
  P8x8           best8x8 / cost8x8 and the MVs of two different sub-modes in one macroblock
  16x8 or 8x16   the partition costs and MVs of block types 2 / 3
  P_Skip         with a non-zero skip MV (skipx / skipy)
  16x16, cbp     an inter 16x16 whose MV equals the skip MV, but with cbp != 0: not skipped
  chroma mode    an intra macroblock with c_ipred_mode != 0 (c_mode)

and one I picture inside every chain (an I macroblock's analysis is intra_role's, not me_mb's).  The
GPU test cannot pass by never reaching a branch: the census is of the results it compares against.

The sequences are test_flow_chain_gpu's 32x32 texture and 80x48 checkerboards, and a 96x64 pan of
jmhip.synth_frame's picture: the same picture displaced by (3, -2) samples per picture, so that
flat areas skip with the neighbours' MV and textured ones code a residual at that MV.
"""
import functools

import numpy as np
import pytest

import deblock_ref as dr
import oracle_lib
from jmpaths import ensure_built, load_jmhip
from test_flow_chain_gpu import checker_seq, texture_seq, with_chroma
from test_flow_gpu import env
from test_gpu_parity import assert_same

jmhip = load_jmhip()
I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE
PSKIP, P16x16, P16x8, P8x16, P8x8, I4MB, I16MB = 0, 1, 2, 3, 8, 9, 10


def pan_seq(w, h, n, seed, step=(3, -2)):
    """A window of one synthetic picture that moves by `step` samples per picture."""
    big = jmhip.synth_frame(w + 64, h + 64, seed, 0)[0]
    pics = []
    for i in range(n):
        x0, y0 = 32 + step[0] * i, 32 + step[1] * i
        pics.append(with_chroma(big[y0:y0 + h, x0:x0 + w].copy()))
    return pics


# name -> (width, height, pictures, slice types, QP, encoder settings)
CASES = {
    "texture32": (32, 32, lambda: texture_seq(32, 32, 4, 1), (I, P, I, P), 24, dict(search_range=32)),
    "checker80": (80, 48, lambda: checker_seq(80, 48, 4, 0), (I, P, I, P), 24, dict(search_range=32)),
    "pan96": (96, 64, lambda: pan_seq(96, 64, 4, 3), (I, P, I, P), 30, dict(search_range=32)),
}
CENSUS = ("I4MB", "I16MB", "P8x8 with two sub-modes", "16x8 or 8x16", "P_Skip with a non-zero MV", "16x16 at the skip MV with cbp != 0",
          "intra with c_ipred_mode != 0")


@functools.lru_cache(maxsize=None)
def oracle_chain(name):
    """[(results, reconstruction, deblocked)] of the case's chain (computed once)."""
    ensure_built()
    w, h, pics, types, qp, kw = CASES[name]
    o = oracle_lib.OracleEncoder(w, h, **kw)
    out = []
    for pic, st in zip(pics(), types):
        res, rec = o.encode(*pic, st, qp)
        dbk, _ = dr.deblock(rec, res, w // 16, h // 16, qp, 0, 0, 0, 8)
        dbk = tuple(np.asarray(p, np.uint8) for p in dbk)
        out.append((res, rec, dbk))
        o.set_reference(*dbk)
    o.close()
    return out


def skip_mv(res, mbx, mby, mbw):
    """FindSkipModeMotionVector [J] / 8.4.1.1 from a picture's results (one slice, one reference)."""
    def nb(x, y, k):
        if x < 0 or y < 0 or x >= mbw:
            return None                                   # not available
        r = res[y * mbw + x]
        return (int(r["ref_idx"][((k >> 3) << 1) + ((k & 3) >> 1)]), int(r["mv"][k][0]), int(r["mv"][k][1]))
    a, b = nb(mbx - 1, mby, 3), nb(mbx, mby - 1, 12)
    c = nb(mbx + 1, mby - 1, 12)
    if c is None:
        c = nb(mbx - 1, mby - 1, 15)
    if a is None or b is None or a == (0, 0, 0) or b == (0, 0, 0):
        return 0, 0
    # 8.4.1.3: a neighbour that is intra (ref_idx -1) or missing counts with MV 0; one neighbour
    # alone with the reference gives its MV, otherwise the median
    c = c or (-1, 0, 0)
    same = [n for n in (a, b, c) if n[0] == 0]
    if len(same) == 1:
        return same[0][1], same[0][2]
    mv = [(n[1], n[2]) if n[0] >= 0 else (0, 0) for n in (a, b, c)]
    return sorted(m[0] for m in mv)[1], sorted(m[1] for m in mv)[1]


def census(name):
    """How many P-picture macroblocks of the oracle's chain are of each kind of CENSUS."""
    w = CASES[name][0]
    mbw = w // 16
    n = dict.fromkeys(CENSUS, 0)
    for (res, _, _), st in zip(oracle_chain(name), CASES[name][3]):
        if st != P:
            continue
        for k, r in enumerate(res):
            mt, intra = int(r["mb_type"]), int(r["mb_type"]) in (I4MB, I16MB)
            n["I4MB"] += mt == I4MB
            n["I16MB"] += mt == I16MB
            n["P8x8 with two sub-modes"] += mt == P8x8 and len(set(int(m) for m in r["b8mode"])) >= 2
            n["16x8 or 8x16"] += mt in (P16x8, P8x16)
            n["intra with c_ipred_mode != 0"] += intra and int(r["c_ipred_mode"]) != 0
            if mt in (PSKIP, P16x16):
                sk = skip_mv(res, k % mbw, k // mbw, mbw)
                mv = (int(r["mv"][0][0]), int(r["mv"][0][1]))
                if mt == PSKIP:
                    assert mv == sk, f"{name}: macroblock {k} is skipped at {mv}, skip_mv() gives {sk}"
                    n["P_Skip with a non-zero MV"] += mv != (0, 0)
                else:
                    assert mv != sk or int(r["cbp"]) != 0, f"{name}: macroblock {k} is a 16x16 at the skip MV without residual"
                    n["16x16 at the skip MV with cbp != 0"] += mv == sk
    return n


def test_census():
    """CPU: together the chains' P pictures hold every kind of macroblock of CENSUS, and every chain
    has an I picture after its first P picture."""
    total = dict.fromkeys(CENSUS, 0)
    for name in CASES:
        types = CASES[name][3]
        assert types[0] == I and I in types[types.index(P):], f"{name}: no I picture inside the chain"
        assert CASES[name][0] <= 96 and CASES[name][1] <= 64 and len(types) <= 4
        got = census(name)
        print(name, got)
        for k in CENSUS:
            total[k] += got[k]
    missing = [k for k in CENSUS if total[k] == 0]
    assert not missing, f"no macroblock of kind {missing} in any chain: {total}"


def device_chain(name, flow):
    w, h, pics, types, qp, kw = CASES[name]
    with env(JMH_FLOW=flow):
        enc = jmhip.Encoder(w, h, **kw)
    out, pending = [], 0
    for i, (pic, st) in enumerate(zip(pics(), types)):   # (test_gpu_parity.run_chain with slice types)
        if i:
            enc.set_reference_slot(-2)
        if pending == enc.depth:
            out.append(enc.pop() + (enc.deblocked(),))
            pending -= 1
        enc.push(*pic, st, qp, deblock=(0, 0, 0))
        pending += 1
    for _ in range(pending):
        out.append(enc.pop() + (enc.deblocked(),))
    assert (enc.timing().flow_launches > 0) == bool(flow)     # the path under test ran
    enc.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_handoff_flow_ticks_oracle(name):
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
