"""The directed pictures (directed_pictures.py) make the oracle choose every intra mode: the census of
its results meets the table of DESIGN.md §6.1 in every configuration, and the decoder (oracle/decoder.c,
with intra predictors of its own) reproduces the reconstruction of every picture set.

These are conditions on the committed picture sets, not measurements: a configuration that misses a
cell gets more pictures, never a lower number.  The GPU side (test_directed_gpu.py) holds the
device's results against the same table."""
import subprocess
import tempfile

import numpy as np
import pytest

import directed_pictures as dp
import oracle_lib
from jmpaths import JMDEC, LENCOD_CPU, ensure_built

CASES = [pytest.param(c, id=c.name) for c in dp.CONFIGS]


@pytest.fixture(scope="module", autouse=True)
def built():
    ensure_built()


@pytest.fixture(scope="module")
def sets():
    cache = {}

    def get(bit_depth):
        if bit_depth not in cache:
            cache[bit_depth] = (dp.for_depth(dp.intra_sets(), bit_depth), dp.for_depth(dp.p_sets(), bit_depth))
        return cache[bit_depth]
    return get


def misses_text(misses):
    return ", ".join(f"{k}: {n} < {v}" for k, n, v in misses)


@pytest.mark.parametrize("slice_mbs", [0, 5])
@pytest.mark.parametrize("cfg", CASES)
def test_intra_census(cfg, slice_mbs, sets):
    """I pictures: every Intra4x4 / Intra8x8 / Intra16x16 / chroma mode wins its share, the DC
    predictions and the modes that read the above-right block win with and without their neighbours,
    Intra16x16 reaches luma cbp 0 and 15 and a DC level of 128."""
    o = oracle_lib.OracleEncoder(dp.W, dp.H, search_range=8, slice_mbs=slice_mbs, **cfg.kw)
    c, _ = dp.run_sets(o, sets(cfg.bit_depth)[0], slice_mbs)
    o.close()
    misses = dp.table_misses(c, dp.table(cfg.t8, slice_mbs, cfg.div))
    assert not misses, misses_text(misses)


@pytest.mark.parametrize("slice_mbs", [0, 5])
@pytest.mark.parametrize("cip", [0, 1])
@pytest.mark.parametrize("cfg", CASES)
def test_p_census(cfg, cip, slice_mbs, sets):
    """P pictures: Intra4x4, Intra8x8 and Intra16x16 macroblocks between inter macroblocks, with and
    without constrained intra prediction."""
    o = oracle_lib.OracleEncoder(dp.W, dp.H, search_range=8, slice_mbs=slice_mbs, constrained_intra_pred=cip, **cfg.kw)
    c, _ = dp.run_sets(o, sets(cfg.bit_depth)[1], slice_mbs)
    o.close()
    misses = dp.table_misses(c, dp.p_table(cfg.t8, cip, cfg.div))
    assert not misses, misses_text(misses)


def test_direction_names_the_mode(sets):
    """Independent of the oracle's mode numbering: a picture that varies along (a, b) only is constant
    along the direction one Intra8x8 mode predicts (H.264 table 8-3), and that mode is the most
    frequent non-DC one of its pictures (smooth families, QP 32, RDO off)."""
    o = oracle_lib.OracleEncoder(dp.W, dp.H, search_range=8, search_mode=0, transform_8x8_mode=1)
    _, per = dp.run_sets(o, sets(8)[0], 0)
    o.close()
    got = {s.direction: dp.dominant_mode(per[s.name]) for s in sets(8)[0] if s.direction is not None}
    assert got == {m: m for _, m in dp.DIRECTIONS}, got


def test_census_availability_by_position():
    """census() derives availability from position alone: hand-made results, one mode everywhere."""
    jm = oracle_lib.jmhip
    res = np.zeros(12, jm.MB_RESULT_DTYPE)
    res["mb_type"] = dp.I4MB
    res["ipred"] = 3
    c = dp.census(res, dp.I_SLICE, dp.W, 0)
    # above-right missing: 5 blocks of every macroblock (the right column below its first row, and blocks
    # 3 and 11 of the decoding order, whose above-right block comes later), the first block row of the
    # picture's first macroblock row (4 x 4), and block (3, 0) of the last macroblock of each lower row
    assert c[("i4", 3)] == 192 and c[("i4ur", 3, 0)] == 12 * 5 + 4 * 4 + 2
    res["mb_type"], res["i16mode"], res["c_ipred_mode"] = dp.I16MB, 2, 0
    c = dp.census(res, dp.I_SLICE, dp.W, 5)
    # runs 0-4, 5-9, 10-11 of a 4-wide picture: left only 1, 2, 3, 6, 7, 11; top only 4; both 9; none 0, 5, 8, 10
    assert [c[("i16dc", k)] for k in ("left", "top", "none", "both")] == [6, 1, 4, 1]
    assert c[("sliceedge", "i16dc")] == 6 and c[("chromadc", "top")] == 1


# ---------------------------------------------------------------- closed loop
def write_yuv(path, pics, bit_depth):
    with open(path, "wb") as f:
        for pic in pics:
            for p in pic:
                f.write(p.astype("<u2" if bit_depth > 8 else np.uint8).tobytes())


def lencod_args(cfg, slice_mbs, cip):
    kw = cfg.kw
    a = [f"SourceWidth={dp.W}", f"SourceHeight={dp.H}", "SearchRange=8", f"ProfileIDC={110 if cfg.bit_depth > 8 else 100}",
         f"Transform8x8Mode={cfg.t8}", f"UseConstrainedIntraPred={cip}", f"SymbolMode={kw.get('symbol_mode', 0)}",
         f"RDOptimization={kw.get('rdo', 0)}", f"SearchMode={kw.get('search_mode', 0)}"]
    if slice_mbs:
        a += ["SliceMode=1", f"SliceArgument={slice_mbs}"]
    if cfg.bit_depth > 8:
        a += [f"SourceBitDepthLuma={cfg.bit_depth}", f"SourceBitDepthChroma={cfg.bit_depth}"]
    return a


def closed_loop(pics, bit_depth, extra):
    with tempfile.TemporaryDirectory() as d:
        write_yuv(f"{d}/in.yuv", pics, bit_depth)
        args = [LENCOD_CPU, "-p", f"OutputFile={d}/a.264", "-p", f"ReconFile={d}/rec.yuv", "-p", f"InputFile={d}/in.yuv",
                "-p", f"FramesToBeEncoded={len(pics)}"]
        for e in extra:
            args += ["-p", e]
        r = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        r = subprocess.run([JMDEC, f"{d}/a.264", f"{d}/dec.yuv"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        rec = open(f"{d}/rec.yuv", "rb").read()
        assert len(rec) == len(pics) * dp.W * dp.H * 3 // 2 * (2 if bit_depth > 8 else 1)
        assert open(f"{d}/dec.yuv", "rb").read() == rec


@pytest.mark.parametrize("slice_mbs", [0, 5])
@pytest.mark.parametrize("cfg", CASES)
def test_closed_loop_intra(cfg, slice_mbs, sets):
    """The decoder's own intra predictors against every mode the census proves was chosen: all I pictures
    of one QP in one stream (the encoder's decisions are those of test_intra_census: same pictures,
    same parameters)."""
    by_qp = {}
    for s in sets(cfg.bit_depth)[0]:
        by_qp.setdefault(s.qp, []).extend(s.pics)
    for qp, pics in by_qp.items():
        closed_loop(pics, cfg.bit_depth, lencod_args(cfg, slice_mbs, 0) + ["IntraPeriod=1", f"QPFirstFrame={qp}", f"QPRemainingFrame={qp}"])


@pytest.mark.parametrize("cip", [0, 1])
@pytest.mark.parametrize("cfg", CASES)
def test_closed_loop_p(cfg, cip, sets):
    """The P family: each reference coded as an I picture at QP 4 (its reconstruction stays close to
    the picture), the checkerboard behind it as a P picture."""
    for s in sets(cfg.bit_depth)[1]:
        for ref, pic in zip(s.refs, s.pics):
            closed_loop([ref, pic], cfg.bit_depth, lencod_args(cfg, 0, cip) + ["QPFirstFrame=4", f"QPRemainingFrame={s.qp}"])
