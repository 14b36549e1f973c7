"""CABAC slice data written on the device (jmh_cabac_write_slices / jmh_cabac_write_results,
csrc/jmh_cabac.hip) == the product's host writer (host/cabac.c through host/cabac_ref.c), byte for
byte and bin count for bin count, slice by slice; lencod -p DeviceCABAC=1 writes the same .264 and the
same reconstruction as DeviceCABAC=0.

Every picture is written in four slice layouts (one slice; 1 MB, 7 MBs -- boundaries mid-row -- and
one row per slice).  Each encoder case asserts from the results that it contains what it is there
for (CASES: need), so it cannot pass vacuously."""
import ctypes
import subprocess
import tempfile

import numpy as np
import pytest

from jmpaths import JMDEC, LENCOD, ensure_built, load_jmhip
from test_gpu_parity import hbd_seq, moving_seq, run_lencod

jmhip = load_jmhip()
pytestmark = pytest.mark.gpu

I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE
PSKIP, P16x16, P8x8, I4MB, I16MB, I8MB = 0, 1, 8, 9, 10, 13


@pytest.fixture(scope="module", autouse=True)
def built():
    ensure_built()


def layouts(mbw, nmb):
    return [0, 1, 7, mbw] if nmb > 7 else [0, 1, mbw]


def assert_slices_equal(dev, ref, what):
    (dbytes, dwhere), (rbytes, rwhere) = dev, ref
    assert len(dbytes) == len(rbytes), what
    for i, (a, b) in enumerate(zip(dbytes, rbytes)):
        if a != b:
            k = next((j for j in range(min(len(a), len(b))) if a[j] != b[j]), min(len(a), len(b)))
            pytest.fail(f"{what}: slice {i} of {len(rbytes)} differs at byte {k} (device {len(a)} bytes, host {len(b)} bytes)")
    assert dwhere == rwhere, f"{what}: offsets / bytes / bins differ"


def check_popped(enc, res, slice_type, qp, what):
    """the picture last popped, through jmh_cabac_write_slices, in every layout"""
    nmb = enc.mbw * enc.mbh
    for step in layouts(enc.mbw, nmb):
        d = jmhip.cabac_slice_descs(nmb, slice_type, qp, step)
        ref = jmhip.cabac_ref(enc.w, enc.h, enc.cfg.transform_8x8_mode, enc.cfg.constrained_intra_pred, res, d, with_where=True)
        assert_slices_equal(enc.cabac_slices(d, with_where=True), ref, f"{what}, {step or nmb} MBs per slice")


# ---- what a case's results must contain -------------------------------------------------------
def coded_blocks(r):
    """the level arrays residual_block_cabac codes for result r (cbp / I16 rules of write_mb_body)"""
    out = []
    if r["mb_type"] == PSKIP:
        return out
    i16 = r["mb_type"] == I16MB
    cbpl, cbpc = int(r["cbp"]) & 15, int(r["cbp"]) >> 4
    if i16:
        out.append(r["luma_dc"])
    for k in range(16):
        if cbpl >> ((k >> 3) * 2 + ((k & 3) >> 1)) & 1:
            out.append(r["luma"][k][1:] if i16 else r["luma"][k])
    if cbpc:
        out += [r["chroma_dc"][0], r["chroma_dc"][1]]
    if cbpc == 2:
        out += [r["chroma_ac"][uv][k][1:] for uv in range(2) for k in range(4)]
    return out


def stats(pictures):
    """pictures: [(slice_type, results)]; the properties the cases assert"""
    s = dict(max_abs=0, max_tc=0, i8=0, inter_t8=0, sub=set(), trailing_run=0, max_run=0, max_mvd=0)
    for st, res in pictures:
        run = 0
        for r in res:
            t = int(r["mb_type"])
            if st == P and t == PSKIP:
                run += 1
                s["max_run"] = max(s["max_run"], run)
                continue
            run = 0
            for b in coded_blocks(r):
                b = np.asarray(b, np.int32)
                s["max_abs"] = max(s["max_abs"], int(np.abs(b).max()))
                s["max_tc"] = max(s["max_tc"], int(np.count_nonzero(b)))
            s["i8"] += t == I8MB
            s["inter_t8"] += t < I4MB and int(r["transform_8x8"]) == 1
            if t == P8x8:
                s["sub"] |= {int(m) for m in r["b8mode"]}
            if st == P and t < I4MB:
                # in the 1-MB-per-slice layout no neighbour is available: the MVP of an inter macroblock's
                # first partition is 0, its mvd = its mv
                s["max_mvd"] = max(s["max_mvd"], int(np.abs(np.asarray(r["mv"][0], np.int32)).max()))
        s["trailing_run"] = max(s["trailing_run"], run)     # one slice per picture: the picture ends in a skip run
    return s


def check_need(s, need):
    if "big_levels" in need:       # the UEG0 escape (|level| >= 16), and a full 16-coefficient block
        assert s["max_abs"] >= 16 and s["max_tc"] == 16, s
    if "skip_runs" in need:        # a slice that ends in skipped macroblocks, and a skip run >= 8
        assert s["trailing_run"] >= 1 and s["max_run"] >= 8, s
    if "t8" in need:               # Intra8x8 and an inter MB with the 8x8 transform
        assert s["i8"] >= 1 and s["inter_t8"] >= 1, s
    if "sub8x8" in need:           # P8x8 with sub-macroblock types 8x4, 4x8 and 4x4
        assert {5, 6, 7} <= s["sub"], s
    assert s["max_mvd"] >= 9, s    # every case: the UEG3 suffix of an mvd component


# (id, width, height, qp, (generator, seed, motion per picture), Encoder options, what the results must
# contain).  tests/test_device_cavlc_gpu.py's CASES with symbol_mode 1; without RDO the entropy coder
# does not change the results, so their seeds hold here too; the QP 51 case's seed was chosen anew (it
# must also hold an inter macroblock with |mvd| >= 9) and the RDO case's checked, both with the CPU oracle (the device's results equal the oracle's, so the choice holds on any machine)
CASES = [
    ("qp0", 64, 48, 0, ("moving", 1, (5, -3)), dict(search_range=8, symbol_mode=1), {"big_levels", "sub8x8"}),
    ("qp51", 64, 48, 51, ("moving", 11, (4, 0)), dict(search_range=8, symbol_mode=1), {"skip_runs"}),
    ("ffs_qp28", 176, 144, 28, ("moving", 3, (5, -3)), dict(search_range=16, symbol_mode=1), {"sub8x8"}),
    ("epzs_t8", 208, 128, 30, ("moving", 8, (5, -3)), dict(search_range=16, search_mode=3, transform_8x8_mode=1, symbol_mode=1),
     {"t8", "sub8x8"}),
    ("cip", 176, 144, 28, ("moving", 6, (5, -3)), dict(search_range=16, constrained_intra_pred=1, symbol_mode=1), {"sub8x8"}),
    ("high10_qp0", 176, 144, 0, ("hbd", 6, (29, -23)), dict(search_range=16, search_mode=3, bit_depth=10, symbol_mode=1),
     {"big_levels", "sub8x8"}),
    ("rdo_cabac", 176, 144, 28, ("moving", 7, (5, -3)), dict(search_range=16, search_mode=3, rdo=1, symbol_mode=1), {"sub8x8"}),
]


def case_pictures(w, h, gen):
    kind, seed, step = gen
    return hbd_seq(w, h, 4, seed, 10, step) if kind == "hbd" else moving_seq(w, h, 4, seed, step)


@pytest.mark.parametrize("name,w,h,qp,gen,kw,need", CASES, ids=[c[0] for c in CASES])
def test_encoder_results(name, w, h, qp, gen, kw, need):
    """I then 3 P pictures: device bytes and bins == host bytes and bins per slice, every layout, every
    picture (test_pipelined_pictures_in_flight makes the same calls with later pictures in flight)"""
    enc = jmhip.Encoder(w, h, **kw)
    pictures = []
    for i, pic in enumerate(case_pictures(w, h, gen)):
        st = I if i == 0 else P
        res, rec = enc.encode(*pic, st, qp)
        pictures.append((st, res))
        check_popped(enc, res, st, qp, f"{name} picture {i}")
        enc.set_reference(*rec)
    enc.close()
    check_need(stats(pictures), need)


def test_pipelined_pictures_in_flight():
    """the call after every pop with up to 4 later pictures in flight behind it == the same at depth 1"""
    w, h, n = 320, 240, 8
    pics = moving_seq(w, h, n, 11, step=(7, -5))
    nmb = (w // 16) * (h // 16)

    def run(depth):
        enc = jmhip.Encoder(w, h, search_range=16, pipeline_depth=depth, symbol_mode=1)
        assert (enc.depth > 1) == (depth != 1)
        out, pending = [], []

        def pop():
            i = pending.pop(0)
            res, _ = enc.pop()
            st = I if i == 0 else P
            d = jmhip.cabac_slice_descs(nmb, st, 28, 0 if i & 1 else 20)
            dev = enc.cabac_slices(d, with_where=True)
            assert_slices_equal(dev, jmhip.cabac_ref(w, h, 0, 0, res, d, with_where=True), f"depth {enc.depth} picture {i}")
            out.append(dev)
        for i, pic in enumerate(pics):
            if i:
                enc.set_reference_slot(-2)
            if len(pending) == enc.depth:
                pop()
            enc.push(*pic, I if i == 0 else P, 28, deblock=(0, 0, 0))
            pending.append(i)
        while pending:
            pop()
        enc.close()
        return out
    assert run(4) == run(1)


def test_one_row_per_slice_3840x48():
    """config 5's layout: 240-macroblock slices, High 10, one row per slice"""
    w, h, qp = 3840, 48, 24
    pics = hbd_seq(w, h, 2, 5, 10, (9, -2))
    enc = jmhip.Encoder(w, h, search_range=16, search_mode=3, bit_depth=10, symbol_mode=1)
    nmb = enc.mbw * enc.mbh
    for i, pic in enumerate(pics):
        st = I if i == 0 else P
        res, rec = enc.encode(*pic, st, qp)
        d = jmhip.cabac_slice_descs(nmb, st, qp, enc.mbw)
        assert len(d) == 3 and d[0].n_mb == 240
        ref = jmhip.cabac_ref(w, h, 0, 0, res, d, with_where=True)
        assert_slices_equal(enc.cabac_slices(d, with_where=True), ref, f"3840x48 picture {i}")
        enc.set_reference(*rec)
    enc.close()


# ---- the unit seam on synthetic results (64x48) ----------------------------------------------
W, H, NMB = 64, 48, 12
QPS = (0, 26, 51)


def extreme_results(slice_p, t8):
    """tests/harness/cabac_core_check.c's +-32767 / -32768 set: I16, I4, I8 (with t8) and, in P slices,
    P16x16 with and without the 8x8 transform, every level at the int16_t extremes"""
    res = np.zeros(NMB, jmhip.MB_RESULT_DTYPE)
    for a in range(NMB):
        r = res[a]
        pick = a % (5 if slice_p else 3)
        t = I16MB if pick == 0 else I4MB if pick == 1 else (I8MB if t8 else I4MB) if pick == 2 else P16x16
        r["mb_type"], r["cbp"] = t, 15 | (2 << 4)
        r["transform_8x8"] = int(t8 and (t == I8MB or pick == 4))
        r["i16mode"], r["c_ipred_mode"] = a & 3, (a >> 1) & 3
        i = np.arange(256)
        r["luma"] = np.where((i + a) & 1, -32768, 32767).reshape(16, 16)
        r["luma_dc"] = np.where(np.arange(16) & 1, 32767, -32768)
        r["chroma_dc"] = np.where(np.arange(8) & 2, 32767, -32768).reshape(2, 4)
        r["chroma_ac"] = np.where(np.arange(128) % 3, -32768, 32767).reshape(2, 4, 16)
        r["ipred"] = [(k + a) % 9 for k in range(16)] if t == I4MB else 2
        r["b8mode"] = 1 if t == P16x16 else 0 if t == I16MB else 11
        r["ref_idx"] = 0 if t == P16x16 else -1
    return res


def skip_results():
    res = np.zeros(NMB, jmhip.MB_RESULT_DTYPE)            # mb_type 0: P_Skip
    for a in range(NMB):
        res["mv"][a] = (a - 3, 2)
    return res


@pytest.fixture(scope="module")
def seam():
    encs = {t8: jmhip.Encoder(W, H, search_range=8, transform_8x8_mode=t8, symbol_mode=1) for t8 in (0, 1)}
    yield encs
    for e in encs.values():
        e.close()


def check_results(enc, res, slice_type, what):
    out = None
    for step in layouts(enc.mbw, NMB):
        d = jmhip.cabac_slice_descs(NMB, slice_type, QPS, step)
        ref = jmhip.cabac_ref(W, H, enc.cfg.transform_8x8_mode, 0, res, d, with_where=True)
        dev = enc.cabac_results(res, d, with_where=True)
        assert_slices_equal(dev, ref, f"{what}, {step or NMB} MBs per slice")
        if step == 1:
            out = dev[1]
    return out


@pytest.mark.parametrize("t8", (0, 1))
def test_seam_extreme_levels(seam, t8):
    """every level +-32767 / -32768: the per-macroblock bound in bins, 12 slices of one macroblock"""
    for st in (I, P):
        where = check_results(seam[t8], extreme_results(st == P, t8), st, f"extremes t8 {t8}")
        assert len(where) == 12
        assert max(w[2] for w in where) > 17000 and all(w[2] <= jmhip.JMC_MB_MAX_BINS for w in where)


def test_seam_all_skip(seam):
    where = check_results(seam[0], skip_results(), P, "all P_Skip")
    assert [w[2] for w in where] == [2] * 12               # mb_skip_flag, end_of_slice_flag 1


# ---- protocol ----------------------------------------------------------------------------------
def test_protocol():
    enc = jmhip.Encoder(W, H, search_range=8, symbol_mode=1)
    one = jmhip.cabac_slice_descs(NMB, I, 26)
    with pytest.raises(jmhip.JmhError) as e:               # no picture popped yet
        enc.cabac_slices(one)
    assert e.value.status == jmhip.JMH_E_STATE
    res = extreme_results(False, 0)
    gap = jmhip.cabac_slice_descs(NMB, I, 26, 4)
    gap[1].first_mb = 5
    over = jmhip.cabac_slice_descs(NMB, I, 26, 4)
    over[2].n_mb = 5
    short = (jmhip.JmhCabacSliceDesc * 2)(*jmhip.cabac_slice_descs(NMB, I, 26, 4)[:2])
    btype = jmhip.cabac_slice_descs(NMB, I, 26)
    btype[0].slice_type = 1
    for bad in (gap, over, short, btype, jmhip.cabac_slice_descs(NMB, I, 52), jmhip.cabac_slice_descs(NMB, I, -1)):
        with pytest.raises(jmhip.JmhError) as e:
            enc.cabac_results(res, bad)
        assert e.value.status == jmhip.JMH_E_INVALID_ARG
    rows = jmhip.cabac_slice_descs(NMB, I, QPS, 4)
    data, where = enc.cabac_results(res, rows, with_where=True)
    total = where[-1][0] + where[-1][1]
    assert sum(len(x) for x in data) == total
    assert enc.cabac_results(res, rows, with_where=True) == (data, where)        # the same call again: the same bytes
    # cap one byte short: rejected before anything is written, where[] filled
    out = np.full(total, 0xa5, np.uint8)
    w = (jmhip.JmhCabacSliceBytes * 3)()
    resc = np.ascontiguousarray(res)
    st = enc.lib.jmh_cabac_write_results(enc.ctx, resc.ctypes.data, 3, ctypes.cast(rows, ctypes.c_void_p), out.ctypes.data, total - 1,
                                         ctypes.cast(w, ctypes.c_void_p))
    assert st == jmhip.JMH_E_INVALID_ARG and (out == 0xa5).all()
    assert [(x.offset, x.nbytes, x.nbins) for x in w] == where
    st = enc.lib.jmh_cabac_write_results(enc.ctx, resc.ctypes.data, 3, ctypes.cast(rows, ctypes.c_void_p), out.ctypes.data, total,
                                         ctypes.cast(w, ctypes.c_void_p))
    assert st == 0 and out.tobytes() == b"".join(data)
    # two calls for the same popped picture
    pic = moving_seq(W, H, 1, 2, (3, 1))[0]
    r0, _ = enc.encode(*pic, I, 30)
    d = jmhip.cabac_slice_descs(NMB, I, 30, 4)
    first = enc.cabac_slices(d, with_where=True)
    assert enc.cabac_slices(d, with_where=True) == first
    assert_slices_equal(first, jmhip.cabac_ref(W, H, 0, 0, r0, d, with_where=True), "popped picture")
    enc.close()


# ---- lencod end to end ---------------------------------------------------------------------------
LENCOD_CASES = [
    ["InputFile=synthetic:1", "FramesToBeEncoded=6", "SourceWidth=176", "SourceHeight=144", "SearchRange=16", "ProfileIDC=77"],
    ["InputFile=synthetic:4", "FramesToBeEncoded=4", "SourceWidth=208", "SourceHeight=128", "SearchRange=16",
     "ProfileIDC=100", "Transform8x8Mode=1", "SearchMode=3"],
    ["InputFile=synthetic:5", "FramesToBeEncoded=4", "SourceWidth=208", "SourceHeight=128", "SearchRange=16", "ProfileIDC=110",
     "SourceBitDepthLuma=10", "SourceBitDepthChroma=10", "SearchMode=3", "RDOptimization=1", "SliceMode=1", "SliceArgument=13"],
    ["InputFile=synthetic:2", "FramesToBeEncoded=4", "SourceWidth=176", "SourceHeight=144", "SearchRange=16", "ProfileIDC=77",
     "PipelineDepth=1"],
]


@pytest.mark.parametrize("extra", LENCOD_CASES, ids=["main_one_slice", "high_t8_epzs", "high10_rdo_row_slices", "depth_1"])
def test_lencod_device_cabac_identical(extra):
    extra = extra + ["SymbolMode=1"]
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        log = run_lencod(LENCOD, a, extra + ["DeviceCABAC=1"])
        assert "CABAC slice data written on the device" in log
        run_lencod(LENCOD, b, extra + ["DeviceCABAC=0"])
        assert open(f"{a}/a.264", "rb").read() == open(f"{b}/a.264", "rb").read(), "bitstreams differ"
        assert open(f"{a}/rec.yuv", "rb").read() == open(f"{b}/rec.yuv", "rb").read(), "reconstructions differ"
        if "Transform8x8Mode=1" in extra:
            r = subprocess.run([JMDEC, f"{a}/a.264", f"{a}/dec.yuv"], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert open(f"{a}/dec.yuv", "rb").read() == open(f"{a}/rec.yuv", "rb").read()
