"""Coded pictures (jmh_frame_push_coded / jmh_frame_pop_coded, include/jmhip_coded.h):
the slice writer and the distortion kernel queued behind each pipelined picture.

The reference in every case is a second Encoder with the same configuration, fed the same pictures
through the ordinary push / pop, followed by the synchronous cavlc_slices / cabac_slices and
deblocked() (recon() where the picture is not deblocked).  Per picture: the bytes of every slice,
every where field (offsets relative to the first slice), and the three SSDs against numpy's
((src - output) ** 2).sum() over the crop in 64-bit integers -- all exact, there is no tolerance."""
import ctypes
import re
import tempfile

import numpy as np
import pytest

from jmpaths import LENCOD, ensure_built, load_jmhip
from test_gpu_parity import hbd_seq, moving_seq, run_lencod

jmhip = load_jmhip()
pytestmark = pytest.mark.gpu

I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE
LEADS = [(3, 0b101), (0, 0), (7, 0x55), (1, 1), (5, 0b10010), (2, 0), (6, 0x3f), (4, 0b1001)]
DBK = (0, 0, 0)


@pytest.fixture(scope="module", autouse=True)
def built():
    ensure_built()


def descs_for(enc, i, qp, step):
    nmb = enc.mbw * enc.mbh
    return jmhip.coded_slice_descs(nmb, I if i == 0 else P, qp, step, lead=LEADS[i % 8:] + LEADS[:i % 8])


def numpy_ssd(src, out, crop):
    cw, ch = crop
    sums = []
    for pl, (s, o) in enumerate(zip(src, out)):
        w, h = (cw, ch) if pl == 0 else (cw // 2, ch // 2)
        sums.append(int(((s[:h, :w].astype(np.int64) - o[:h, :w].astype(np.int64)) ** 2).sum()))
    return tuple(sums)


def chain(enc, pics, qp, dbk, step, coded, crop=None):
    """IPPP chain through the pipeline, popping only when it is full.  coded(i): picture i is pushed
    coded.  Per picture: coded -> ("c", data, where, stats, output or None); ordinary -> ("o", data, where, output, results)
    with data / where from the synchronous writer of the context's coder."""
    cabac = enc.cfg.symbol_mode != 0
    out, pending = [], []

    def pop():
        i = pending.pop(0)
        d = descs_for(enc, i, qp, step)
        if coded(i):
            data, where, stats = enc.pop_coded()
            assert not enc.lib.jmh_get_mb_result(enc.ctx, 0), "a coded picture's results stay on the device"
            pic = (enc.deblocked() if dbk else enc.recon()) if i % 4 == 0 else None   # on demand, from the device buffers
            out.append(("c", data, where, stats, pic))
        else:
            res, rec = enc.pop()
            a, b = jmhip.split_coded(d)
            data, where = enc.cabac_slices(b, with_where=True) if cabac else enc.cavlc_slices(a, with_where=True)
            out.append(("o", data, where, enc.deblocked() if dbk else rec, res))
    for i, pic in enumerate(pics):
        if i:
            enc.set_reference_slot(-2 if dbk else -1)
        if len(pending) == enc.depth:
            pop()
        if coded(i):
            enc.push_coded(*pic, I if i == 0 else P, qp, descs_for(enc, i, qp, step), crop=crop, deblock=dbk)
        else:
            enc.push(*pic, I if i == 0 else P, qp, deblock=dbk)
        pending.append(i)
    while pending:
        pop()
    return out


def rel(where, cabac):
    """(relative offset, nbytes, nbits or nbins) per slice, of either a coded or a synchronous where list"""
    o0 = where[0][0]
    if len(where[0]) == 4:
        return [(w[0] - o0, w[1], w[3] if cabac else w[2]) for w in where]
    return [(w[0] - o0, w[1], w[2]) for w in where]


def assert_coded_equals_ref(got, ref, pics, crop, cabac, what):
    assert len(got) == len(ref) == len(pics)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == "c" and r[0] == "o"
        _, data, where, stats, pic = g
        _, rdata, rwhere, rout, _ = r
        assert len(data) == len(rdata), f"{what} picture {i}"
        for k, (a, b) in enumerate(zip(data, rdata)):
            assert a == b, f"{what} picture {i}: slice {k} differs ({len(a)} vs {len(b)} bytes)"
        assert rel(where, cabac) == rel(rwhere, cabac), f"{what} picture {i}: where"
        for w in where:
            assert (w[2] == 0) if cabac else (w[3] == 0), "the other coder's field is 0"
        want = numpy_ssd(pics[i], rout, crop)
        print(f"{what} picture {i}: ssd {stats['ssd']} numpy {want} fallback {stats['fallback']}")
        assert stats["ssd"] == want, f"{what} picture {i}: ssd"
        if pic is not None:
            for a, b in zip(pic, rout):
                assert np.array_equal(a, b), f"{what} picture {i}: the picture read after the pop"


def run_case(w, h, qp, step, dbk, kw, make_pics, crop=None, n_pics=None, want_fallback=0):
    enc, ref = jmhip.Encoder(w, h, **kw), jmhip.Encoder(w, h, **kw)
    try:
        assert enc.ring_entries >= enc.depth + 2
        n = n_pics if n_pics is not None else enc.ring_entries + 3      # every ring entry is reused
        pics = make_pics(n)
        got = chain(enc, pics, qp, dbk, step, lambda i: True, crop)
        want = chain(ref, pics, qp, dbk, step, lambda i: False)
        assert_coded_equals_ref(got, want, pics, crop or (w, h), enc.cfg.symbol_mode != 0, f"{w}x{h} {kw}")
        if want_fallback is not None:
            assert all(g[3]["fallback"] == want_fallback for g in got)
        return got, want
    finally:
        enc.close()
        ref.close()


# ---- 1, 2: CAVLC on the dataflow path, every ring entry reused -------------------------------------
def test_cavlc_three_slices_deblocked():
    """64x48, slices of 5 / 5 / 2 macroblocks, SearchMode 0 (k_mb_flow feeds the writer), ring + 3 pictures"""
    got, _ = run_case(64, 48, 28, 5, DBK, dict(search_range=8, slice_mbs=5), lambda n: moving_seq(64, 48, n, 2, (5, -3)))
    assert [len(g[1]) for g in got] == [3] * len(got)


def test_cavlc_one_slice_not_deblocked():
    """one slice per picture, deblock off: the SSD is against the reconstruction"""
    run_case(64, 48, 28, 0, None, dict(search_range=8), lambda n: moving_seq(64, 48, n, 3, (5, -3)))


# ---- 3: CABAC, High profile ---------------------------------------------------------------------
@pytest.mark.parametrize("kw,hbd", [
    (dict(rdo=1), False),
    (dict(bit_depth=10), True),
], ids=["rdo", "high10"])
def test_cabac_high_profile(kw, hbd):
    """64x48, slices of 4 macroblocks, EPZS; bit_depth 10: the u16 SSD and the High 10 bins"""
    kw = dict(search_range=8, search_mode=3, transform_8x8_mode=1, symbol_mode=1, slice_mbs=4, **kw)
    mk = (lambda n: hbd_seq(64, 48, n, 4, 10, (5, -3))) if hbd else (lambda n: moving_seq(64, 48, n, 4, (5, -3)))
    got, _ = run_case(64, 48, 26, 4, DBK, kw, mk, n_pics=6)
    assert all(sum(w[3] for w in g[2]) > 0 for g in got)        # bins were counted


# ---- 4: crop ------------------------------------------------------------------------------------
def noise(w, h, seed, n=1):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
             rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)) for _ in range(n)]


def test_crop():
    """coded 48x32, crop 46x30 (not a dword multiple: 46 = 11 dwords + 2, chroma 23 = 5 dwords + 3)"""
    pics = noise(48, 32, 5, 3)
    # (noise at QP 30 needs more than the default capacity per macroblock: the first pictures may fall back, which changes nothing here)
    got, want = run_case(48, 32, 30, 0, DBK, dict(search_range=8), lambda n: pics, crop=(46, 30), n_pics=3, want_fallback=None)
    for g, r, pic in zip(got, want, pics):
        full = numpy_ssd(pic, r[3], (48, 32))
        assert all(a < b for a, b in zip(g[3]["ssd"], full)), (g[3]["ssd"], full)   # noise is not reconstructed exactly in the padding


# ---- 5: overflow fallback -----------------------------------------------------------------------
@pytest.mark.parametrize("symbol_mode", [0, 1], ids=["cavlc", "cabac"])
def test_overflow_falls_back_and_grows(symbol_mode, monkeypatch):
    """JMH_CODED_CAP so small that the first picture (noise at QP 4) overflows: it is coded by the
    synchronous path at its pop (fallback == 1, equal bytes); a picture pushed after that pop was
    queued with the grown capacity (fallback == 0, equal bytes)"""
    cap, w, h = 8, 64, 48
    nmb = (w // 16) * (h // 16)
    monkeypatch.setenv("JMH_CODED_CAP", str(cap))
    first = noise(w, h, 6)[0]
    pics = [first] * 5                                            # a still picture: the P pictures are small
    kw = dict(search_range=8, symbol_mode=symbol_mode, slice_mbs=4)
    got, want = run_case(w, h, 4, 4, DBK, kw, lambda n: pics, n_pics=5, want_fallback=None)
    total0 = sum(wh[1] for wh in want[0][2])
    assert total0 > ((nmb * cap + 3) & ~3), "the premise: the first picture's counted bytes exceed the configured capacity"
    assert got[0][3]["fallback"] == 1
    assert got[-1][3]["fallback"] == 0                            # pushed after the first pop: the grown capacity
    total_last = sum(wh[1] for wh in want[-1][2])
    print(f"symbol_mode {symbol_mode}: first picture {total0} bytes, last {total_last}, fallbacks {[g[3]['fallback'] for g in got]}")


# ---- 6: mixing and errors -----------------------------------------------------------------------
def test_mixed_with_ordinary_pictures_and_errors():
    w, h, qp, n = 64, 48, 28, 9
    kw = dict(search_range=8, slice_mbs=5)
    pics = moving_seq(w, h, n, 7, (5, -3))
    enc, ref = jmhip.Encoder(w, h, **kw), jmhip.Encoder(w, h, **kw)
    try:
        got = chain(enc, pics, qp, DBK, 5, lambda i: i % 2 == 1)
        want = chain(ref, pics, qp, DBK, 5, lambda i: False)
        for i, (g, r) in enumerate(zip(got, want)):
            assert g[0] == ("c" if i % 2 else "o")
            assert g[1] == r[1] and rel(g[2], False) == rel(r[2], False), f"picture {i}: bytes / where"
            if g[0] == "c":
                assert g[3]["ssd"] == numpy_ssd(pics[i], r[3], (w, h)) and g[3]["fallback"] == 0
            else:
                assert g[4].tobytes() == r[4].tobytes() and all(np.array_equal(a, b) for a, b in zip(g[3], r[3]))
    finally:
        enc.close()
        ref.close()

    enc = jmhip.Encoder(w, h, **kw)
    try:
        nmb = enc.mbw * enc.mbh
        assert nmb == 12
        good = descs_for(enc, 0, qp, 5)
        # descriptors that do not tile the picture: nothing is queued
        for runs in ([5, 5, 3], [5, 5], [12, 0], []):
            with pytest.raises(jmhip.JmhError) as e:
                enc.push_coded(*pics[0], I, qp, jmhip.coded_from_runs(runs, I, qp))
            assert e.value.status == jmhip.JMH_E_INVALID_ARG
        gap = jmhip.coded_from_runs([5, 5, 2], I, qp)
        gap[1].first_mb = 6
        bad_lead = jmhip.coded_from_runs([12], I, qp)
        bad_lead[0].lead_nbits = 8
        for d in (gap, bad_lead):
            with pytest.raises(jmhip.JmhError) as e:
                enc.push_coded(*pics[0], I, qp, d)
            assert e.value.status == jmhip.JMH_E_INVALID_ARG
        with pytest.raises(jmhip.JmhError) as e:
            enc.push_coded(*pics[0], I, qp, good, crop=(w + 1, h))
        assert e.value.status == jmhip.JMH_E_INVALID_ARG
        with pytest.raises(jmhip.JmhError) as e:                  # nothing was queued by any of them
            enc.pop()
        assert e.value.status == jmhip.JMH_E_STATE

        # the wrong pop returns JMH_E_STATE and loses nothing
        enc.push_coded(*pics[0], I, qp, good, deblock=DBK)
        with pytest.raises(jmhip.JmhError) as e:
            enc.pop()
        assert e.value.status == jmhip.JMH_E_STATE
        # a short cap: where is filled, the picture stays; a second pop with room succeeds
        with pytest.raises(jmhip.JmhError) as e:
            enc.pop_coded(cap=4)
        assert e.value.status == jmhip.JMH_E_INVALID_ARG
        short_where = e.value.where
        data, where, stats = enc.pop_coded()
        assert where == short_where and sum(wh[1] for wh in where) > 4
        assert data == want[0][1] and stats["ssd"] == numpy_ssd(pics[0], want[0][3], (w, h))
        enc.set_reference_slot(-2)
        enc.push(*pics[1], P, qp, deblock=DBK)
        where1, stats1 = (jmhip.JmhCodedBytes * 3)(), jmhip.JmhCodedStats()
        out = np.zeros(4096, np.uint8)
        st = enc.lib.jmh_frame_pop_coded(enc.ctx, out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.cast(where1, ctypes.c_void_p),
                                         ctypes.byref(stats1))
        assert st == jmhip.JMH_E_STATE
        res, _ = enc.pop()
        assert res.tobytes() == want[1][4].tobytes()
    finally:
        enc.close()


# ---- 7: lencod ----------------------------------------------------------------------------------
LENCOD_CASES = [
    ["InputFile=synthetic:31", "FramesToBeEncoded=6", "SourceWidth=176", "SourceHeight=144", "SearchRange=16", "SliceMode=1",
     "SliceArgument=13", "DeviceCAVLC=1"],
    ["InputFile=synthetic:32", "FramesToBeEncoded=6", "SourceWidth=176", "SourceHeight=144", "SearchRange=16", "ProfileIDC=110",
     "SourceBitDepthLuma=10", "SourceBitDepthChroma=10", "SearchMode=3", "RDOptimization=1", "SliceMode=1",
     "SliceArgument=13", "SymbolMode=1", "DeviceCABAC=1"],
    ["InputFile=synthetic:33", "FramesToBeEncoded=6", "SourceWidth=174", "SourceHeight=142", "SearchRange=16", "DeviceCAVLC=1"],
]
PIC_LINE = re.compile(r"^\s*(\d+)\((IDR| P )\)\s+(\d+)\s+(\d+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)\s")


def picture_columns(log):
    """(frame, type, bits, QP, SnrY, SnrU, SnrV) of every per-picture line, as printed"""
    rows = [m.groups() for m in map(PIC_LINE.match, log.splitlines()) if m]
    return rows


@pytest.mark.parametrize("extra", LENCOD_CASES, ids=["cavlc_slices", "cabac_high10_rdo", "cropped_recon"])
def test_lencod_device_writer_async_identical(extra):
    """DeviceWriterAsync=1 writes the same .264 and recon file and prints the same bits, QP and PSNR columns"""
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        la = run_lencod(LENCOD, a, extra + ["DeviceWriterAsync=1"])
        assert "queued behind each picture" in la
        lb = run_lencod(LENCOD, b, extra)
        assert "queued behind each picture" not in lb
        assert open(f"{a}/a.264", "rb").read() == open(f"{b}/a.264", "rb").read()
        assert open(f"{a}/rec.yuv", "rb").read() == open(f"{b}/rec.yuv", "rb").read()
        ca, cb = picture_columns(la), picture_columns(lb)
        assert len(ca) == 6 and ca == cb
