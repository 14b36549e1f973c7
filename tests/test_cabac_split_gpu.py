"""One CABAC slice coded on many waves (jmh_cabac_set_split, csrc/jmh_cabac_split.hip)
== the product's host writer (host/cabac.c through host/cabac_ref.c), byte for byte and bin count for
bin count, slice by slice.  The reference is always jmhip.cabac_ref; the unsplit device path
(k_cabac_code) is compared as well, but it is not the reference.  Coded pictures with the split set
equal those of a second context without it; lencod -p DeviceCABACSplit=64 writes the same .264 and
the same reconstruction as DeviceCABACSplit=0.

The ABI admits 16..65536 bins per chunk, so of a case's own chunk lengths (nbins, nbins - 1 and
(nbins + 1) // 2 of its longest slice) those outside that range are left out; the CPU test
(test_cabac_split_core.py) runs them all."""
import tempfile

import numpy as np
import pytest

from jmpaths import LENCOD, ensure_built, load_jmhip
from test_coded_gpu import DBK, assert_coded_equals_ref, chain, noise
from test_device_cabac_gpu import NMB, QPS, H, W, assert_slices_equal, extreme_results, skip_results
from test_gpu_parity import hbd_seq, moving_seq, run_lencod

jmhip = load_jmhip()
pytestmark = pytest.mark.gpu

I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE


@pytest.fixture(scope="module", autouse=True)
def built():
    ensure_built()


def chunks_of(where, L):
    """(chunks of the picture, chunks of the slice that has the most) for where[] and chunk length L"""
    per = [max(1, -(-w[2] // L)) for w in where]
    return sum(per), max(per)


def check_split(enc, call, ref, lengths, what):
    """call(): the device writer; ref: (bytes, where) of the host writer.  Unsplit, then every L"""
    enc.cabac_split(0)
    assert_slices_equal(call(), ref, f"{what}, unsplit")
    assert enc.cabac_split_info() == dict(chunk_bins=0, chunks=0, longest_slice_chunks=0, scratch_bytes=0, setting=0)
    for L in lengths:
        enc.cabac_split(L)
        assert_slices_equal(call(), ref, f"{what}, L = {L}")
        info = enc.cabac_split_info()
        total, longest = chunks_of(ref[1], L)
        assert (info["chunk_bins"], info["setting"], info["chunks"], info["longest_slice_chunks"]) == (L, L, total, longest), (what, L, info)
        if L < max(w[2] for w in ref[1]):
            assert longest > 1 and info["scratch_bytes"] > 0
    enc.cabac_split(0)


# ---- the unit seam on synthetic results (64x48) ----------------------------------------------
@pytest.fixture(scope="module")
def seam():
    encs = {t8: jmhip.Encoder(W, H, search_range=8, transform_8x8_mode=t8, symbol_mode=1) for t8 in (0, 1)}
    yield encs
    for e in encs.values():
        e.close()


SEAM = [("extremes_P", P, 0), ("extremes_P_t8", P, 1), ("extremes_I", I, 0), ("extremes_I_t8", I, 1), ("all_skip", P, 0)]


@pytest.mark.parametrize("name,st,t8", SEAM, ids=[c[0] for c in SEAM])
def test_seam(seam, name, st, t8):
    """every level +-32767 / -32768 (the longest carries and 0xff runs of the CPU sets) and all P_Skip (slices
    of 2 bins), in four layouts, chunks of 16, 64, 4096 and the longest slice's own lengths"""
    enc = seam[t8]
    res = skip_results() if name == "all_skip" else extreme_results(st == P, t8)
    for step in (0, 1, 5, 7):
        d = jmhip.cabac_slice_descs(NMB, st, QPS, step)
        ref = jmhip.cabac_ref(W, H, t8, 0, res, d, with_where=True)
        nbins = max(w[2] for w in ref[1])
        own = [L for L in (nbins, nbins - 1, (nbins + 1) // 2) if 16 <= L <= 65536]
        check_split(enc, lambda: enc.cabac_results(res, d, with_where=True), ref, [16, 64, 4096] + own, f"{name}, {step or NMB} MBs per slice")
        if name != "all_skip":
            assert nbins > 17000 and (step != 1 or len(own) == 3)


# ---- encoder results ---------------------------------------------------------------------------
@pytest.mark.parametrize("qp", (10, 30))
def test_encoder_results_main(qp):
    """96x64, I + P + P, Main: one slice and 6 MBs per slice, L = 64"""
    w, h = 96, 64
    enc = jmhip.Encoder(w, h, search_range=8, symbol_mode=1)
    nmb = enc.mbw * enc.mbh
    for i, pic in enumerate(moving_seq(w, h, 3, 4, (5, -3))):
        st = I if i == 0 else P
        res, rec = enc.encode(*pic, st, qp)
        for step in (0, 6):
            d = jmhip.cabac_slice_descs(nmb, st, qp, step)
            ref = jmhip.cabac_ref(w, h, 0, 0, res, d, with_where=True)
            check_split(enc, lambda: enc.cabac_slices(d, with_where=True), ref, [64], f"qp {qp} picture {i}, {step or nmb} MBs per slice")
        enc.set_reference(*rec)
    enc.close()


def test_encoder_results_high10_rdo_t8_row_slices():
    """128x64, High 10 + RDO + the 8x8 transform, one row per slice (config 5's shape in small), L = 256"""
    w, h, qp = 128, 64, 24
    enc = jmhip.Encoder(w, h, search_range=16, search_mode=3, bit_depth=10, rdo=1, transform_8x8_mode=1, symbol_mode=1)
    nmb = enc.mbw * enc.mbh
    multi = 0
    for i, pic in enumerate(hbd_seq(w, h, 3, 5, 10, (9, -2))):
        st = I if i == 0 else P
        res, rec = enc.encode(*pic, st, qp)
        d = jmhip.cabac_slice_descs(nmb, st, qp, enc.mbw)
        assert len(d) == 4
        ref = jmhip.cabac_ref(w, h, 1, 0, res, d, with_where=True)
        check_split(enc, lambda: enc.cabac_slices(d, with_where=True), ref, [256], f"high 10 picture {i}")
        multi += chunks_of(ref[1], 256)[1] > 1
        enc.set_reference(*rec)
    enc.close()
    assert multi, "no slice of any picture had more than one chunk"


# ---- coded pictures ----------------------------------------------------------------------------
def coded_pair(w, h, qp, step, kw, pics, split):
    """the five pictures as coded pictures of a context whose split follows split(i) before push i, all five
    pushed before the first pop, and of a context without a split"""
    kw = dict(kw, pipeline_depth=5)
    enc, ref = jmhip.Encoder(w, h, **kw), jmhip.Encoder(w, h, **kw)
    try:
        # chain() pops only when enc.depth pictures wait: five pushes precede the first pop
        assert enc.depth >= 5 and len(pics) == 5 and enc.ring_entries >= enc.depth + 2
        push = enc.push_coded

        def push_with_split(*a, **k):
            enc.cabac_split(split(push_with_split.i))
            push_with_split.i += 1
            return push(*a, **k)
        push_with_split.i = 0
        enc.push_coded = push_with_split
        got = chain(enc, pics, qp, DBK, step, lambda i: True)
        want = chain(ref, pics, qp, DBK, step, lambda i: False)
        assert_coded_equals_ref(got, want, pics, (w, h), True, f"{w}x{h} coded, split")
        return got
    finally:
        enc.close()
        ref.close()


def test_coded_pictures_split():
    """96x64, five pictures pushed before the first pop, split 64 set before the pushes"""
    w, h = 96, 64
    got = coded_pair(w, h, 20, 6, dict(search_range=8, symbol_mode=1, slice_mbs=6), moving_seq(w, h, 5, 9, (5, -3)), lambda i: 64)
    assert all(g[3]["fallback"] == 0 for g in got)
    assert max(wh[3] for g in got for wh in g[2]) > 64, "no slice has more than one chunk"


def test_coded_pictures_split_changes_between_pushes():
    """the split changes before every push, five settings in flight at once: a queued picture keeps what it was queued with"""
    w, h = 96, 64
    got = coded_pair(w, h, 20, 0, dict(search_range=8, symbol_mode=1), moving_seq(w, h, 5, 9, (5, -3)), lambda i: (64, 0, 16, 4096, 0)[i])
    assert all(g[3]["fallback"] == 0 for g in got)


def test_coded_pictures_split_overflow_falls_back(monkeypatch):
    """JMH_CODED_CAP so small that the first picture (noise at QP 4) overflows: coded at its pop by the
    synchronous path (fallback == 1), with the split, and equal bytes"""
    w, h = 64, 48
    monkeypatch.setenv("JMH_CODED_CAP", "8")
    pics = [noise(w, h, 6)[0]] * 5
    got = coded_pair(w, h, 4, 4, dict(search_range=8, symbol_mode=1, slice_mbs=4), pics, lambda i: 64)
    assert got[0][3]["fallback"] == 1


# ---- protocol ----------------------------------------------------------------------------------
def test_protocol():
    enc = jmhip.Encoder(W, H, search_range=8, symbol_mode=1)
    res = extreme_results(False, 0)
    d = jmhip.cabac_slice_descs(NMB, I, 26, 4)
    ref = jmhip.cabac_ref(W, H, 0, 0, res, d, with_where=True)
    assert enc.cabac_split_info()["setting"] == 0                      # the state after jmh_create
    enc.cabac_split(64)
    for bad in (1, 15, 65537, -1, 1 << 20):
        with pytest.raises(jmhip.JmhError) as e:
            enc.cabac_split(bad)
        assert e.value.status == jmhip.JMH_E_INVALID_ARG
        assert enc.cabac_split_info()["setting"] == 64                 # nothing changed
    assert_slices_equal(enc.cabac_results(res, d, with_where=True), ref, "after refused settings")
    assert enc.cabac_split_info()["chunks"] == chunks_of(ref[1], 64)[0]
    for ok in (16, 65536, 0):
        enc.cabac_split(ok)
        assert enc.cabac_split_info()["setting"] == ok
    assert_slices_equal(enc.cabac_results(res, d, with_where=True), ref, "split 0 again")
    info = enc.cabac_split_info()
    assert info["chunks"] == 0 and info["chunk_bins"] == 0
    enc.close()
    cavlc = jmhip.Encoder(W, H, search_range=8, symbol_mode=0)
    with pytest.raises(jmhip.JmhError) as e:
        cavlc.cabac_split(64)
    assert e.value.status == jmhip.JMH_E_UNSUPPORTED_CFG
    assert cavlc.cabac_split_info()["setting"] == 0
    sd = jmhip.slice_descs(NMB, P, 4)                                  # the context stays usable
    assert len(cavlc.cavlc_results(skip_results(), sd)) == 3
    cavlc.close()


# ---- lencod end to end ---------------------------------------------------------------------------
SMALL = ["FramesToBeEncoded=3", "SourceWidth=176", "SourceHeight=144", "SearchRange=16", "SymbolMode=1", "DeviceCABAC=1"]
LENCOD_CASES = [
    ["InputFile=synthetic:1", "ProfileIDC=77"] + SMALL,
    ["InputFile=synthetic:2", "ProfileIDC=77", "SliceMode=1", "SliceArgument=11"] + SMALL,
    ["InputFile=synthetic:5", "ProfileIDC=110", "SourceBitDepthLuma=10", "SourceBitDepthChroma=10", "SearchMode=3", "RDOptimization=1",
     "DeviceWriterAsync=1"] + SMALL,
]


@pytest.mark.parametrize("extra", LENCOD_CASES, ids=["main_one_slice", "slices_of_11", "high10_rdo_async"])
def test_lencod_split_identical(extra):
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        log = run_lencod(LENCOD, a, extra + ["DeviceCABACSplit=64"])
        assert "every slice in chunks of 64 bins" in log
        log = run_lencod(LENCOD, b, extra + ["DeviceCABACSplit=0"])
        assert "chunks of" not in log and "CABAC slice data written on the device" in log
        assert open(f"{a}/a.264", "rb").read() == open(f"{b}/a.264", "rb").read(), "bitstreams differ"
        assert open(f"{a}/rec.yuv", "rb").read() == open(f"{b}/rec.yuv", "rb").read(), "reconstructions differ"
