"""NAL units finished on the device (include/jmhip_nal.h) against tests/nal_ref.py,
the packaging restated from the standard: the synchronous seam on the directed units of
tests/nal_cases.py, armed coded pictures against un-armed ones of a second encoder, the fallback, and
lencod DeviceNAL=1 against DeviceNAL=0."""
import subprocess
import tempfile

import numpy as np
import pytest

import nal_cases
import nal_ref
from jmpaths import JMDEC, LENCOD, ensure_built, load_jmhip
from test_gpu_parity import hbd_seq, moving_seq, run_lencod

jmhip = load_jmhip()
pytestmark = pytest.mark.gpu

I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE
DBK = (0, 0, 0)
W, H = 64, 48
NMB = (W // 16) * (H // 16)


@pytest.fixture(scope="module", autouse=True)
def built():
    ensure_built()


@pytest.fixture(scope="module")
def enc8():
    e = jmhip.Encoder(W, H, search_range=8)
    yield e
    e.close()


def wrap(enc, units, nbins=0, cap=None):
    """jmh_nal_wrap of units whose payloads lie one behind the other, three bytes of filler between them"""
    payload, where = bytearray(), []
    for _, _, _, pay in units:
        payload += b"\xEE\x00\x00"
        where.append((len(payload), len(pay)))
        payload += pay
    return enc.nal_wrap([(r, t, h) for r, t, h, _ in units], payload, where, nbins, cap)


def check_units(enc, units, what, nbins=0, bit_depth=8):
    want, want_where = nal_ref.access_unit(units, nbins, NMB, bit_depth)
    got, where = wrap(enc, units, nbins)
    assert where == want_where, f"{what}: where"
    assert got == want, f"{what}: bytes ({len(got)} vs {len(want)})"
    return want


# ---- 1: the synchronous seam ---------------------------------------------------------------------
def test_wrap_directed_units(enc8):
    tile, chunk = jmhip.nal_geometry()
    rng = np.random.default_rng(7)
    groups = {
        "runs around the tile": nal_cases.runs_around(tile),
        "runs around the chunk": nal_cases.runs_around(chunk),
        "runs across the junction": nal_cases.runs_across_junction(),
        "sizes": nal_cases.sized_units(tile, rng) + nal_cases.sized_units(chunk, rng),
        "chunks of zeros": nal_cases.zero_chunks(chunk),
        "units in a row": nal_cases.units_in_a_row(),
        "random": nal_cases.random_units(2000, chunk, rng),
    }
    total = {"escapes": 0, "tile": 0, "chunk": 0, "junction": 0, "zero_chunk": 0}
    for name, units in groups.items():
        check_units(enc8, units, name)
        for k, v in nal_ref.census(units, tile, chunk).items():
            total[k] += v
    print(f"{sum(len(u) for u in groups.values())} units, census {total}")
    assert all(v >= 1 for v in total.values()), total
    for name in ("runs around the tile", "runs around the chunk", "runs across the junction", "chunks of zeros"):
        key = {"runs around the tile": "tile", "runs around the chunk": "chunk", "runs across the junction": "junction",
               "chunks of zeros": "zero_chunk"}[name]
        assert nal_ref.census(groups[name], tile, chunk)[key] >= 1, name


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_wrap_zero_words(bit_depth, enc8):
    enc = enc8 if bit_depth == 8 else jmhip.Encoder(W, H, search_range=8, bit_depth=10, transform_8x8_mode=1)
    try:
        cases = [c for c in nal_cases.zero_word_cases(NMB) if c[2] == bit_depth]
        assert len(cases) == 6
        for unit, bins, bd, words in cases:
            plain = check_units(enc, [unit], "no bins", 0, bd)
            au = check_units(enc, [unit], f"bins {bins}", bins, bd)
            assert len(au) - len(plain) == 3 * words and au[len(plain):] == b"\x00\x00\x03" * words, (bins, bd, words)
            assert nal_ref.zero_words_closed_form(bins, len(plain) - 4, NMB, bd) == words
        # several units: the words follow the last one and count towards it
        units = [cases[3][0], nal_cases.run_unit(9, 3, 1, 2), cases[3][0]]
        check_units(enc, units, "three units and words", cases[5][1] * 3, bit_depth)
    finally:
        if enc is not enc8:
            enc.close()


def test_wrap_cap_one_byte_short(enc8):
    units = nal_cases.units_in_a_row()
    want, want_where = nal_ref.access_unit(units)
    with pytest.raises(jmhip.JmhError) as ei:
        wrap(enc8, units, cap=len(want) - 1)
    assert ei.value.status == jmhip.JMH_E_INVALID_ARG and ei.value.total == len(want) and ei.value.where == want_where
    got, where = wrap(enc8, units, cap=len(want))
    assert got == want and where == want_where


# ---- 2: coded pictures ---------------------------------------------------------------------------
TAILS = (b"\x00\x00", b"\x00", b"\x01")


def heads_for(i, n):
    """Picture i's heads: they end in 00 00, in 00, in 01 in turn, so that zero runs cross the junction"""
    return [(3 if i == 0 else 2, 5 if i == 0 else 1, bytes([0x88, 0x80 | k, i + 1][:(i + k) % 4]) + TAILS[(i + k) % 3]) for k in range(n)]


def noise(n, bd=8):
    rng = np.random.default_rng(11)
    dt, hi = (np.uint8, 256) if bd == 8 else (np.uint16, 1 << bd)
    pic = (rng.integers(0, hi, (H, W), dtype=dt), rng.integers(0, hi, (H // 2, W // 2), dtype=dt), rng.integers(0, hi, (H // 2, W // 2), dtype=dt))
    return [pic] * n


def coded_chain(enc, n, qp, step, push, armed):
    """I P P ... through the pipeline, popping when it is full; armed(i): picture i gets heads"""
    out, pending = [], 0
    nmb = enc.mbw * enc.mbh
    for i in range(n):
        if i:
            enc.set_reference_slot(-2)
        if pending == enc.depth:
            out.append(enc.pop_coded())
            pending -= 1
        d = jmhip.coded_slice_descs(nmb, I if i == 0 else P, qp, step, lead=[(3, 0b101), (0, 0), (7, 0x55)])
        push(i, I if i == 0 else P, d, heads_for(i, len(d)) if armed(i) else None)
        pending += 1
    while pending:
        out.append(enc.pop_coded())
        pending -= 1
    return out


def assert_armed_equals_ref(got, want, armed, cabac, bit_depth, what):
    assert len(got) == len(want)
    for i, ((data, where, stats), (rdata, rwhere, rstats)) in enumerate(zip(got, want)):
        assert stats["ssd"] == rstats["ssd"], f"{what} picture {i}: ssd"
        assert [w[2:] for w in where] == [w[2:] for w in rwhere], f"{what} picture {i}: nbits / nbins"
        if not armed(i):
            assert data == rdata and where == rwhere, f"{what} picture {i}: an un-armed picture"
            continue
        heads = heads_for(i, len(rdata))
        units = [(r, t, h, pay) for (r, t, h), pay in zip(heads, rdata)]
        au, au_where = nal_ref.access_unit(units, sum(w[3] for w in rwhere) if cabac else 0, NMB, bit_depth)
        assert [w[:2] for w in where] == au_where, f"{what} picture {i}: where"
        assert b"".join(data) == au, f"{what} picture {i}: the access unit"
        print(f"{what} picture {i}: {len(au)} bytes, {len(au) - sum(len(h[2]) + len(p) for h, p in zip(heads, rdata)) - 5 * len(heads)} "
              f"escape and zero-word bytes, fallback {stats['fallback']}")


CODED = {
    "cavlc3_noise_qp10": (dict(search_range=8, slice_mbs=5), 5, 10, "noise", 0, False),
    "cavlc3_pan_qp30": (dict(search_range=8, slice_mbs=5), 5, 30, "pan", 0, False),
    "cabac_rows_noise_qp10": (dict(search_range=8, search_mode=3, transform_8x8_mode=1, symbol_mode=1, slice_mbs=4), 4, 10, "noise", 0, False),
    "cabac_rows_pan_qp30_split64": (dict(search_range=8, search_mode=3, transform_8x8_mode=1, symbol_mode=1, slice_mbs=4), 4, 30, "pan", 64, False),
    "cabac_high10_pan_qp26": (dict(search_range=8, search_mode=3, transform_8x8_mode=1, symbol_mode=1, slice_mbs=4, bit_depth=10), 4, 26, "pan10", 0,
                              False),
    "cavlc3_pan_qp30_device": (dict(search_range=8, slice_mbs=5), 5, 30, "pan", 0, True),
}


@pytest.mark.parametrize("case", list(CODED), ids=list(CODED))
def test_armed_coded_pictures(case, monkeypatch):
    """Armed pop_coded == nal_ref on (heads, the un-armed pop_coded bytes of a second encoder fed the
    same pictures); armed and un-armed pictures alternate (I armed, P not, P armed, ...)"""
    kw, step, qp, src, split, device = CODED[case]
    monkeypatch.setenv("JMH_CODED_CAP", "1024")                   # noise at QP 10 stays on the device path
    n = 5
    bd = kw.get("bit_depth", 8)
    pics = noise(n, bd) if src == "noise" else hbd_seq(W, H, n, 4, 10, (5, -3)) if src == "pan10" else moving_seq(W, H, n, 4, (5, -3))
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    armed = lambda i: i % 2 == 0
    try:
        if split:
            enc.cabac_split(split)
            ref.cabac_split(split)
        if device:
            dev = [enc.device_picture(jmhip.to_device(p, jmhip.JMH_PIX_I420)) for p in pics]
            push = lambda i, st, d, heads: enc.push_coded_device(dev[i], st, qp, d, deblock=DBK, heads=heads)
        else:
            push = lambda i, st, d, heads: enc.push_coded(*pics[i], st, qp, d, deblock=DBK, heads=heads)
        got = coded_chain(enc, n, qp, step, push, armed)
        want = coded_chain(ref, n, qp, step, lambda i, st, d, heads: ref.push_coded(*pics[i], st, qp, d, deblock=DBK), lambda i: False)
        assert_armed_equals_ref(got, want, armed, kw.get("symbol_mode", 0) != 0, bd, case)
        assert all(g[2]["fallback"] == 0 for g in got)
    finally:
        enc.close()
        ref.close()


def test_arming_is_for_one_push_and_n_must_match():
    pics = moving_seq(W, H, 3, 5, (5, -3))
    enc = jmhip.Encoder(W, H, search_range=8, slice_mbs=5)
    try:
        d = jmhip.coded_slice_descs(NMB, I, 28, 5)
        assert len(d) == 3
        with pytest.raises(jmhip.JmhError) as ei:                  # two heads for three slices
            enc.push_coded(*pics[0], I, 28, d, deblock=DBK, heads=heads_for(0, 2))
        assert ei.value.status == jmhip.JMH_E_INVALID_ARG
        enc.push_coded(*pics[0], I, 28, d, deblock=DBK)            # nothing was queued, the arming is gone
        plain = enc.pop_coded()
        heads = jmhip.nal_heads(heads_for(1, 3))
        jmhip._check(enc.lib.jmh_coded_nal_heads(enc.ctx, 3, heads), "jmh_coded_nal_heads")
        enc.push(*pics[0], I, 28, deblock=DBK)                     # an ordinary push drops it as well
        enc.pop()
        enc.push_coded(*pics[0], I, 28, d, deblock=DBK)
        again = enc.pop_coded()
        assert again[0] == plain[0] and again[1] == plain[1]
        enc.push_coded(*pics[0], I, 28, d, deblock=DBK, heads=heads_for(0, 3))
        data, where, _ = enc.pop_coded()
        au, au_where = nal_ref.access_unit([(r, t, h, p) for (r, t, h), p in zip(heads_for(0, 3), plain[0])])
        assert b"".join(data) == au and [w[:2] for w in where] == au_where
        assert enc.lib.jmh_coded_nal_heads(enc.ctx, 0, heads) == jmhip.JMH_E_INVALID_ARG
        heads[1].nbytes = jmhip.JMH_NAL_HEAD_MAX + 1
        assert enc.lib.jmh_coded_nal_heads(enc.ctx, 3, heads) == jmhip.JMH_E_INVALID_ARG
    finally:
        enc.close()


# ---- 3: fallback ---------------------------------------------------------------------------------
@pytest.mark.parametrize("symbol_mode", [0, 1], ids=["cavlc", "cabac"])
def test_armed_overflow_falls_back_and_grows(symbol_mode, monkeypatch):
    """JMH_CODED_CAP as test_coded_gpu.py's test_overflow_falls_back_and_grows sets it: the first armed
    picture is finished by the synchronous calls at its pop (fallback 1, equal bytes), a later one on
    the device again"""
    monkeypatch.setenv("JMH_CODED_CAP", "8")
    pics = noise(5)
    kw = dict(search_range=8, symbol_mode=symbol_mode, slice_mbs=4)
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    try:
        got = coded_chain(enc, 5, 4, 4, lambda i, st, d, heads: enc.push_coded(*pics[i], st, 4, d, deblock=DBK, heads=heads), lambda i: True)
        want = coded_chain(ref, 5, 4, 4, lambda i, st, d, heads: ref.push_coded(*pics[i], st, 4, d, deblock=DBK), lambda i: False)
        assert_armed_equals_ref(got, want, lambda i: True, symbol_mode != 0, 8, f"overflow {symbol_mode}")
        assert sum(w[1] for w in want[0][1]) > ((NMB * 8 + 3) & ~3), "the premise: the first picture exceeds the configured capacity"
        assert got[0][2]["fallback"] == 1 and got[-1][2]["fallback"] == 0
    finally:
        enc.close()
        ref.close()


# ---- 4: lencod -----------------------------------------------------------------------------------
LENCOD_CASES = {
    "cavlc_three_slices": ["InputFile=synthetic:41", "SliceMode=1", "SliceArgument=33", "DeviceCAVLC=1"],
    "cabac_split64": ["InputFile=synthetic:42", "ProfileIDC=100", "SymbolMode=1", "Transform8x8Mode=1", "SliceMode=1", "SliceArgument=11",
                      "DeviceCABAC=1", "DeviceCABACSplit=64"],
    "cavlc_device_input": ["InputFile=synthetic:43", "SliceMode=1", "SliceArgument=33", "DeviceCAVLC=1", "DeviceInput=1"],
}


@pytest.mark.parametrize("case", list(LENCOD_CASES), ids=list(LENCOD_CASES))
def test_lencod_device_nal_identical(case):
    """DeviceNAL=1 writes the same .264 as DeviceNAL=0 and reports the same bits; the stream decodes to the recon file"""
    extra = ["FramesToBeEncoded=4", "SourceWidth=176", "SourceHeight=144", "SearchRange=16", "QPFirstFrame=20", "QPRemainingFrame=22",
             "DeviceWriterAsync=1"] + LENCOD_CASES[case]
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        la = run_lencod(LENCOD, a, extra + ["DeviceNAL=1"])
        lb = run_lencod(LENCOD, b, extra + ["DeviceNAL=0"])
        assert "NAL units finished on the device" in la and "NAL units finished on the device" not in lb
        sa, sb = open(f"{a}/a.264", "rb").read(), open(f"{b}/a.264", "rb").read()
        assert sa == sb and len(sa) > 0
        bits = lambda log: [ln.split()[1] for ln in log.splitlines() if "(IDR)" in ln or "( P )" in ln]
        assert len(bits(la)) == 4 and bits(la) == bits(lb)
        total = lambda log: [ln for ln in log.splitlines() if "SNR Y(dB)" in ln]
        assert total(la) == total(lb) and total(la)
        r = subprocess.run([JMDEC, f"{a}/a.264", f"{a}/dec.yuv"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert open(f"{a}/dec.yuv", "rb").read() == open(f"{a}/rec.yuv", "rb").read()
