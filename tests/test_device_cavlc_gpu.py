"""CAVLC slice data written on the device (jmh_cavlc_write_slices / jmh_cavlc_write_results,
csrc/jmh_cavlc.hip) == the product's host writer (host/bitstream.c through host/cavlc_ref.c), byte
for byte and slice by slice; lencod -p DeviceCAVLC=1 writes the same .264 as DeviceCAVLC=0.

Every picture is written in four slice layouts (one slice; 1 MB, 7 MBs -- boundaries mid-row -- and
one row per slice) with lead bits of 0..7 bits.  Each encoder case asserts from the results that it
contains what it is there for (CASES: need), so it cannot pass vacuously."""
import subprocess
import tempfile

import numpy as np
import pytest

from jmpaths import JMDEC, LENCOD, ensure_built, load_jmhip
from test_gpu_parity import hbd_seq, moving_seq, run_lencod

jmhip = load_jmhip()
pytestmark = pytest.mark.gpu

I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE
LEADS = [(3, 0b101), (0, 0), (7, 0x55), (1, 1), (5, 0b10010), (2, 0), (6, 0x3f), (4, 0b1001)]


@pytest.fixture(scope="module", autouse=True)
def built():
    ensure_built()


def layouts(mbw, nmb):
    return [0, 1, 7, mbw] if nmb > 7 else [0, 1, mbw]


def assert_slices_equal(dev, ref, what):
    assert len(dev) == len(ref), what
    for i, (a, b) in enumerate(zip(dev, ref)):
        if a != b:
            k = next((j for j in range(min(len(a), len(b))) if a[j] != b[j]), min(len(a), len(b)))
            pytest.fail(f"{what}: slice {i} of {len(ref)} differs at byte {k} (device {len(a)} bytes, host {len(b)} bytes)")


def check_popped(enc, res, slice_type, what):
    """the picture last popped, through jmh_cavlc_write_slices, in every layout"""
    nmb = enc.mbw * enc.mbh
    for i, step in enumerate(layouts(enc.mbw, nmb)):
        d = jmhip.slice_descs(nmb, slice_type, step, lead=LEADS[i:] + LEADS[:i])
        ref = jmhip.cavlc_ref(enc.w, enc.h, enc.cfg.transform_8x8_mode, enc.cfg.constrained_intra_pred, res, d)
        assert_slices_equal(enc.cavlc_slices(d), ref, f"{what}, {step or nmb} MBs per slice")


# ---- what a case's results must contain -------------------------------------------------------
def coded_blocks(r):
    """the level arrays residual_block_cavlc codes for result r (cbp / I16 rules of write_mb)"""
    out = []
    if r["mb_type"] == jmhip_types.PSKIP:
        return out
    i16 = r["mb_type"] == jmhip_types.I16MB
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


class jmhip_types:
    PSKIP, P8x8, I4MB, I16MB, I8MB = 0, 8, 9, 10, 13


def stats(pictures):
    """pictures: [(slice_type, results)]; the properties the cases assert"""
    s = dict(max_abs=0, max_tc=0, i8=0, inter_t8=0, sub=set(), trailing_run=0, max_run=0)
    for st, res in pictures:
        run = 0
        for r in res:
            t = int(r["mb_type"])
            if st == P and t == jmhip_types.PSKIP:
                run += 1
                s["max_run"] = max(s["max_run"], run)
                continue
            run = 0
            for b in coded_blocks(r):
                b = np.asarray(b, np.int32)
                s["max_abs"] = max(s["max_abs"], int(np.abs(b).max()))
                s["max_tc"] = max(s["max_tc"], int(np.count_nonzero(b)))
            s["i8"] += t == jmhip_types.I8MB
            s["inter_t8"] += t < jmhip_types.I4MB and int(r["transform_8x8"]) == 1
            if t == jmhip_types.P8x8:
                s["sub"] |= {int(m) for m in r["b8mode"]}
        s["trailing_run"] = max(s["trailing_run"], run)     # one slice per picture: the picture ends in a skip run
    return s


def check_need(s, need):
    if "big_levels" in need:       # level_prefix >= 14 at suffixLength 0, and a full block
        assert s["max_abs"] >= 16 and s["max_tc"] == 16, s
    if "skip_runs" in need:        # a slice that ends in a skip run, and a run >= 8
        assert s["trailing_run"] >= 1 and s["max_run"] >= 8, s
    if "t8" in need:               # Intra8x8 and an inter MB with the 8x8 transform
        assert s["i8"] >= 1 and s["inter_t8"] >= 1, s
    if "sub8x8" in need:           # P8x8 with sub-macroblock types 8x4, 4x8 and 4x4
        assert {5, 6, 7} <= s["sub"], s


# (id, width, height, qp, (generator, seed, motion per picture), Encoder options, what the results
# must contain).  Every case but QP 51 (which skips: it carries its own requirement) must hold P8x8
# macroblocks with the sub-macroblock types 8x4, 4x8 and 4x4; seeds and motion were chosen so
# (the device's results equal the CPU oracle's, so the choice holds on any machine)
CASES = [
    ("qp0", 64, 48, 0, ("moving", 1, (5, -3)), dict(search_range=8), {"big_levels", "sub8x8"}),
    ("qp51", 64, 48, 51, ("moving", 7, (4, 0)), dict(search_range=8), {"skip_runs"}),
    ("ffs_qp28", 176, 144, 28, ("moving", 3, (5, -3)), dict(search_range=16), {"sub8x8"}),
    ("epzs_t8", 208, 128, 30, ("moving", 8, (5, -3)), dict(search_range=16, search_mode=3, transform_8x8_mode=1), {"t8", "sub8x8"}),
    ("cip", 176, 144, 28, ("moving", 6, (5, -3)), dict(search_range=16, constrained_intra_pred=1), {"sub8x8"}),
    ("high10_qp0", 176, 144, 0, ("hbd", 6, (29, -23)), dict(search_range=16, search_mode=3, bit_depth=10), {"big_levels", "sub8x8"}),
    ("rdo_cavlc", 176, 144, 28, ("moving", 7, (5, -3)), dict(search_range=16, search_mode=3, rdo=1, symbol_mode=0), {"sub8x8"}),
]


def case_pictures(w, h, gen):
    kind, seed, step = gen
    return hbd_seq(w, h, 4, seed, 10, step) if kind == "hbd" else moving_seq(w, h, 4, seed, step)


@pytest.mark.parametrize("name,w,h,qp,gen,kw,need", CASES, ids=[c[0] for c in CASES])
def test_encoder_results(name, w, h, qp, gen, kw, need):
    """I then 3 P pictures: device bytes == host bytes per slice, every layout, every picture"""
    enc = jmhip.Encoder(w, h, **kw)
    pictures = []
    for i, pic in enumerate(case_pictures(w, h, gen)):
        st = I if i == 0 else P
        res, rec = enc.encode(*pic, st, qp)
        pictures.append((st, res))
        check_popped(enc, res, st, f"{name} picture {i}")
        enc.set_reference(*rec)
    enc.close()
    check_need(stats(pictures), need)


# ---- the unit seam on synthetic results (64x48) ----------------------------------------------
W, H, NMB = 64, 48, 12


def max_results():
    res = np.zeros(NMB, jmhip.MB_RESULT_DTYPE)
    res["mb_type"], res["cbp"], res["ipred"] = jmhip_types.I16MB, 15 | (2 << 4), 2
    sign = np.where(np.arange(256) & 1, -32767, 32767).astype(np.int16)
    for a in range(NMB):
        res["i16mode"][a] = a & 3
        res["luma"][a] = np.roll(sign, a).reshape(16, 16)
        res["luma_dc"][a] = sign[:16]
        res["chroma_dc"][a] = -sign[:8].reshape(2, 4)
        res["chroma_ac"][a] = np.where(np.arange(128) % 3, -32767, 32767).astype(np.int16).reshape(2, 4, 16)
    return res


def ones_results(slice_p):
    res = np.zeros(NMB, jmhip.MB_RESULT_DTYPE)
    res["mb_type"], res["cbp"] = (1 if slice_p else jmhip_types.I4MB), 15 | (2 << 4)
    for a in range(NMB):
        for k in range(16):
            res["ipred"][a][k] = 2 if slice_p else (k + a) % 9
            i = np.arange(16)
            res["luma"][a][k] = np.where((i + k + a) % (2 + k % 3), 0, np.where((i + a) & 2, -1, 1))
        i = np.arange(128)
        res["chroma_ac"][a] = np.where((i + a) % 3, 0, np.where(i & 4, 1, -1)).reshape(2, 4, 16)
        res["chroma_dc"][a] = np.array([[-1, 0, 1, 0], [-1, 0, 1, 0]])
    return res


def skip_results(last_coded):
    res = np.zeros(NMB, jmhip.MB_RESULT_DTYPE)            # mb_type 0: P_Skip
    for a in range(NMB):
        res["mv"][a] = (a - 3, 2)
    if last_coded:
        res[NMB - 1] = ones_results(True)[5]
        res["mv"][NMB - 1] = (9, -4)
    return res


def random_results(rng, slice_p, t8):
    """random results that are valid input of write_mb (any values a slice of that type may hold)"""
    res = np.zeros(NMB, jmhip.MB_RESULT_DTYPE)
    T = jmhip_types
    for a in range(NMB):
        r = res[a]
        types = [0, 0, 1, 2, 3, 8, 8, T.I4MB, T.I16MB] + ([T.I8MB] if t8 else []) if slice_p else [T.I4MB, T.I16MB] + ([T.I8MB] if t8 else [])
        t = types[rng.integers(len(types))]
        i16, nxn = t == T.I16MB, t in (T.I4MB, T.I8MB)
        cbpl = 0 if rng.integers(4) == 0 else int(rng.integers(16))
        if i16:
            cbpl = 15 if cbpl & 1 else 0
        r["mb_type"], r["cbp"] = t, 0 if t == 0 else cbpl | (int(rng.integers(3)) << 4)
        r["i16mode"], r["c_ipred_mode"] = rng.integers(4), rng.integers(4)
        r["b8mode"] = rng.integers(4, 8, 4) if t == T.P8x8 else (11 if nxn else t)
        r["ref_idx"] = -1 if (i16 or nxn) else 0
        ip = rng.integers(0, 9, 16) if nxn else np.full(16, 2)
        if t == T.I8MB:
            ip = np.array([ip[(k & 8) | (k & 2)] for k in range(16)])
        r["ipred"] = ip
        mv = np.stack([rng.integers(-16, 17, 16), rng.integers(-4, 5, 16)], 1)
        big = rng.integers(8, size=16) == 0
        mv[big] = rng.integers(-32768, 32768, (int(big.sum()), 2))
        if t in (0, 1):
            mv[:] = mv[0]
        r["mv"] = mv
        r["transform_8x8"] = int(t8 and (t == T.I8MB or (not i16 and not nxn and t != 0 and rng.integers(2))))

        def levels(shape):
            k = rng.integers(16, size=shape)
            mag = np.select([k < 7, k < 11, k < 13, k < 15], [0, 1, rng.integers(1, 5, shape), rng.integers(1, 65, shape)],
                            rng.integers(1, 32768, shape))
            return np.where(rng.integers(2, size=shape), -mag, mag).astype(np.int16)
        r["luma"] = rng.integers(1, 4, (16, 16)) * (rng.integers(8, size=(16, 16)) > 0) if rng.integers(4) == 0 else levels((16, 16))
        r["luma_dc"], r["chroma_dc"], r["chroma_ac"] = levels(16), levels((2, 4)), levels((2, 4, 16))
    return res


@pytest.fixture(scope="module")
def seam():
    encs = {t8: jmhip.Encoder(W, H, search_range=8, transform_8x8_mode=t8) for t8 in (0, 1)}
    yield encs
    for e in encs.values():
        e.close()


def check_results(enc, res, slice_type, what, with_where=False):
    out = None
    for i, step in enumerate(layouts(enc.mbw, NMB)):
        d = jmhip.slice_descs(NMB, slice_type, step, lead=LEADS[i:] + LEADS[:i])
        ref = jmhip.cavlc_ref(W, H, enc.cfg.transform_8x8_mode, 0, res, d)
        dev, where = enc.cavlc_results(res, d, with_where=True)
        assert_slices_equal(dev, ref, f"{what}, {step or NMB} MBs per slice")
        if step == 1:
            out = where
    return out


def test_seam_all_max_levels(seam):
    """every MB Intra16x16 with all 400 levels +-32767 (level_prefix up to 19): the per-MB bound"""
    res = max_results()
    for st in (I, P):
        where = check_results(seam[0], res, st, "all-max")
        for (off, nbytes, nbits), (lead, _) in zip(where, (LEADS[1:] + LEADS[:1]) * 2):   # 1 MB per slice
            assert 14000 < nbits - lead <= jmhip.JMW_MB_MAX_BITS - 1 and nbytes == nbits // 8 + 1


def test_seam_ones_and_zero_patterns(seam):
    check_results(seam[0], ones_results(False), I, "+-1 / 0 (I)")
    check_results(seam[0], ones_results(True), P, "+-1 / 0 (P)")


def test_seam_all_skip(seam):
    res = skip_results(False)
    check_results(seam[0], res, P, "all P_Skip")
    assert seam[0].cavlc_results(res, jmhip.slice_descs(NMB, P)) == [bytes([0b00011011])]   # ue(12), stop bit


def test_seam_skip_except_last(seam):
    check_results(seam[0], skip_results(True), P, "P_Skip except the last MB")


def test_seam_random_results_200_pictures(seam):
    rng = np.random.default_rng(20240607)
    for pic in range(200):
        slice_p, t8 = pic % 3 != 0, (pic >> 1) & 1
        res = random_results(rng, slice_p, t8)
        d = jmhip.slice_descs(NMB, P if slice_p else I, [0, 1, 7, 4][pic & 3], lead=LEADS[pic & 7:] + LEADS[:pic & 7])
        ref = jmhip.cavlc_ref(W, H, t8, 0, res, d)
        assert_slices_equal(seam[t8].cavlc_results(res, d), ref, f"random picture {pic}")


@pytest.mark.parametrize("lead", range(8))
def test_seam_lead_bits(seam, lead):
    res = random_results(np.random.default_rng(lead), True, 1)
    d = jmhip.slice_descs(NMB, P, 7, lead=[(lead, 0xff), (lead, 0)])
    dev = seam[1].cavlc_results(res, d)
    assert_slices_equal(dev, jmhip.cavlc_ref(W, H, 1, 0, res, d), f"lead_nbits {lead}")
    assert dev[0][0] >> (8 - lead) == (1 << lead) - 1 and dev[1][0] >> (8 - lead) == 0


# ---- errors ------------------------------------------------------------------------------------
def test_errors():
    enc = jmhip.Encoder(W, H, search_range=8)
    one = jmhip.slice_descs(NMB, I)
    with pytest.raises(jmhip.JmhError) as e:               # no picture popped yet
        enc.cavlc_slices(one)
    assert e.value.status == jmhip.JMH_E_STATE
    res = ones_results(False)
    gap = jmhip.slice_descs(NMB, I, 4)
    gap[1].first_mb = 5
    over = jmhip.slice_descs(NMB, I, 4)
    over[2].n_mb = 5
    short = jmhip.slice_descs(NMB, I, 4)[:2]
    for bad in (gap, over, (jmhip.JmhSliceDesc * 2)(*short)):
        with pytest.raises(jmhip.JmhError) as e:
            enc.cavlc_results(res, bad)
        assert e.value.status == jmhip.JMH_E_INVALID_ARG
    data, where = enc.cavlc_results(res, one, with_where=True)
    total = where[-1][0] + where[-1][1]
    assert len(data[0]) == total
    # cap one byte short: rejected before anything is written
    import ctypes
    out = np.full(total, 0xa5, np.uint8)
    w = (jmhip.JmhSliceBytes * 1)()
    resc = np.ascontiguousarray(res)
    st = enc.lib.jmh_cavlc_write_results(enc.ctx, resc.ctypes.data, 1, ctypes.cast(one, ctypes.c_void_p), out.ctypes.data, total - 1,
                                         ctypes.cast(w, ctypes.c_void_p))
    assert st == jmhip.JMH_E_INVALID_ARG and (out == 0xa5).all() and w[0].nbytes == total
    st = enc.lib.jmh_cavlc_write_results(enc.ctx, resc.ctypes.data, 1, ctypes.cast(one, ctypes.c_void_p), out.ctypes.data, total,
                                         ctypes.cast(w, ctypes.c_void_p))
    assert st == 0 and out.tobytes() == data[0]
    enc.close()


# ---- pipelined: the call after every pop, pictures in flight behind it -------------------------
def test_pipelined_equals_depth_1():
    w, h, n = 320, 240, 8
    pics = moving_seq(w, h, n, 11, step=(7, -5))
    nmb = (w // 16) * (h // 16)

    def run(depth):
        enc = jmhip.Encoder(w, h, search_range=16, pipeline_depth=depth)
        assert (enc.depth > 1) == (depth != 1)
        out, pending = [], []

        def pop():
            i = pending.pop(0)
            res, _ = enc.pop()
            st = I if i == 0 else P
            d = jmhip.slice_descs(nmb, st, 0 if i & 1 else 20, lead=LEADS[i:])
            dev = enc.cavlc_slices(d)
            assert_slices_equal(dev, jmhip.cavlc_ref(w, h, 0, 0, res, d), f"depth {enc.depth} picture {i}")
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


# ---- lencod end to end ---------------------------------------------------------------------------
# two of tools/make_golden.py's CAVLC configurations: one slice per picture, and SliceMode 1
LENCOD_CASES = [
    ["InputFile=synthetic:1", "FramesToBeEncoded=10", "SourceWidth=176", "SourceHeight=144", "SearchRange=16"],
    ["InputFile=synthetic:4", "FramesToBeEncoded=4", "SourceWidth=352", "SourceHeight=288", "SearchRange=32",
     "ProfileIDC=100", "Transform8x8Mode=1", "SearchMode=3", "SliceMode=1", "SliceArgument=22"],
]


@pytest.mark.parametrize("extra", LENCOD_CASES, ids=["one_slice", "slice_mode_1"])
def test_lencod_device_cavlc_identical(extra):
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        log = run_lencod(LENCOD, a, extra + ["DeviceCAVLC=1"])
        assert "CAVLC slice data written on the device" in log
        run_lencod(LENCOD, b, extra + ["DeviceCAVLC=0"])
        assert open(f"{a}/a.264", "rb").read() == open(f"{b}/a.264", "rb").read(), "bitstreams differ"
        r = subprocess.run([JMDEC, f"{a}/a.264", f"{a}/dec.yuv"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert open(f"{a}/dec.yuv", "rb").read() == open(f"{a}/rec.yuv", "rb").read()
