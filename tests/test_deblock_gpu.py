"""The fused device deblocking (csrc/jmh_deblock.h: deblock_mb inside final_core, k_mb_flow and
k_rdo_final) == the reference written from H.264 8.7 (tests/deblock_ref.py), sample for sample.

For every picture the reference is given the device's own reconstruction and results of that
picture (their equality with the oracle is pinned by test_gpu_parity.py and its siblings), so a
difference here is the filter's.  P pictures reference the device-deblocked previous picture
(set_reference_slot(-2)), the product path.  The cases and the threshold sweep are those of
test_deblock_ref.py (deblock_cases.py), run through every route that reaches deblock_mb:

    route          kernel that deblocks (jmh_launch_final / c->flow in jmhip_abi.hip)
    flow           k_mb_flow: final_core<512 threads> -> deblock_prefetch + deblock_mb<u8, 512, PRE>
    ticks          JMH_FLOW=0: k_mb_final512<u8, false> (the same body, one launch per tick)
    epzs, cip      no dataflow path: k_mb_final512<u8, false> behind the EPZS / constrained-intra analysis
    slice*         flow, with slice edges inside the picture (idc 0 filters across them)
    t8             k_mb_final<5, u8, true>
    hbd9, hbd10    k_mb_final<8, u16, true>
    rdo_*          k_rdo_final: deblock_mb<pel, 256, no prefetch>, 8 and 10 bits, CAVLC and CABAC rates
k_mb_final<5, u8, false> and k_mb_final<8, u8, true> need more than 512 macroblocks in one tick and
are not reached at these sizes.
"""
import numpy as np
import pytest

import deblock_cases as dc
import deblock_ref as dr
from jmpaths import ensure_built, load_jmhip
from test_flow_gpu import env
from test_gpu_parity import moving_seq, run_chain

jmhip = load_jmhip()
pytestmark = pytest.mark.gpu
I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE


@pytest.fixture(scope="module", autouse=True)
def built():
    ensure_built()
    jmhip.load()


def assert_deblocked(dev, rec, res, mbw, mbh, qp, cqo, ab, bd, what):
    """dev == deblock(rec, res); on a difference: the first differing sample, its plane and MB, and the
    bS and branch the reference took there.  Returns (counters, trace)."""
    trace = {}
    ref, cnt = dr.deblock(rec, res, mbw, mbh, qp, cqo, ab[0], ab[1], bd, trace=trace)
    for pl, (d, r) in enumerate(zip(dev, ref)):
        if not np.array_equal(d, r):
            y, x = (int(a) for a in np.argwhere(d != r)[0])
            sub = 16 if pl == 0 else 8
            took = trace.get((pl, y, x))
            took = "bS %d, %s, %s%d of the line" % (took[0], "+".join(took[1]), took[2], took[3]) if took else "no line filtered here"
            pytest.fail(f"{what}: plane {'YUV'[pl]} differs first at row {y}, column {x} (MB x={x // sub}, y={y // sub}, mb_type "
                        f"{res['mb_type'][(y // sub) * mbw + x // sub]}): device {d[y, x]}, reference {r[y, x]} (unfiltered "
                        f"{rec[pl][y, x]}); reference: {took}; {int((d != r).sum())} samples differ in this plane")
    return cnt, trace


def device_chain(enc, pics, qp, cqo, ab, bd, what, idc=0):
    mbw, mbh = enc.mbw, enc.mbh
    records = []
    for i, pic in enumerate(pics):
        if i:
            enc.set_reference_slot(-2)
        res, rec = enc.encode(*pic, P if i else I, qp, cqo, deblock=(idc, ab[0], ab[1]))
        cnt, trace = assert_deblocked(enc.deblocked(), rec, res, mbw, mbh, qp, cqo, ab, bd, f"{what} picture {i}")
        records.append((rec, res, cnt, trace))
    return records


class Route:
    def __init__(self, name, kw=None, env=None, bd=8, flow=False, native=False, slice_rows=False):
        self.name, self.kw, self.env, self.bd, self.flow, self.native, self.slice_rows = name, kw or {}, env or {}, bd, flow, native, slice_rows

    def __repr__(self):
        return self.name

    def encoder(self, w, h, **kw):
        kw.update(self.kw)
        if self.slice_rows:
            kw["slice_mbs"] = w // 16
        with env(**self.env):
            return jmhip.Encoder(w, h, **kw)

    def check_path(self, enc):
        """The launches went where the route says (jmh_timing.flow_launches: k_mb_flow)."""
        t = enc.timing()
        assert (t.flow_launches > 0) == self.flow, (self.name, t.flow_launches)


EPZS = dict(search_mode=3)
ROUTES = [
    Route("flow", flow=True, native=True),
    Route("ticks", env=dict(JMH_FLOW=0), native=True),
    Route("epzs", EPZS),
    Route("t8", dict(transform_8x8_mode=1, **EPZS)),
    Route("rdo_cavlc", dict(rdo=1, symbol_mode=0, **EPZS)),
    Route("rdo_cabac", dict(rdo=1, symbol_mode=1, **EPZS)),
    Route("slice1", dict(slice_mbs=1), flow=True),
    Route("slice5", dict(slice_mbs=5), flow=True),
    Route("slice_row", slice_rows=True, flow=True),
    Route("cip", dict(constrained_intra_pred=1)),
    Route("hbd9", dict(bit_depth=9, **EPZS), bd=9, native=True),
    Route("hbd10", dict(bit_depth=10, **EPZS), bd=10, native=True),
    Route("hbd10_ffs", dict(bit_depth=10, search_mode=0), bd=10),
    Route("rdo_cavlc_10", dict(bit_depth=10, rdo=1, symbol_mode=0, **EPZS), bd=10),
    Route("rdo_cabac_10", dict(bit_depth=10, rdo=1, symbol_mode=1, **EPZS), bd=10),
]


def route_cases():
    for r in ROUTES:
        for c in dc.CASES:
            if c.bd == r.bd and (c.name != "t8_epzs" or r.name == "t8"):
                yield pytest.param(r, c, id=f"{r.name}-{c.name}")


@pytest.mark.parametrize("route,case", list(route_cases()))
def test_cases(route, case):
    enc = route.encoder(case.w, case.h, **case.kw)
    records = device_chain(enc, case.pics(), case.qp, case.cqo, case.ab, case.bd, f"{route.name} {case.name}")
    route.check_path(enc)
    enc.close()
    allc = sum((r[2] for r in records), dr.Counter())
    print(route.name, case.name, dict(sorted(allc.items())))
    if route.native or (route.name == "t8" and case.name == "t8_epzs"):
        dc.check_case(case, records)                 # the decisions are the oracle's: the CPU file's needs hold here too
    elif case.check != "none_filtered":              # other decisions: the case still has to filter
        assert dc.total(allc, "L_filt") > 0 and dc.total(allc, "L_edge_bS3") > 0, dict(allc)


@pytest.mark.parametrize("route", ROUTES, ids=repr)
def test_width_176(route):
    """11 macroblocks per row (no multiple of 8): width-dependent addressing."""
    w, h, qp, ab = 176, 144, 30, (1, -1)
    pics = moving_seq(w, h, 3, 21, (7, -5))
    if route.bd > 8:
        pics = dc.widen(pics, route.bd)
    enc = route.encoder(w, h, search_range=16)
    records = device_chain(enc, pics, qp, 0, ab, route.bd, f"{route.name} 176x144")
    route.check_path(enc)
    enc.close()
    allc = sum((r[2] for r in records), dr.Counter())
    assert allc["L_filt_bS1"] + allc["L_filt_bS2"] > 0 and allc["L_filt_bS3"] > 0 and allc["L_filt_bS4"] > 0, dict(allc)
    assert dc.total(allc, "C_filt") > 0 and dc.total(allc, "L_gated") > 0, dict(allc)


@pytest.mark.parametrize("qp", dc.SWEEP_QPS)
@pytest.mark.parametrize("route", ROUTES, ids=repr)
def test_threshold_sweep(route, qp):
    pics = dc.sweep_pics()
    if route.bd > 8:
        pics = dc.widen(pics, route.bd)
    enc = route.encoder(dc.SWEEP_W, dc.SWEEP_H, search_range=8)
    for cqo in dc.SWEEP_CQO:
        for ab in dc.SWEEP_AB:
            records = device_chain(enc, pics, qp, cqo, ab, route.bd, f"{route.name} QP {qp} {ab} offset {cqo}")
            dc.check_sweep(qp, ab, cqo, sum((r[2] for r in records), dr.Counter()))
    enc.close()


# ---------------- several pictures' macroblocks in one launch ----------------
@pytest.mark.parametrize("kw", [{}, dict(search_mode=3), dict(rdo=1, symbol_mode=1, search_mode=3)], ids=["flow", "epzs", "rdo"])
def test_pipelined_push_pop(kw):
    """Default pipeline depth, 320x240, 6 pictures: each picture's deblocked planes read after its pop."""
    w, h, qp, ab = 320, 240, 32, (0, 0)
    pics = moving_seq(w, h, 6, 31, (11, -7))
    enc = jmhip.Encoder(w, h, search_range=16, **kw)
    assert enc.depth > 1
    out = run_chain(enc, pics, qp, (0,) + ab, pipelined=True)
    enc.close()
    assert len(out) == 6
    allc = dr.Counter()
    for i, (res, rec, dbk) in enumerate(out):
        allc += assert_deblocked(dbk, rec, res, w // 16, h // 16, qp, 0, ab, 8, f"pipelined picture {i}")[0]
    assert allc["L_filt_bS1"] + allc["L_filt_bS2"] > 0 and allc["L_filt_bS3"] > 0 and allc["L_filt_bS4"] > 0, dict(allc)


def test_encode_slot_chain():
    """bench.py's path: encode_slot on device-resident pictures (slots=3), then a read-back picture on
    top of the chain's deblocked reference."""
    w, h, qp, ab = 96, 64, 30, (1, -2)
    pics = moving_seq(w, h, 4, 32, (5, -3))
    enc = jmhip.Encoder(w, h, search_range=8, slots=3)
    for i in range(3):
        enc.load_frame(i, *pics[i])
    enc.encode_slot(0, I, qp, deblock=(0,) + ab)
    for i in (1, 2):
        enc.set_reference_slot(-2)
        enc.encode_slot(i, P, qp, deblock=(0,) + ab)
    enc.set_reference_slot(-2)
    res, rec = enc.encode(*pics[3], P, qp, deblock=(0,) + ab)
    cnt, _ = assert_deblocked(enc.deblocked(), rec, res, w // 16, h // 16, qp, 0, ab, 8, "after the slot chain")
    assert dc.total(cnt, "L_filt") > 0 and (res["mb_type"] != 0).any()
    # the chain itself, picture by picture through the host-copy path, leaves the same last picture
    b = jmhip.Encoder(w, h, search_range=8)
    for i in range(4):
        if i:
            b.set_reference_slot(-2)
        bres, brec = b.encode(*pics[i], P if i else I, qp, deblock=(0,) + ab)
        assert_deblocked(b.deblocked(), brec, bres, w // 16, h // 16, qp, 0, ab, 8, f"sequential picture {i}")
    for x, y in zip(enc.deblocked(), b.deblocked()):
        assert np.array_equal(x, y)
    enc.close()
    b.close()


# ---------------- disable_deblocking_filter_idc ----------------
@pytest.mark.parametrize("kw", [{}, dict(rdo=1, symbol_mode=0, search_mode=3), dict(bit_depth=10, search_mode=3)], ids=["flow", "rdo", "hbd10"])
def test_idc1_copies_the_reconstruction(kw):
    w, h = 96, 64
    pics = moving_seq(w, h, 2, 33, (5, -3))
    if kw.get("bit_depth"):
        pics = dc.widen(pics, 10)
    enc = jmhip.Encoder(w, h, search_range=8, **kw)
    for i, pic in enumerate(pics):
        if i:
            enc.set_reference_slot(-2)
        res, rec = enc.encode(*pic, P if i else I, 36, deblock=(1, 3, 3))
        for d, r in zip(enc.deblocked(), rec):
            assert np.array_equal(d, r)
    enc.close()


@pytest.mark.parametrize("kw", [{}, dict(slice_mbs=24), dict(slice_mbs=100)], ids=["no_slices", "slice_is_picture", "slice_beyond_picture"])
def test_idc2_one_slice_equals_idc0(kw):
    """One slice per picture has no slice edge inside the picture: idc 2 filters what idc 0 does."""
    case = dc.CASES[0]
    enc = jmhip.Encoder(case.w, case.h, **dict(case.kw, **kw))
    records = device_chain(enc, case.pics(), case.qp, 0, case.ab, 8, f"idc 2 {kw}", idc=2)
    enc.close()
    dc.check_case(case, records)


@pytest.mark.parametrize("slice_mbs", [1, 5, 6, 23])
@pytest.mark.parametrize("kw", [{}, dict(rdo=1, symbol_mode=1, search_mode=3)], ids=["flow", "rdo"])
def test_idc2_with_slices_is_rejected(kw, slice_mbs):
    """Several slices per picture: idc 2 would have to leave the slice edges alone, which deblock_mb does
    not do; the picture is refused, by every entry point, and the context stays usable."""
    w, h = 96, 64
    pics = moving_seq(w, h, 1, 34)
    enc = jmhip.Encoder(w, h, search_range=8, slots=2, slice_mbs=slice_mbs, **kw)
    enc.load_frame(0, *pics[0])
    for call in (lambda: enc.encode(*pics[0], I, 30, deblock=(2, 0, 0)), lambda: enc.push(*pics[0], I, 30, deblock=(2, 0, 0)),
                 lambda: enc.encode_slot(0, I, 30, deblock=(2, 0, 0))):
        with pytest.raises(jmhip.JmhError) as e:
            call()
        assert e.value.status == jmhip.JMH_E_UNSUPPORTED_CFG
    # idc 0 and 1 are accepted as before
    res, rec = enc.encode(*pics[0], I, 30, deblock=(0, 0, 0))
    assert_deblocked(enc.deblocked(), rec, res, w // 16, h // 16, 30, 0, (0, 0), 8, "idc 0 after the refusal")
    enc.encode(*pics[0], I, 30, deblock=(1, 0, 0))
    enc.close()
