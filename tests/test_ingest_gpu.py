"""Pictures that are already on the device (include/jmhip_input.h): k_ingest packs
and pads an I420 / NV12 / I010 / P010 picture where a host picture is packed on the CPU and
uploaded.

The reference of the seam is numpy: the source samples (clamped to maxv for I010, as read_hbd of
host/yuv.c does) replicated to the coded size (jmhip.pad_to_coded, jm_pad_picture in numpy).  The
reference of every pipeline case is a second Encoder with the same configuration, fed the same
pictures padded on the host through the ordinary push.  Every check is exact."""
import tempfile

import numpy as np
import pytest

from jmpaths import LENCOD, ensure_built, load_jmhip
from test_gpu_parity import run_lencod

jmhip = load_jmhip()
pytestmark = pytest.mark.gpu

I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE
I420, NV12, I010, P010 = jmhip.JMH_PIX_I420, jmhip.JMH_PIX_NV12, jmhip.JMH_PIX_I010, jmhip.JMH_PIX_P010
NAMES = {I420: "I420", NV12: "NV12", I010: "I010", P010: "P010"}
DBK = (0, 0, 0)
# coded size -> source sizes (tests/test_ingest_core.py runs the same list through the core)
SIZES = {(32, 32): [(32, 32), (18, 18), (30, 2), (2, 30), (2, 2)], (48, 32): [(34, 18)]}


@pytest.fixture(scope="module", autouse=True)
def built():
    ensure_built()


@pytest.fixture(scope="module")
def contexts():
    """one Encoder per (coded size, bit depth), shared by the seam cases"""
    made = {}

    def get(w, h, bd):
        if (w, h, bd) not in made:
            made[(w, h, bd)] = jmhip.Encoder(w, h, search_range=8, bit_depth=bd, pipeline_depth=2)
        return made[(w, h, bd)]
    yield get
    for e in made.values():
        e.close()


def source(rng, w, h, fmt, bd):
    """random samples of the source size over the format's whole range; I010: about one in eight
    above maxv, and 0, maxv, maxv + 1, 65535 in every plane.  Returns (planes, clamped count)."""
    maxv = (1 << bd) - 1
    out, over = [], 0
    for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
        if fmt == I010:
            a = rng.integers(0, maxv + 1, (ph, pw)).astype(np.uint16)
            hot = rng.integers(0, 8, (ph, pw)) == 0
            a[hot] = rng.integers(maxv + 1, 65536, int(hot.sum())).astype(np.uint16)
            flat = a.reshape(-1)
            for k, v in enumerate((0, maxv, maxv + 1, 65535)):
                flat[(flat.size - 1) * k // 3] = v
            over += int((a > maxv).sum())
        else:
            a = rng.integers(0, maxv + 1, (ph, pw)).astype(np.uint16 if bd > 8 else np.uint8)
        out.append(a)
    return tuple(out), over


def expected(pics, fmt, bd, cw, ch):
    maxv = (1 << bd) - 1
    return jmhip.pad_to_coded(tuple(np.minimum(a, maxv).astype(a.dtype) for a in pics), cw, ch)


def ingest_case(enc, rng, fmt, bd, w, h, pad, mis, what):
    pics, over = source(rng, w, h, fmt, bd)
    pic = enc.device_picture(jmhip.to_device(pics, fmt, pad_stride=pad, misalign=mis))
    try:
        got = enc.ingest(pic)
        clamped = enc.input_clamped()
    finally:
        enc.device_free(pic.base)
    for name, a, b in zip("YUV", got, expected(pics, fmt, bd, enc.w, enc.h)):
        assert a.dtype == b.dtype and np.array_equal(a, b), f"{what}: plane {name} differs at {np.argwhere(a != b)[:4].tolist()}"
    assert clamped == over, f"{what}: clamp count"


# ---- the seam -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,bd", [(I420, 8), (NV12, 8), (I010, 9), (I010, 10), (P010, 10)], ids=["I420", "NV12", "I010_9", "I010_10", "P010"])
def test_seam_sizes_strides_misalignments(contexts, fmt, bd):
    """every source size of the CPU list, strides tight / +1 (8-bit) / +2 / +26 (and +4, which makes
    the 30-wide P010 and NV12 rows 16-byte aligned with a straddling vector), plane bases 0..3
    bytes (8-bit) or 0 / 2 bytes (16-bit) off a 256-byte boundary: the 16-byte loads, the dword
    loads with every funnel shift, the straddling vector and the vectors beyond the source"""
    rng = np.random.default_rng(100 + fmt * 16 + bd)
    wide = fmt >= I010
    n = 0
    for (cw, ch), sources in SIZES.items():
        enc = contexts(cw, ch, bd)
        for w, h in sources:
            for pad in ((0, 2, 4, 26) if wide else (0, 1, 2, 4, 26)):
                for mis in ((0, 2) if wide else (0, 1, 2, 3)):
                    ingest_case(enc, rng, fmt, bd, w, h, pad, mis, f"{NAMES[fmt]} {bd} bits {w}x{h} in {cw}x{ch} stride +{pad} base +{mis}")
                    n += 1
    assert n == 6 * (4 * 2 if wide else 5 * 4)


@pytest.mark.parametrize("fmt,bd", [(I420, 8), (NV12, 8), (I010, 10), (P010, 10)], ids=["I420", "NV12", "I010", "P010"])
def test_seam_row_longer_than_a_wave(contexts, fmt, bd):
    """3840x32: a luma row is 240 (8-bit) or 480 (16-bit) vectors, more than the 64 lanes of the wave
    that owns it; from a full-width source (aligned and misaligned) and from a 3826x30 one"""
    rng = np.random.default_rng(7 + fmt)
    enc = contexts(3840, 32, bd)
    for w, h, pad, mis in ((3840, 32, 0, 0), (3840, 32, 2, 2), (3826, 30, 0, 0)):
        ingest_case(enc, rng, fmt, bd, w, h, pad, mis, f"{NAMES[fmt]} {w}x{h} in 3840x32 stride +{pad} base +{mis}")


# ---- the pipeline -------------------------------------------------------------------------------
def seq(w, h, n, seed, bd=8):
    """n source pictures of w x h: a moving smooth texture plus noise, so that P pictures find motion"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h + 4 * n, 0:w + 4 * n]
    big = (128 + 90 * np.sin(xx / 5.0) * np.cos(yy / 7.0)).astype(np.int32)
    out = []
    for i in range(n):
        y = np.clip(big[2 * i:2 * i + h, 3 * i:3 * i + w] + rng.integers(-5, 6, (h, w)), 0, 255).astype(np.uint16)
        u = y[::2, ::2] // 2 + 40
        v = 255 - y[1::2, 1::2]
        if bd > 8:
            pl = tuple(np.ascontiguousarray((p << (bd - 8)) | rng.integers(0, 1 << (bd - 8), p.shape).astype(np.uint16)) for p in (y, u, v))
        else:
            pl = tuple(np.ascontiguousarray(p.astype(np.uint8)) for p in (y, u, v))
        out.append(pl)
    return out


def chain(enc, n, push):
    """IPPP through the pipeline, each P on the previous picture's device deblocking, popping only
    when the pipeline is full; push(i, slice_type).  Per picture (results, recon, deblocked)."""
    out, pending = [], 0

    def pop():
        res, rec = enc.pop()
        out.append((res.tobytes(), rec, enc.deblocked()))
    for i in range(n):
        if i:
            enc.set_reference_slot(-2)
        if pending == enc.depth:
            pop()
            pending -= 1
        push(i, I if i == 0 else P)
        pending += 1
    while pending:
        pop()
        pending -= 1
    return out


def assert_chains_equal(got, want, what):
    assert len(got) == len(want)
    for i, (g, r) in enumerate(zip(got, want)):
        assert g[0] == r[0], f"{what} picture {i}: results"
        for k in (1, 2):
            for a, b in zip(g[k], r[k]):
                assert np.array_equal(a, b), f"{what} picture {i}: {'recon' if k == 1 else 'deblocked'}"


def resident(enc, pics, fmt, pad=2, mis=0):
    """every picture uploaded into its own allocation (complete on return)"""
    return [enc.device_picture(jmhip.to_device(p, fmt, pad_stride=pad, misalign=mis)) for p in pics]


W, H, SW, SH, QP = 64, 48, 50, 38, 28
PIPE = [
    ("ffs_i420", dict(search_range=8), I420),
    ("ffs_nv12", dict(search_range=8), NV12),
    ("epzs_high10_i010", dict(search_range=8, search_mode=3, bit_depth=10, transform_8x8_mode=1), I010),
    ("epzs_high10_p010", dict(search_range=8, search_mode=3, bit_depth=10, transform_8x8_mode=1), P010),
    ("rdo_cabac_nv12", dict(search_range=8, search_mode=3, rdo=1), NV12),
]


@pytest.mark.parametrize("kw,fmt", [c[1:] for c in PIPE], ids=[c[0] for c in PIPE])
def test_pipeline_device_push_equals_host_push(kw, fmt):
    """four pictures of 50x38 in a 64x48 context: push_device of the unpadded source == push of the
    picture padded on the host"""
    bd = kw.get("bit_depth", 8)
    pics = seq(SW, SH, 4, 11 + fmt, bd)
    padded = [jmhip.pad_to_coded(p, W, H) for p in pics]
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    dev = []
    try:
        dev = resident(enc, pics, fmt, pad=2, mis=2)
        got = chain(enc, 4, lambda i, st: enc.push_device(dev[i], st, QP, deblock=DBK))
        want = chain(ref, 4, lambda i, st: ref.push(*padded[i], st, QP, deblock=DBK))
        assert_chains_equal(got, want, NAMES[fmt])
        assert enc.input_clamped() == 0
    finally:
        for d in dev:
            enc.device_free(d.base)
        enc.close()
        ref.close()


def test_pipeline_alternating_host_and_device_pushes():
    """one context takes host pictures (even) and device pictures (odd, NV12 and I420 in turn)"""
    pics = seq(SW, SH, 6, 21)
    padded = [jmhip.pad_to_coded(p, W, H) for p in pics]
    kw = dict(search_range=8)
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    dev = {}
    try:
        for i in (1, 3, 5):
            dev[i] = resident(enc, [pics[i]], NV12 if i == 3 else I420, pad=1, mis=1)[0]
        got = chain(enc, 6, lambda i, st: enc.push_device(dev[i], st, QP, deblock=DBK) if i in dev else enc.push(*padded[i], st, QP, deblock=DBK))
        want = chain(ref, 6, lambda i, st: ref.push(*padded[i], st, QP, deblock=DBK))
        assert_chains_equal(got, want, "alternating")
    finally:
        for d in dev.values():
            enc.device_free(d.base)
        enc.close()
        ref.close()


def test_pipeline_i010_clamp_count_at_the_pop():
    """an I010 picture with samples above maxv through push_device: coded as the clamped picture, the
    count answered for the picture last popped (and 0 again after a host picture)"""
    rng = np.random.default_rng(3)
    kw = dict(search_range=8, search_mode=3, bit_depth=10)
    pics, over = source(rng, SW, SH, I010, 10)
    want_pic = expected(pics, I010, 10, W, H)
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    dev = []
    try:
        dev = resident(enc, [pics], I010)
        enc.push_device(dev[0], I, QP)
        res, rec = enc.pop()
        assert over > 0 and enc.input_clamped() == over
        ref.push(*want_pic, I, QP)
        rres, rrec = ref.pop()
        assert res.tobytes() == rres.tobytes() and all(np.array_equal(a, b) for a, b in zip(rec, rrec))
        enc.push(*want_pic, I, QP)
        enc.pop()
        assert enc.input_clamped() == 0
    finally:
        for d in dev:
            enc.device_free(d.base)
        enc.close()
        ref.close()


# ---- coded pictures -----------------------------------------------------------------------------
def coded_chain(enc, n, push, step):
    out, pending = [], 0
    for i in range(n):
        if i:
            enc.set_reference_slot(-2)
        if pending == enc.depth:
            out.append(enc.pop_coded())
            pending -= 1
        push(i, I if i == 0 else P, jmhip.coded_slice_descs(enc.mbw * enc.mbh, I if i == 0 else P, QP, step, lead=[(3, 0b101), (0, 0)]))
        pending += 1
    while pending:
        out.append(enc.pop_coded())
        pending -= 1
    return out


@pytest.mark.parametrize("kw,fmt,split", [
    (dict(search_range=8, slice_mbs=5), NV12, 0),
    (dict(search_range=8, search_mode=3, rdo=1, slice_mbs=5), I420, 1024),
], ids=["cavlc_nv12", "cabac_split_i420"])
def test_coded_device_push_equals_coded_host_push(kw, fmt, split):
    """push_coded_device / pop_coded == push_coded / pop_coded with the crop at the source size:
    the bytes of every slice, every where field, the SSDs, fallback"""
    pics = seq(SW, SH, 4, 31 + fmt)
    padded = [jmhip.pad_to_coded(p, W, H) for p in pics]
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    dev = []
    try:
        if split:
            enc.cabac_split(split)
            ref.cabac_split(split)
        dev = resident(enc, pics, fmt)
        got = coded_chain(enc, 4, lambda i, st, d: enc.push_coded_device(dev[i], st, QP, d, crop=(SW, SH), deblock=DBK), 5)
        want = coded_chain(ref, 4, lambda i, st, d: ref.push_coded(*padded[i], st, QP, d, crop=(SW, SH), deblock=DBK), 5)
        assert len(got) == len(want) == 4
        for i, ((data, where, stats), (rdata, rwhere, rstats)) in enumerate(zip(got, want)):
            assert len(data) == len(rdata) == 3 and data == rdata, f"picture {i}: slice bytes"
            assert where == rwhere, f"picture {i}: where"
            assert stats == rstats and stats["fallback"] == 0, f"picture {i}: {stats} vs {rstats}"
    finally:
        for d in dev:
            enc.device_free(d.base)
        enc.close()
        ref.close()


# ---- ordering -----------------------------------------------------------------------------------
@pytest.mark.parametrize("use_stream", [True, False], ids=["caller_stream", "null_stream_and_wait"])
def test_one_device_buffer_reused_for_every_picture(use_stream):
    """Picture i is uploaded into the one buffer and pushed; picture i + 1 is uploaded into the same
    buffer at once.  With a caller stream the upload and the push name it (the library makes the
    stream wait for the packing kernel); with stream NULL the host waits (input_wait) before each
    overwrite.  Six pictures (more than the pipeline holds at once where the depth is below six)."""
    n = 6
    pics = seq(SW, SH, n, 41)
    padded = [jmhip.pad_to_coded(p, W, H) for p in pics]
    kw = dict(search_range=8)
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    layouts = [jmhip.to_device(p, NV12, pad_stride=6) for p in pics]
    base = stream = None
    try:
        base = enc.device_alloc(max(L.buf.nbytes for L in layouts))
        stream = enc.device_stream() if use_stream else None
        enc.device_upload(base, layouts[0].buf, stream)

        def push(i, st):
            enc.push_device(layouts[i].at(base, stream), st, QP, deblock=DBK)
            if i + 1 < n:
                if not use_stream:
                    enc.input_wait()
                enc.device_upload(base, layouts[i + 1].buf, stream)
        got = chain(enc, n, push)
        want = chain(ref, n, lambda i, st: ref.push(*padded[i], st, QP, deblock=DBK))
        assert_chains_equal(got, want, "reused buffer")
    finally:
        if stream:
            enc.device_stream_destroy(stream)
        if base:
            enc.device_free(base)
        enc.close()
        ref.close()


# ---- protocol -----------------------------------------------------------------------------------
def test_rejections_leave_the_context_usable():
    pics = seq(SW, SH, 1, 51)
    padded = jmhip.pad_to_coded(pics[0], W, H)
    enc, ref = jmhip.Encoder(W, H, search_range=8, pipeline_depth=2), jmhip.Encoder(W, H, search_range=8, pipeline_depth=2)
    good = None
    try:
        good = resident(enc, pics, I420)[0]

        def status(**change):
            pic = jmhip.DevicePicture(good.format, good.width, good.height, good.planes, good.strides)
            for k, v in change.items():
                setattr(pic, k, v)
            with pytest.raises(jmhip.JmhError) as e:
                enc.push_device(pic, I, QP)
            return e.value.status
        # wrong format for the bit depth (with strides and addresses that pass the format's argument rules)
        assert status(format=P010, strides=[2 * SW + 2, 2 * SW + 2, 0]) == jmhip.JMH_E_UNSUPPORTED_CFG
        assert status(format=I010, strides=[2 * SW + 2, SW + 2, SW + 2]) == jmhip.JMH_E_UNSUPPORTED_CFG
        assert status(format=4) == jmhip.JMH_E_INVALID_ARG
        assert status(width=SW - 1) == jmhip.JMH_E_INVALID_ARG                       # odd
        assert status(height=SH + 1) == jmhip.JMH_E_INVALID_ARG
        assert status(width=W + 2) == jmhip.JMH_E_INVALID_ARG                        # beyond the coded size
        assert status(height=0) == jmhip.JMH_E_INVALID_ARG
        assert status(strides=[SW - 1, SW // 2, SW // 2]) == jmhip.JMH_E_INVALID_ARG   # short strides
        assert status(strides=[SW, SW // 2, SW // 2 - 1]) == jmhip.JMH_E_INVALID_ARG
        assert status(format=NV12, strides=[SW, SW - 1, 0]) == jmhip.JMH_E_INVALID_ARG
        # an odd 16-bit address or stride: an argument error, before the format is held against the bit depth
        assert status(format=I010, planes=[good.planes[0], good.planes[1] + 1, good.planes[2]], strides=[2 * SW + 2, SW + 2, SW + 2]) == jmhip.JMH_E_INVALID_ARG
        assert status(format=I010, strides=[2 * SW + 1, SW + 2, SW + 2]) == jmhip.JMH_E_INVALID_ARG
        assert status(planes=[good.planes[0], None, good.planes[2]]) == jmhip.JMH_E_INVALID_ARG   # a null plane
        assert status(planes=[good.planes[0], good.planes[1], None]) == jmhip.JMH_E_INVALID_ARG
        # nothing was claimed or queued: the pipeline takes its full depth, and one push more is refused
        assert enc.depth == 2
        enc.push_device(good, I, QP, deblock=DBK)
        enc.push_device(good, I, QP, deblock=DBK)
        with pytest.raises(jmhip.JmhError) as e:
            enc.push_device(good, I, QP, deblock=DBK)
        assert e.value.status == jmhip.JMH_E_STATE
        ref.push(*padded, I, QP, deblock=DBK)
        rres, rrec = ref.pop()
        for _ in range(2):
            res, rec = enc.pop()
            assert res.tobytes() == rres.tobytes() and all(np.array_equal(a, b) for a, b in zip(rec, rrec))
        enc.push_device(good, I, QP, deblock=DBK)                                     # and a good push follows
        res, rec = enc.pop()
        assert res.tobytes() == rres.tobytes()
    finally:
        if good:
            enc.device_free(good.base)
        enc.close()
        ref.close()


# ---- lencod -------------------------------------------------------------------------------------
LENCOD_CASES = [
    ["InputFile=synthetic:41", "FramesToBeEncoded=3", "SourceWidth=162", "SourceHeight=130", "SearchRange=16", "DeviceCAVLC=1"],
    ["InputFile=synthetic:42", "FramesToBeEncoded=3", "SourceWidth=176", "SourceHeight=144", "SearchRange=16"],
    ["InputFile=synthetic:43", "FramesToBeEncoded=3", "SourceWidth=162", "SourceHeight=130", "SearchRange=16", "ProfileIDC=110",
     "SourceBitDepthLuma=10", "SourceBitDepthChroma=10", "SearchMode=3", "RDOptimization=1", "SymbolMode=1", "DeviceCABAC=1",
     "DeviceWriterAsync=1"],
]


@pytest.mark.parametrize("extra", LENCOD_CASES, ids=["cavlc_162x130", "cavlc_176x144", "cabac_high10_async_162x130"])
def test_lencod_device_input_identical(extra):
    """DeviceInput=1 writes the same .264 and recon file and prints the same picture lines but for their times"""
    from test_coded_gpu import picture_columns
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        la = run_lencod(LENCOD, a, extra + ["DeviceInput=1"])
        assert "pushed from device memory" in la
        lb = run_lencod(LENCOD, b, extra)
        assert "pushed from device memory" not in lb
        assert open(f"{a}/a.264", "rb").read() == open(f"{b}/a.264", "rb").read()
        assert open(f"{a}/rec.yuv", "rb").read() == open(f"{b}/rec.yuv", "rb").read()
        ca, cb = picture_columns(la), picture_columns(lb)
        assert len(ca) == 3 and ca == cb
