"""4:2:2 and 4:4:4 pictures pushed from the device (include/jmhip_yuv.h): k_ingest_yuv
reduces the chroma of a planar, semi-planar or packed picture to 4:2:0, packs and pads it where
k_ingest moves a 4:2:0 one.

The reference of the seam is numpy: jmhip.yuv_reduce (the formulas of the header in exact integers;
tests/test_yuv_core.py checks it against hand-computed cases) and jmhip.pad_to_coded.  The reference
of every pipeline case is a second Encoder with the same configuration, fed the reduced pictures
padded on the host through the ordinary push.  Every check is exact.

Coded 64x48 from 50x34: padding on both axes and an odd chroma width of 25, so every row has whole
vectors, a straddling one and vectors beyond the source."""
import tempfile

import numpy as np
import pytest

import scale_ref as sr
from jmpaths import LENCOD, ensure_built, load_jmhip
from test_gpu_parity import run_lencod
from test_ingest_gpu import assert_chains_equal, chain, coded_chain, seq

jmhip = load_jmhip()
pytestmark = pytest.mark.gpu

I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE
LEFT = jmhip.JMH_PIX_CHROMA_LEFT
INVALID, UNSUPPORTED = jmhip.JMH_E_INVALID_ARG, jmhip.JMH_E_UNSUPPORTED_CFG
NAMES = {jmhip.JMH_PIX_I422: "I422", jmhip.JMH_PIX_NV16: "NV16", jmhip.JMH_PIX_YUYV: "YUYV", jmhip.JMH_PIX_UYVY: "UYVY", jmhip.JMH_PIX_I444: "I444",
         jmhip.JMH_PIX_VUYA8: "VUYA8", jmhip.JMH_PIX_I210: "I210", jmhip.JMH_PIX_P210: "P210", jmhip.JMH_PIX_Y210: "Y210", jmhip.JMH_PIX_I410: "I410",
         jmhip.JMH_PIX_Y410: "Y410"}
I422, NV16, YUYV, UYVY, I444, VUYA8, I210, P210, Y210, I410, Y410 = NAMES
BYTES, WORDS, DWORDS = (I422, NV16, YUYV, UYVY, I444), (I210, P210, Y210, I410), (VUYA8, Y410)
CLAMPS = (I210, I410)
# every format, the 4:4:4 ones at both sitings
VARIANTS = [f for fmt in NAMES for f in ((fmt, fmt | LEFT) if fmt in jmhip.YUV_444 else (fmt,))]
DBK = (0, 0, 0)
W, H, SW, SH, QP = 64, 48, 50, 34, 28


def name(fmt):
    return NAMES[fmt & ~LEFT] + ("_left" if fmt & LEFT else "")


def depth(fmt):
    return 10 if (fmt & ~LEFT) >= I210 else 8


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
    """random planar samples of the format's shape over its whole range; I210 / I410: about one in
    eight above maxv, and 0, maxv, maxv + 1, 65535 in every plane.  Returns (planes, clamped count)."""
    layout = fmt & ~LEFT
    maxv = (1 << bd) - 1
    cw = w if layout in jmhip.YUV_444 else w // 2
    out, over = [], 0
    for pw in (w, cw, cw):
        a = rng.integers(0, maxv + 1, (h, pw)).astype(np.uint16 if bd > 8 else np.uint8)
        if layout in CLAMPS:
            hot = rng.integers(0, 8, (h, pw)) == 0
            a[hot] = rng.integers(maxv + 1, 65536, int(hot.sum())).astype(np.uint16)
            flat = a.reshape(-1)
            for k, v in enumerate((0, maxv, maxv + 1, 65535)):
                flat[(flat.size - 1) * k // 3] = v
            over += int((a > maxv).sum())
        out.append(a)
    return tuple(out), over


def expected(pics, fmt, bd, cw, ch):
    return jmhip.pad_to_coded(jmhip.yuv_reduce(*pics, fmt, bd), cw, ch)


def assert_planes(got, want, what):
    for pl, a, b in zip("YUV", got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: plane {pl} {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
        assert np.array_equal(a, b), f"{what}: plane {pl} differs at {np.argwhere(a != b)[:4].tolist()}"


def ingest_case(enc, rng, fmt, bd, w, h, pad, mis, what):
    pics, over = source(rng, w, h, fmt, bd)
    pic = enc.device_picture(jmhip.to_device_yuv(pics, fmt, pad_stride=pad, misalign=mis))
    try:
        got = enc.ingest(pic)
        clamped = enc.input_clamped()
    finally:
        enc.device_free(pic.base)
    assert_planes(got, expected(pics, fmt, bd, enc.w, enc.h), what)
    assert clamped == over, f"{what}: clamp count {clamped}, {over} source samples above maxv"


def misalignments(fmt):
    layout = fmt & ~LEFT
    return (0, 1, 2, 3) if layout in BYTES else (0, 2) if layout in WORDS else (0, 4)


# ---- 1: the seam --------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", VARIANTS, ids=[name(f) for f in VARIANTS])
def test_seam_sizes_strides_misalignments(contexts, fmt):
    """50x34 and 2x2 (chroma 1x1) in 64x48; strides tight and +28; plane bases off a 256-byte boundary
    by every amount the format's words allow: the 16-byte loads, the dword loads with every funnel
    shift, the straddling vector and the vectors beyond the source; random samples over the whole
    range"""
    bd = depth(fmt)
    rng = np.random.default_rng(300 + fmt)
    enc = contexts(W, H, bd)
    for w, h in ((SW, SH), (2, 2)):
        for pad in (0, 28):
            for mis in misalignments(fmt):
                ingest_case(enc, rng, fmt, bd, w, h, pad, mis, f"{name(fmt)} {w}x{h} in {W}x{H} stride +{pad} base +{mis}")


@pytest.mark.parametrize("fmt", [NV16, UYVY, VUYA8 | LEFT, I210, Y210, Y410 | LEFT], ids=["NV16", "UYVY", "VUYA8_left", "I210", "Y210", "Y410_left"])
def test_seam_row_longer_than_a_wave(contexts, fmt):
    """2080x32: a chroma row is 65 (8-bit) or 130 (16-bit) vectors, more than the 64 lanes of the wave
    that owns it, so a lane takes a second step (and its left neighbour from the step before); from a
    full-width source, aligned and not, and from a 2066x30 one"""
    bd = depth(fmt)
    rng = np.random.default_rng(7 + fmt)
    enc = contexts(2080, 32, bd)
    mis = misalignments(fmt)[1]
    for w, h, pad, m in ((2080, 32, 0, 0), (2080, 32, 4, mis), (2066, 30, 0, 0)):
        ingest_case(enc, rng, fmt, bd, w, h, pad, m, f"{name(fmt)} {w}x{h} in 2080x32 stride +{pad} base +{m}")


# ---- 2: the clamp count -------------------------------------------------------------------------
@pytest.mark.parametrize("bd", (9, 10))
@pytest.mark.parametrize("fmt", [I210, I410, I410 | LEFT], ids=["I210", "I410", "I410_left"])
def test_clamp_count_is_the_numpy_count(contexts, fmt, bd):
    """samples above maxv of the source, luma and both chroma planes, each once: not the padding's
    replicas, not the left neighbours read a second time"""
    rng = np.random.default_rng(40 + fmt + bd)
    enc = contexts(W, H, bd)
    pics, over = source(rng, SW, SH, fmt, bd)
    assert over == sum(int((a > (1 << bd) - 1).sum()) for a in pics) and over > 100
    pic = enc.device_picture(jmhip.to_device_yuv(pics, fmt, pad_stride=4))
    try:
        got = enc.ingest(pic)
        assert enc.input_clamped() == over
        assert_planes(got, expected(pics, fmt, bd, W, H), f"{name(fmt)} {bd} bits")
        # and at the pop of a pushed picture; 0 again after a format that does not count
        enc.push_device(pic, I, QP)
        enc.pop()
        assert enc.input_clamped() == over
        enc.push(*expected(pics, fmt, bd, W, H), I, QP)
        enc.pop()
        assert enc.input_clamped() == 0
    finally:
        enc.device_free(pic.base)


# ---- 3: the pipeline ----------------------------------------------------------------------------
def seq_yuv(w, h, n, seed, fmt, bd=8):
    """n moving pictures with chroma of the format's shape that is no replication of a 4:2:0 plane"""
    out = []
    maxv = (1 << bd) - 1
    for y, _, _ in seq(w, h, n, seed, bd):
        u = (y.astype(np.int32) // 2 + (40 << (bd - 8))).astype(y.dtype)
        v = (maxv - np.roll(y, 1, axis=1).astype(np.int32)).astype(y.dtype)
        if (fmt & ~LEFT) not in jmhip.YUV_444:
            u, v = np.ascontiguousarray(u[:, ::2]), np.ascontiguousarray(v[:, 1::2])
        out.append((y, u, v))
    return out


def resident_yuv(enc, pics, fmt, pad=4, mis=0):
    return [enc.device_picture(jmhip.to_device_yuv(p, fmt, pad_stride=pad, misalign=mis)) for p in pics]


PIPE = [
    ("uyvy", dict(search_range=8), UYVY),
    ("i444", dict(search_range=8), I444),
    ("y210_high10_epzs", dict(search_range=8, search_mode=3, bit_depth=10, transform_8x8_mode=1), Y210),
]


@pytest.mark.parametrize("kw,fmt", [c[1:] for c in PIPE], ids=[c[0] for c in PIPE])
def test_pipeline_device_push_equals_host_push_of_the_reduced_picture(kw, fmt):
    """I + P + P of 50x34 in a 64x48 context: push_device of the source == push of the numpy-reduced
    picture padded on the host, results and reconstructions"""
    bd = kw.get("bit_depth", 8)
    pics = seq_yuv(SW, SH, 3, 11 + fmt, fmt, bd)
    padded = [expected(p, fmt, bd, W, H) for p in pics]
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    dev = []
    try:
        dev = resident_yuv(enc, pics, fmt)
        got = chain(enc, 3, lambda i, st: enc.push_device(dev[i], st, QP, deblock=DBK))
        want = chain(ref, 3, lambda i, st: ref.push(*padded[i], st, QP, deblock=DBK))
        assert_chains_equal(got, want, name(fmt))
        assert enc.input_clamped() == 0
    finally:
        for d in dev:
            enc.device_free(d.base)
        enc.close()
        ref.close()


def test_coded_device_push_equals_coded_host_push_of_the_reduced_picture():
    """push_coded_device of UYVY / pop_coded == push_coded of the reduced picture / pop_coded with the
    crop at the source size: the bytes of every slice, every where field, the SSDs"""
    kw = dict(search_range=8, slice_mbs=5)
    pics = seq_yuv(SW, SH, 3, 31, UYVY)
    padded = [expected(p, UYVY, 8, W, H) for p in pics]
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    dev = []
    try:
        dev = resident_yuv(enc, pics, UYVY)
        got = coded_chain(enc, 3, lambda i, st, d: enc.push_coded_device(dev[i], st, QP, d, crop=(SW, SH), deblock=DBK), 5)
        want = coded_chain(ref, 3, lambda i, st, d: ref.push_coded(*padded[i], st, QP, d, crop=(SW, SH), deblock=DBK), 5)
        assert len(got) == len(want) == 3
        for i, ((data, where, stats), (rdata, rwhere, rstats)) in enumerate(zip(got, want)):
            assert len(data) == len(rdata) == 3 and data == rdata, f"picture {i}: slice bytes"
            assert where == rwhere, f"picture {i}: where"
            assert stats == rstats and stats["fallback"] == 0, f"picture {i}: {stats} vs {rstats}"
    finally:
        for d in dev:
            enc.device_free(d.base)
        enc.close()
        ref.close()


# ---- 4: the identity ----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [I422, I444], ids=["I422", "I444"])
def test_replicated_420_chroma_gives_the_420_push(fmt):
    """an I422 / centred I444 source whose chroma planes replicate an I420 picture's: the chain of
    its device pushes is the chain of the I420 device pushes"""
    pics = seq(SW, SH, 3, 61 + fmt)
    rep = (lambda c: c.repeat(2, 0).repeat(2, 1)) if fmt == I444 else (lambda c: c.repeat(2, 0))
    kw = dict(search_range=8)
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    dev, dev420 = [], []
    try:
        dev = resident_yuv(enc, [(y, rep(u), rep(v)) for y, u, v in pics], fmt)
        dev420 = [ref.device_picture(jmhip.to_device(p, jmhip.JMH_PIX_I420, pad_stride=2)) for p in pics]
        got = chain(enc, 3, lambda i, st: enc.push_device(dev[i], st, QP, deblock=DBK))
        want = chain(ref, 3, lambda i, st: ref.push_device(dev420[i], st, QP, deblock=DBK))
        assert_chains_equal(got, want, name(fmt))
    finally:
        for d in dev:
            enc.device_free(d.base)
        for d in dev420:
            ref.device_free(d.base)
        enc.close()
        ref.close()


# ---- 5: with a scale ----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [YUYV, VUYA8], ids=["YUYV", "VUYA8"])
def test_scaled_ingest_is_the_scaler_on_the_reduced_picture(contexts, fmt):
    """100x68, beyond the coded size, reduced at its own size and then resampled to 50x34 (bicubic) and
    padded to 64x48: the numpy scaler of tests/scale_ref.py on the library's taps applied to
    yuv_reduce of the source"""
    rng = np.random.default_rng(70 + fmt)
    enc = contexts(W, H, 8)
    pics, _ = source(rng, 100, 68, fmt, 8)
    want, _ = sr.scale_picture(jmhip.yuv_reduce(*pics, fmt, 8), SW, SH, W, H, jmhip.JMH_SCALE_BICUBIC, False, 8, jmhip.scale_taps)
    enc.input_scale(SW, SH, jmhip.JMH_SCALE_BICUBIC)
    pic = None
    try:
        pic = enc.device_picture(jmhip.to_device_yuv(pics, fmt, pad_stride=4))
        got = enc.ingest(pic)
    finally:
        enc.input_scale(None)
        if pic:
            enc.device_free(pic.base)
    assert_planes(got, want, f"{name(fmt)} 100x68 to 50x34")


# ---- 6: protocol --------------------------------------------------------------------------------
def test_rejections_leave_the_context_usable():
    pics = seq_yuv(SW, SH, 1, 51, I444)
    padded = expected(pics[0], I444, 8, W, H)
    enc, ref = jmhip.Encoder(W, H, search_range=8, pipeline_depth=2), jmhip.Encoder(W, H, search_range=8, pipeline_depth=2)
    good = None
    try:
        good = resident_yuv(enc, pics, I444, pad=14)[0]              # three planes, strides of 64: room for every layout below
        assert good.strides == [64, 64, 64]
        p0, p1, p2 = good.planes

        def status(**change):
            pic = jmhip.DevicePicture(good.format, good.width, good.height, good.planes, good.strides)
            for k, v in change.items():
                setattr(pic, k, v)
            with pytest.raises(jmhip.JmhError) as e:
                enc.push_device(pic, I, QP)
            return e.value.status
        # each format against the wrong bit depth (the arguments pass the format's own rules): the 16-bit ones in this 8-bit context
        w16 = 16                                                         # a width whose rows fit a stride of 64 in every layout
        for fmt in (I210, P210, Y210, I410, Y410, I410 | LEFT):
            assert status(format=fmt, width=w16) == UNSUPPORTED, name(fmt)
        e10 = jmhip.Encoder(W, H, search_range=8, bit_depth=10)
        e9 = jmhip.Encoder(W, H, search_range=8, bit_depth=9)
        try:
            for other, fmts in ((e10, (I422, NV16, YUYV, UYVY, I444, VUYA8, VUYA8 | LEFT)), (e9, (I422, UYVY, VUYA8, P210, Y210, Y410))):
                base = other.device_alloc(64 * SH * 3)
                try:
                    for fmt in fmts:
                        pic = jmhip.DevicePicture(fmt, w16, SH, [base, base + 64 * SH, base + 128 * SH], [64, 64, 64])
                        with pytest.raises(jmhip.JmhError) as e:
                            other.push_device(pic, I, QP)
                        assert e.value.status == UNSUPPORTED, name(fmt)
                finally:
                    other.device_free(base)
        finally:
            e10.close()
            e9.close()
        # short strides
        assert status(strides=[SW - 1, SW, SW]) == INVALID
        assert status(strides=[SW, SW, SW - 1]) == INVALID                                     # I444: full-size chroma rows
        assert status(format=I422, strides=[SW, SW // 2 - 1, SW // 2]) == INVALID
        assert status(format=NV16, strides=[SW, SW - 1, 0]) == INVALID
        assert status(format=YUYV, width=34, strides=[64, 0, 0]) == INVALID                    # 2 * 34 > 64
        assert status(format=UYVY, width=34, strides=[67, 0, 0]) == INVALID
        assert status(format=VUYA8, width=18, strides=[64, 0, 0]) == INVALID                   # 4 * 18 > 64
        assert status(format=Y210, width=18, strides=[64, 0, 0]) == INVALID
        assert status(format=Y410, width=18, strides=[64, 0, 0]) == INVALID
        assert status(format=I210, width=34, strides=[64, 64, 64]) == INVALID
        assert status(format=I410, width=w16, strides=[64, 30, 64]) == INVALID
        # an odd 16-bit address or stride, a dword format that is not dword aligned: argument errors, before the bit depth
        assert status(format=I210, width=w16, planes=[p0, p1 + 1, p2]) == INVALID
        assert status(format=P210, width=w16, planes=[p0 + 1, p1, None]) == INVALID
        assert status(format=Y210, width=w16, planes=[p0 + 1, None, None]) == INVALID
        assert status(format=Y210, width=8, strides=[63, 0, 0]) == INVALID
        assert status(format=I410, width=w16, strides=[64, 64, 63]) == INVALID
        assert status(format=VUYA8, width=8, planes=[p0 + 2, None, None]) == INVALID
        assert status(format=VUYA8, width=8, planes=[p0 + 1, None, None]) == INVALID
        assert status(format=VUYA8, width=8, strides=[62, 0, 0]) == INVALID
        assert status(format=Y410, width=8, planes=[p0 + 2, None, None]) == INVALID
        assert status(format=Y410, width=8, strides=[66, 0, 0]) == INVALID
        # a null plane that the format reads
        assert status(planes=[p0, None, p2]) == INVALID
        assert status(planes=[p0, p1, None]) == INVALID
        assert status(planes=[None, p1, p2]) == INVALID
        assert status(format=I422, planes=[p0, p1, None]) == INVALID
        assert status(format=NV16, planes=[p0, None, p2]) == INVALID
        assert status(format=UYVY, width=w16, planes=[None, p1, p2]) == INVALID
        # the size rules
        assert status(width=SW - 1) == INVALID and status(height=SH + 1) == INVALID and status(height=0) == INVALID
        assert status(width=W + 2, strides=[128, 128, 128]) == INVALID and status(height=H + 2) == INVALID
        # the flag on the older formats, the other flags on the new ones, the codes between the ranges
        i420 = dict(planes=[p0, p1, p2], strides=[64, 64, 64])
        assert status(format=jmhip.JMH_PIX_I420 | LEFT, **i420) == INVALID
        assert status(format=jmhip.JMH_PIX_NV12 | LEFT, **i420) == INVALID
        assert status(format=jmhip.JMH_PIX_BGRA8 | LEFT, width=w16) == INVALID
        assert status(format=I444 | jmhip.JMH_PIX_BT709) == INVALID and status(format=UYVY | jmhip.JMH_PIX_FULL_RANGE, width=w16) == INVALID
        assert status(format=I444 | 1 << 11) == INVALID
        for code in (4, 15, 20, 31, 38, 39, 45, 63):
            assert status(format=code) == INVALID and status(format=code | LEFT) == INVALID, code
        # the 4:2:2 formats take the flag (no effect)
        pic = jmhip.DevicePicture(I422 | LEFT, SW, SH, good.planes, good.strides)
        plain = jmhip.DevicePicture(I422, SW, SH, good.planes, good.strides)
        assert_planes(enc.ingest(pic), enc.ingest(plain), "I422 with the flag")
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


# ---- 7: ordering --------------------------------------------------------------------------------
def test_one_device_buffer_reused_on_the_callers_stream():
    """Picture i is uploaded into the one buffer on a caller stream and pushed with that stream in the
    picture; picture i + 1 is uploaded into the same buffer at once (the library makes the stream
    wait for the packing kernel).  Equal to the chain of separate buffers."""
    n = 5
    pics = seq_yuv(SW, SH, n, 41, YUYV)
    kw = dict(search_range=8)
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    layouts = [jmhip.to_device_yuv(p, YUYV, pad_stride=8) for p in pics]
    base = stream = None
    dev = []
    try:
        base = enc.device_alloc(max(L.buf.nbytes for L in layouts))
        stream = enc.device_stream()
        enc.device_upload(base, layouts[0].buf, stream)

        def push(i, st):
            enc.push_device(layouts[i].at(base, stream), st, QP, deblock=DBK)
            if i + 1 < n:
                enc.device_upload(base, layouts[i + 1].buf, stream)
        got = chain(enc, n, push)
        dev = resident_yuv(ref, pics, YUYV)
        want = chain(ref, n, lambda i, st: ref.push_device(dev[i], st, QP, deblock=DBK))
        assert_chains_equal(got, want, "reused buffer")
    finally:
        if stream:
            enc.device_stream_destroy(stream)
        if base:
            enc.device_free(base)
        for d in dev:
            ref.device_free(d.base)
        enc.close()
        ref.close()


# ---- 8: lencod ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,w,h,keys", [(UYVY, 64, 48, ["DeviceInputYUV=35"]), (I444 | LEFT, 50, 34, ["DeviceInputYUV=36", "DeviceInputChromaLeft=1"])],
                         ids=["uyvy_64x48", "i444_left_50x34"])
def test_lencod_device_input_yuv_identical(fmt, w, h, keys):
    """3 frames from a file in the layout with DeviceInputYUV == the numpy-reduced I420 file with
    DeviceInput=1 alone: the same .264, every other key the same"""
    pics = seq_yuv(w, h, 3, 81, fmt)
    common = ["FramesToBeEncoded=3", f"SourceWidth={w}", f"SourceHeight={h}", "SearchRange=8", "DeviceCAVLC=1", "DeviceWriterAsync=1", "DeviceInput=1"]
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        with open(f"{a}/in.raw", "wb") as f:
            for p in pics:
                L = jmhip.to_device_yuv(p, fmt)
                planes = [L.buf[o:o + h * st] for o, st in zip(L.offsets, L.strides)]      # tight rows: a plane is one block
                f.write(b"".join(x.tobytes() for x in planes))
        with open(f"{b}/in.yuv", "wb") as f:
            for p in pics:
                f.write(b"".join(x.tobytes() for x in jmhip.yuv_reduce(*p, fmt, 8)))
        la = run_lencod(LENCOD, a, common + keys + [f"InputFile={a}/in.raw"])
        assert "reduced to 4:2:0 on the device" in la and ("left-sited" in la) == bool(fmt & LEFT)
        lb = run_lencod(LENCOD, b, common + [f"InputFile={b}/in.yuv"])
        assert "reduced to 4:2:0" not in lb
        sa, sb = open(f"{a}/a.264", "rb").read(), open(f"{b}/a.264", "rb").read()
        assert len(sa) > 100 and sa == sb
        assert open(f"{a}/rec.yuv", "rb").read() == open(f"{b}/rec.yuv", "rb").read()
