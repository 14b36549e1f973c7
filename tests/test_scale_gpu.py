"""Device pushes scaled to a chosen size (include/jmhip_scale.h): with a scale set the
ingest kernel packs the source at its own size and k_scale resamples that into the coded picture.

The reference is tests/scale_ref.py: the header's two integer passes and the padding in numpy, on the
tables jmh_scale_taps returns (tests/test_scale_core.py holds those against float64).  The reference of
every pipeline case is the same context, or a second one, fed the reference picture with the setting
off.  Every check is exact."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import rgb_ref
import scale_ref as sr
import tensor_ref as tr
from jmpaths import LENCOD, ensure_built, load_jmhip
from test_gpu_parity import run_lencod
from test_ingest_gpu import coded_chain, resident, seq

jmhip = load_jmhip()
pytestmark = pytest.mark.gpu

I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE
I420, NV12, I010, P010 = jmhip.JMH_PIX_I420, jmhip.JMH_PIX_NV12, jmhip.JMH_PIX_I010, jmhip.JMH_PIX_P010
BGRA8 = jmhip.JMH_PIX_BGRA8
INVALID, UNSUPPORTED = jmhip.JMH_E_INVALID_ARG, jmhip.JMH_E_UNSUPPORTED_CFG
DBK = (0, 0, 0)
QP = 28


@pytest.fixture(scope="module", autouse=True)
def built():
    ensure_built()


@pytest.fixture(scope="module")
def contexts():
    """one Encoder per (coded size, bit depth), shared by the seam cases; every case sets its own scale"""
    made = {}

    def get(w, h, bd):
        if (w, h, bd) not in made:
            made[(w, h, bd)] = jmhip.Encoder(w, h, search_range=8, bit_depth=bd, pipeline_depth=2)
        return made[(w, h, bd)]
    yield get
    for e in made.values():
        e.close()


@functools.lru_cache(maxsize=None)
def taps(n_src, n_dst, filter, left):
    return jmhip.scale_taps(n_src, n_dst, filter, left)


def reference(pics, ow, oh, W, H, filter, left, bd):
    return sr.scale_picture(pics, ow, oh, W, H, filter, left, bd, taps)


def assert_planes(got, want, what):
    for name, a, b in zip("YUV", got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: plane {name} {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
        assert np.array_equal(a, b), f"{what}: plane {name} differs at {np.argwhere(a != b)[:4].tolist()}"


def scaled_ingest(enc, pics, fmt, case, pad=0, mis=0):
    W, H, w, h, ow, oh, filter, left = case
    enc.input_scale(ow, oh, filter, left)
    pic = enc.device_picture(jmhip.to_device(pics, fmt, pad_stride=pad, misalign=mis))
    try:
        return enc.ingest(pic)
    finally:
        enc.device_free(pic.base)
        enc.input_scale(None)


# ---- 1: the seam --------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("case", sr.CASES, ids=[sr.case_id(c) for c in sr.CASES])
def test_seam_equals_reference(contexts, case, bd):
    """enc.ingest of an I420 (8 bits) or I010 (10 bits) picture with a scale set == scale_ref, the
    padding included; 64x48 -> 64x48 is also the unscaled ingest"""
    W, H, w, h, ow, oh, filter, left = case
    enc = contexts(W, H, bd)
    rng = np.random.default_rng(w * 131 + h * 7 + ow + bd)
    pics = sr.random_yuv(rng, w, h, bd)
    fmt = I420 if bd == 8 else I010
    got = scaled_ingest(enc, pics, fmt, case)
    want, peak = reference(pics, ow, oh, W, H, filter, left, bd)
    assert_planes(got, want, sr.case_id(case))
    assert enc.scale_info() is None
    if (w, h) == (W, H):
        pic = enc.device_picture(jmhip.to_device(pics, fmt))
        try:
            assert_planes(enc.ingest(pic), got, "identity against the unscaled ingest")
        finally:
            enc.device_free(pic.base)


FORMAT_CASE = (64, 48, 130, 98, 48, 34, sr.BICUBIC, True)


@pytest.mark.parametrize("fmt,bd", [(NV12, 8), (I010, 10), (P010, 10), (I420, 8)], ids=["NV12", "I010", "P010", "I420_misaligned"])
def test_seam_formats(contexts, fmt, bd):
    """the planar and semi-planar formats through the one scaler; I420 with every plane base 2 bytes
    off 16-byte alignment and padded strides"""
    W, H, w, h, ow, oh, filter, left = FORMAT_CASE
    enc = contexts(W, H, bd)
    pics = sr.random_yuv(np.random.default_rng(60 + fmt), w, h, bd)
    got = scaled_ingest(enc, pics, fmt, FORMAT_CASE, pad=6, mis=2)
    assert_planes(got, reference(pics, ow, oh, W, H, filter, left, bd)[0], f"format {fmt}")
    assert enc.input_clamped() == 0


def test_seam_i010_still_counts_the_source():
    """samples above maxv are clamped and counted at the source's size, then scaled"""
    W, H, w, h, ow, oh, filter, left = FORMAT_CASE
    enc = jmhip.Encoder(W, H, search_range=8, bit_depth=10)
    try:
        rng = np.random.default_rng(5)
        pics = list(sr.random_yuv(rng, w, h, 10))
        hot = rng.integers(0, 8, pics[0].shape) == 0
        pics[0] = np.where(hot, 4000, pics[0]).astype(np.uint16)
        got = scaled_ingest(enc, tuple(pics), I010, FORMAT_CASE)
        assert enc.input_clamped() == int(hot.sum()) > 0
        clamped = tuple(np.minimum(a, 1023).astype(np.uint16) for a in pics)
        assert_planes(got, reference(clamped, ow, oh, W, H, filter, left, 10)[0], "I010 above maxv")
    finally:
        enc.close()


def test_seam_rgb_and_tensors(contexts):
    """BGRA8, a u8 HWC tensor and an f16 CHW tensor: converted and chroma-boxed at the source's size
    (rgb_ref / tensor_ref), then scaled"""
    W, H, w, h, ow, oh, filter, left = FORMAT_CASE
    enc = contexts(W, H, 8)
    rng = np.random.default_rng(77)
    enc.input_scale(ow, oh, filter, left)
    try:
        words = rgb_ref.random_words(rng, w, h, BGRA8)
        pic = enc.device_picture(jmhip.to_device_rgb(words, BGRA8 | jmhip.JMH_PIX_BT709, pad_stride=8, misalign=4))
        try:
            got = enc.ingest(pic)
        finally:
            enc.device_free(pic.base)
        src = rgb_ref.convert(words, BGRA8 | jmhip.JMH_PIX_BT709, 8)
        assert_planes(got, reference(src, ow, oh, W, H, filter, left, 8)[0], "BGRA8")
        for dtype, layout in ((tr.U8, "hwc"), (tr.F16, "chw")):
            chans = tr.random_chans(rng, w, h, dtype)
            arr = np.stack(chans, axis=-1 if layout == "hwc" else 0)
            t = enc.device_tensor(jmhip.to_device_tensor(arr, layout, flags=jmhip.JMH_PIX_FULL_RANGE, dtype=dtype))
            try:
                got = enc.ingest_tensor(t)
            finally:
                enc.device_free(t.base)
            src = tr.convert_source_size(chans, dtype, tr.FULL_RANGE, 8)
            assert_planes(got, reference(src, ow, oh, W, H, filter, left, 8)[0], f"tensor {tr.NAMES[dtype]} {layout}")
    finally:
        enc.input_scale(None)


# ---- 2: extremes --------------------------------------------------------------------------------
def worst_signs(n_src, n_dst, filter, n):
    """the signs of the tap row with the largest sum(|q|), repeated with its period along n samples so
    that the row's own taps meet them: True where the tap is positive"""
    first, q = taps(n_src, n_dst, filter, False)
    row = int(np.abs(q.astype(np.int64)).sum(axis=1).argmax())
    T = q.shape[1]
    j = np.arange(n)
    return q[row][(j - int(first[row])) % T] > 0, int(np.abs(q[row].astype(np.int64)).sum())


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("case", [(176, 144, 120, 90, 176, 144, sr.LANCZOS3, False), (64, 48, 256, 192, 64, 48, sr.LANCZOS3, False),
                                  (64, 48, 130, 98, 48, 34, sr.BICUBIC, False)], ids=["up_lanczos3", "down4_lanczos3", "down_bicubic"])
def test_extremes(contexts, case, bd):
    """runs of 0 and maxv that follow the signs of the worst tap row on both axes (the largest and,
    inverted, the smallest intermediates and sums there are), constant maxv, constant 0"""
    W, H, w, h, ow, oh, filter, left = case
    enc = contexts(W, H, bd)
    maxv = (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8
    planes, mags = [], []
    for pw, ph, dw, dh in ((w, h, ow, oh), (w // 2, h // 2, ow // 2, oh // 2)):
        sx, mx = worst_signs(pw, dw, filter, pw)
        sy, my = worst_signs(ph, dh, filter, ph)
        planes.append(np.where(sy[:, None] & sx[None, :], maxv, 0).astype(dt))
        mags += [mx, my]
    assert max(mags) <= 32767
    peak_pic = (planes[0], planes[1], planes[1])
    pictures = {"peaks": peak_pic, "inverted": tuple((maxv - a).astype(dt) for a in peak_pic),
                "maxv": tuple(np.full_like(a, maxv) for a in peak_pic), "zero": tuple(np.zeros_like(a) for a in peak_pic)}
    top = 0
    for name, pics in pictures.items():
        got = scaled_ingest(enc, pics, I420 if bd == 8 else I010, case)
        want, peak = reference(pics, ow, oh, W, H, filter, left, bd)
        top = max(top, peak)
        assert_planes(got, want, f"{name} at {bd} bits")
        if name == "maxv":
            assert all((a == maxv).all() for a in got)
        if name == "zero":
            assert all((a == 0).all() for a in got)
    print(f"largest |h| of the reference, {sr.case_id(case)} at {bd} bits: {top} (largest sum(|q|) {max(mags)})")
    assert top <= 32767


# ---- 3: coded pushes ----------------------------------------------------------------------------
@pytest.mark.parametrize("kw,split", [(dict(search_range=8, slice_mbs=33), 0), (dict(search_range=8, search_mode=3, rdo=1, slice_mbs=33), 1024)],
                         ids=["cavlc", "cabac_split"])
def test_coded_push_scaled_equals_coded_push_of_the_reference(kw, split):
    """push_coded_device of 352x288 I420 sources scaled into a 176x144 context == push_coded_device of
    the scale_ref pictures with the setting off: slice bytes, where, the SSDs, over I P P"""
    W, H, w, h = 176, 144, 352, 288
    pics = seq(w, h, 3, 91)
    small = [reference(p, W, H, W, H, sr.LANCZOS3, True, 8)[0] for p in pics]
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    dev, rdev = [], []
    try:
        if split:
            enc.cabac_split(split)
            ref.cabac_split(split)
        enc.input_scale(W, H, sr.LANCZOS3, chroma_left=True)
        assert enc.scale_info() == {"filter": 3, "chroma_left": True, "out_width": W, "out_height": H}
        dev, rdev = resident(enc, pics, I420), resident(ref, small, I420)
        got = coded_chain(enc, 3, lambda i, st, d: enc.push_coded_device(dev[i], st, QP, d, deblock=DBK), 33)
        want = coded_chain(ref, 3, lambda i, st, d: ref.push_coded_device(rdev[i], st, QP, d, deblock=DBK), 33)
        assert len(got) == len(want) == 3
        for i, ((data, where, stats), (rdata, rwhere, rstats)) in enumerate(zip(got, want)):
            assert len(data) == 3 and data == rdata, f"picture {i}: slice bytes"
            assert where == rwhere, f"picture {i}: where"
            assert stats == rstats, f"picture {i}: {stats} vs {rstats}"
    finally:
        for e, ds in ((enc, dev), (ref, rdev)):
            for d in ds:
                e.device_free(d.base)
            e.close()


def test_torch_tensor_larger_than_the_coded_size():
    """a (3, 288, 352) float16 torch tensor through from_torch into a 176x144 context: the seam and a
    coded push (tests/scale_torch_child.py: torch has to be imported before the library is loaded)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scale_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    if r.returncode == 0 and "SKIP:" in r.stdout:
        pytest.skip(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and "scaled torch tensor: OK" in r.stdout, (r.stdout + r.stderr)[-4000:]


# ---- 4: the setting changes in flight -----------------------------------------------------------
def test_setting_changed_between_two_pushes():
    """A is pushed under one geometry, B under another with a larger source (the scratch picture
    grows while A's kernels may still be queued); each equals its own reference"""
    W, H = 64, 48
    g1, g2 = (W, H, 130, 98, 48, 34, sr.BICUBIC, False), (W, H, 256, 192, 64, 48, sr.LANCZOS3, True)
    a, b = seq(130, 98, 1, 61)[0], seq(256, 192, 1, 62)[0]
    want = [reference(p, g[4], g[5], W, H, g[6], g[7], 8)[0] for p, g in ((a, g1), (b, g2))]
    enc, ref = jmhip.Encoder(W, H, search_range=8, pipeline_depth=2), jmhip.Encoder(W, H, search_range=8, pipeline_depth=2)
    dev = []
    try:
        dev = resident(enc, [a], NV12) + resident(enc, [b], I420)
        enc.input_scale(g1[4], g1[5], g1[6], g1[7])
        enc.push_device(dev[0], I, QP, deblock=DBK)
        enc.input_scale(g2[4], g2[5], g2[6], g2[7])
        enc.push_device(dev[1], I, QP, deblock=DBK)
        enc.input_scale(None)
        for i in range(2):
            res, rec = enc.pop()
            ref.push(*want[i], I, QP, deblock=DBK)
            rres, rrec = ref.pop()
            assert res.tobytes() == rres.tobytes(), f"picture {i}: results"
            assert_planes(rec, rrec, f"picture {i}: recon")
    finally:
        for d in dev:
            enc.device_free(d.base)
        enc.close()
        ref.close()


# ---- 5: ordering --------------------------------------------------------------------------------
def test_source_overwritten_on_the_callers_stream_after_the_push():
    """the source is uploaded on a caller stream, pushed with that stream, and overwritten on it as soon
    as the push returns: the picture is the first content's"""
    W, H = 64, 48
    case = (W, H, 256, 192, 64, 48, sr.LANCZOS3, False)
    first, second = seq(256, 192, 2, 71)
    want = reference(first, 64, 48, W, H, sr.LANCZOS3, False, 8)[0]
    enc, ref = jmhip.Encoder(W, H, search_range=8), jmhip.Encoder(W, H, search_range=8)
    layouts = [jmhip.to_device(p, NV12, pad_stride=6) for p in (first, second)]
    base = stream = None
    try:
        base = enc.device_alloc(layouts[0].buf.nbytes)
        stream = enc.device_stream()
        enc.input_scale(case[4], case[5], case[6], case[7])
        enc.device_upload(base, layouts[0].buf, stream)
        enc.push_device(layouts[0].at(base, stream), I, QP, deblock=DBK)
        enc.device_upload(base, layouts[1].buf, stream)
        res, rec = enc.pop()
        ref.push(*want, I, QP, deblock=DBK)
        rres, rrec = ref.pop()
        assert res.tobytes() == rres.tobytes()
        assert_planes(rec, rrec, "recon")
    finally:
        if stream:
            enc.device_stream_destroy(stream)
        if base:
            enc.device_free(base)
        enc.close()
        ref.close()


# ---- 6: refusals --------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    W, H = 64, 48
    enc = jmhip.Encoder(W, H, search_range=8, pipeline_depth=2)
    made = []
    try:
        def picture(w, h):
            made.append(enc.device_picture(jmhip.to_device(sr.random_yuv(np.random.default_rng(w + h), w, h, 8), I420)))
            return made[-1]

        def status(call):
            with pytest.raises(jmhip.JmhError) as e:
                call()
            return e.value.status
        # the setting itself: refused, and left as it was
        enc.input_scale(62, 34, sr.BICUBIC, True)
        was = enc.scale_info()
        for bad in ((63, 34, 2), (62, 33, 2), (66, 34, 2), (62, 50, 2), (0, 34, 2), (62, 34, 4), (62, 34, -1)):
            assert status(lambda: enc.input_scale(*bad)) == INVALID, bad
        s = jmhip.JmhScale(2, 2, 62, 34)                                               # an unknown flag
        assert enc.lib.jmh_input_scale(enc.ctx, jmhip.ctypes.byref(s)) == INVALID
        assert enc.scale_info() == was == {"filter": 2, "chroma_left": True, "out_width": 62, "out_height": 34}
        # sources under a setting
        good = picture(250, 130)
        odd = jmhip.DevicePicture(I420, 249, 130, good.planes, good.strides)
        assert status(lambda: enc.push_device(odd, I, QP)) == INVALID and status(lambda: enc.ingest(odd)) == INVALID
        huge = jmhip.DevicePicture(I420, jmhip.JMH_SCALE_SRC_MAX + 2, 2, good.planes, [jmhip.JMH_SCALE_SRC_MAX + 2] * 3)
        assert status(lambda: enc.push_device(huge, I, QP)) == INVALID
        enc.input_scale(64, 48, sr.LANCZOS3)
        steep = picture(288, 48)                                                       # 9:2 with Lanczos3: 28 taps
        assert status(lambda: enc.push_device(steep, I, QP)) == UNSUPPORTED and status(lambda: enc.ingest(steep)) == UNSUPPORTED
        enc.input_scale(62, 34, sr.LANCZOS3)
        assert status(lambda: enc.push_device(good, I, QP)) == UNSUPPORTED             # 250 -> 62 is above 4:1: 26 taps
        # nothing was claimed or queued: the pipeline takes its full depth
        enc.input_scale(62, 34, sr.BICUBIC)
        enc.push_device(good, I, QP, deblock=DBK)
        enc.push_device(good, I, QP, deblock=DBK)
        assert status(lambda: enc.push_device(good, I, QP)) == jmhip.JMH_E_STATE
        a, b = enc.pop(), enc.pop()
        assert a[0].tobytes() == b[0].tobytes()
        # off: the coded size bounds the source again
        enc.input_scale(None)
        assert enc.scale_info() is None
        wide = picture(66, 48)
        assert status(lambda: enc.push_device(wide, I, QP)) == INVALID and status(lambda: enc.push_device(good, I, QP)) == INVALID
        fits = picture(50, 38)
        enc.push_device(fits, I, QP, deblock=DBK)                                     # and a good push follows
        enc.pop()
    finally:
        for d in made:
            enc.device_free(d.base)
        enc.close()


# ---- 7: lencod ----------------------------------------------------------------------------------
@pytest.mark.parametrize("bd,extra", [
    (8, ["DeviceCAVLC=1"]),
    (10, ["ProfileIDC=110", "SourceBitDepthLuma=10", "SourceBitDepthChroma=10", "SearchMode=3", "RDOptimization=1", "SymbolMode=1", "DeviceCABAC=1"]),
], ids=["cavlc_8", "cabac_high10"])
def test_lencod_device_input_scale_identical(bd, extra):
    """DeviceInputScale=3 DeviceInputWidth=352 DeviceInputHeight=288 on a 352x288 file == a plain DeviceInput=1
    run on the 176x144 file scale_ref makes from it: the same .264"""
    w, h, W, H, n = 352, 288, 176, 144, 3
    pics = seq(w, h, n, 111, bd)
    common = [f"FramesToBeEncoded={n}", f"SourceWidth={W}", f"SourceHeight={H}", "SearchRange=16", "DeviceInput=1", "DeviceWriterAsync=1"] + extra
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        with open(f"{a}/in.yuv", "wb") as f:
            for p in pics:
                f.write(b"".join(x.tobytes() for x in p))
        with open(f"{b}/in.yuv", "wb") as f:
            for p in pics:
                f.write(b"".join(x.tobytes() for x in reference(p, W, H, W, H, sr.LANCZOS3, False, bd)[0]))
        la = run_lencod(LENCOD, a, common + [f"InputFile={a}/in.yuv", "DeviceInputScale=3", f"DeviceInputWidth={w}", f"DeviceInputHeight={h}"])
        assert f"the source has {w}x{h} samples: resampled on the device to {W}x{H}, Lanczos3, chroma centred" in la
        lb = run_lencod(LENCOD, b, common + [f"InputFile={b}/in.yuv"])
        assert "resampled on the device" not in lb and "pushed from device memory" in lb
        got, want = open(f"{a}/a.264", "rb").read(), open(f"{b}/a.264", "rb").read()
        assert len(want) > 100 and got == want
