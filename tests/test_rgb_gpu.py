"""RGB pictures pushed from the device (include/jmhip_rgb.h): k_ingest_rgb converts a
BGRA8 / RGBA8 / RGB10A2 / BGR10A2 picture to 4:2:0, packs and pads it where k_ingest moves a YUV one.

The reference of the seam is tests/rgb_ref.py, a numpy restatement of the definition's formulas
(tests/test_rgb_core.py holds it against the table, the core and the library).  The reference of
every pipeline case is a second Encoder with the same configuration, fed the picture rgb_ref
converted and padded on the host through the ordinary push.  Every check is exact."""
import tempfile

import numpy as np
import pytest

import rgb_ref
from jmpaths import LENCOD, ensure_built, load_jmhip
from test_gpu_parity import run_lencod
from test_ingest_gpu import assert_chains_equal, chain, coded_chain

jmhip = load_jmhip()
pytestmark = pytest.mark.gpu

I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE
BGRA8, RGBA8, RGB10A2, BGR10A2 = rgb_ref.LAYOUTS
BT709, FULL = rgb_ref.BT709, rgb_ref.FULL_RANGE
FLAGS = (0, BT709, FULL, BT709 | FULL)
DBK = (0, 0, 0)
# coded size -> source sizes: 48x32 has an odd number of macroblock columns (8-byte chroma rows) and a
# vector that straddles the width; 1056x32 is wider than one wave step of 512 pixels
SIZES = {(48, 32): [(34, 18)], (32, 32): [(2, 2), (30, 2), (2, 30), (32, 32)], (1056, 32): [(1042, 18)]}


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


# ---- 1: the seam --------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", rgb_ref.LAYOUTS, ids=[rgb_ref.NAMES[f] for f in rgb_ref.LAYOUTS])
def test_seam_equals_reference(contexts, layout):
    """enc.ingest == rgb_ref, bit-exactly: both matrices and both ranges, every source size, strides
    tight / +4 / +52, bases 0 / 4 / 8 / 12 bytes off a 256-byte boundary (the 16-byte loads and the
    dword loads), random words plus the eight corners; nothing counted as clamped"""
    bd = rgb_ref.depth_of(layout)
    rng = np.random.default_rng(300 + layout)
    n = 0
    for (cw, ch), sources in SIZES.items():
        enc = contexts(cw, ch, bd)
        for w, h in sources:
            words = rgb_ref.random_words(rng, w, h, layout)
            want = {fl: rgb_ref.to_yuv(words, layout | fl, bd, cw, ch) for fl in FLAGS}      # once per picture
            for pad in (0, 4, 52):
                for mis in (0, 4, 8, 12):
                    base = enc.device_alloc(jmhip.to_device_rgb(words, layout, pad_stride=pad, misalign=mis).buf.nbytes)
                    try:
                        for fl in FLAGS:
                            pic = enc.device_picture(jmhip.to_device_rgb(words, layout | fl, pad_stride=pad, misalign=mis), base=base)
                            got = enc.ingest(pic)
                            what = f"{rgb_ref.NAMES[layout]} flags {fl:#x} {w}x{h} in {cw}x{ch} stride +{pad} base +{mis}"
                            for name, a, b in zip("YUV", got, want[fl]):
                                assert a.dtype == b.dtype and np.array_equal(a, b), f"{what}: plane {name} differs at {np.argwhere(a != b)[:4].tolist()}"
                            assert enc.input_clamped() == 0, what
                            n += 1
                    finally:
                        enc.device_free(base)
    assert n == 6 * 3 * 4 * 4


# ---- 2: status codes ----------------------------------------------------------------------------
def test_status_codes(contexts):
    e8, e9, e10 = contexts(32, 32, 8), contexts(32, 32, 9), contexts(32, 32, 10)
    words = rgb_ref.random_words(np.random.default_rng(5), 30, 18, BGRA8)
    good = None
    try:
        good = e8.device_picture(jmhip.to_device_rgb(words, BGRA8, pad_stride=8))
        assert good.strides == [128]

        def status(enc, **change):
            pic = jmhip.DevicePicture(good.format, good.width, good.height, good.planes, good.strides)
            for k, v in change.items():
                setattr(pic, k, v)
            codes = []
            for push in (False, True):
                try:
                    if push:
                        enc.push_device(pic, I, 28)
                        enc.pop()
                    else:
                        enc.ingest(pic)
                    codes.append(jmhip.JMH_OK)
                except jmhip.JmhError as e:
                    codes.append(e.status)
            assert codes[0] == codes[1], codes          # the seam and the push answer alike
            return codes[0]
        UNSUP, INVAL, OK = jmhip.JMH_E_UNSUPPORTED_CFG, jmhip.JMH_E_INVALID_ARG, jmhip.JMH_OK
        # the right layout in the wrong context bit depth
        assert status(e10, format=BGRA8) == UNSUP and status(e10, format=RGBA8 | BT709) == UNSUP
        assert status(e8, format=RGB10A2) == UNSUP and status(e8, format=BGR10A2 | FULL) == UNSUP
        for f in rgb_ref.LAYOUTS:
            assert status(e9, format=f) == UNSUP, f
        # the argument rules, before the bit depth is looked at
        for enc in (e8, e10):
            assert status(enc, format=jmhip.JMH_PIX_I420 | BT709) == INVAL                  # a flag on a YUV format
            assert status(enc, format=jmhip.JMH_PIX_NV12 | FULL) == INVAL
            assert status(enc, format=BGRA8 | 1 << 10) == INVAL and status(enc, format=BGRA8 | 1 << 7) == INVAL   # an unknown bit
            assert status(enc, format=BGRA8 - (1 << 31)) == INVAL                           # a negative format
            assert status(enc, strides=[4 * 30 - 4]) == INVAL                                # stride 4w - 4
            assert status(enc, planes=[good.planes[0] + 2]) == INVAL                         # address + 2
            assert status(enc, strides=[128 + 2]) == INVAL                                   # stride + 2
            assert status(enc, width=29) == INVAL and status(enc, height=17) == INVAL        # odd
            assert status(enc, width=34, strides=[256]) == INVAL                             # beyond the coded size
            assert status(enc, height=34) == INVAL and status(enc, width=0) == INVAL
            assert status(enc, planes=[None]) == INVAL                                       # a null plane[0]
            assert status(enc, planes=[None, good.planes[0], good.planes[0]]) == INVAL
            for f in (4, 5, 15, 20, 255):                                                    # 4 is still invalid; so are 5..15 and 20
                assert status(enc, format=f, planes=[good.planes[0]] * 3, strides=[128] * 3) == INVAL, f
        # plane[1] and plane[2] are not read: null is fine, and so is anything else
        assert status(e8, planes=[good.planes[0], None, None]) == OK
        assert status(e8, planes=[good.planes[0], 2, 3], strides=[128, 1, -7]) == OK
        assert status(e8, planes=[good.planes[0] + 4], width=28) == OK                       # any multiple of 4
    finally:
        if good:
            e8.device_free(good.base)


# ---- the pipeline -------------------------------------------------------------------------------
W, H, SW, SH, QP = 64, 48, 62, 46, 28


def rgb_seq(w, h, n, seed, layout):
    """n pictures of w x h words: a moving smooth texture per component plus noise, so that P pictures
    find motion; alpha is noise"""
    rng = np.random.default_rng(seed)
    ten = layout >= RGB10A2
    top, sh = (1023, 10) if ten else (255, 8)
    yy, xx = np.mgrid[0:h + 4 * n, 0:w + 4 * n]
    comps = [(0.5 + 0.35 * np.sin(xx / a) * np.cos(yy / b)) * top for a, b in ((5.0, 7.0), (6.0, 4.0), (9.0, 5.0))]
    out = []
    for i in range(n):
        c = [np.clip(p[2 * i:2 * i + h, 3 * i:3 * i + w] + rng.integers(-top // 50, top // 50 + 1, (h, w)), 0, top).astype(np.uint32) for p in comps]
        alpha = rng.integers(0, 4 if ten else 256, (h, w)).astype(np.uint32)
        out.append(np.ascontiguousarray(c[0] | c[1] << sh | c[2] << 2 * sh | alpha << 3 * sh))
    return out


def resident(enc, pics, fmt, pad=4, mis=4):
    """every picture uploaded into its own allocation (complete on return)"""
    return [enc.device_picture(jmhip.to_device_rgb(p, fmt, pad_stride=pad, misalign=mis)) for p in pics]


# ---- 3 ----
@pytest.mark.parametrize("kw,fmt", [
    (dict(search_range=8), BGRA8),
    (dict(search_range=8, search_mode=3, bit_depth=10, transform_8x8_mode=1), RGB10A2 | BT709 | FULL),
], ids=["ffs_bgra8", "epzs_high10_rgb10a2_709_full"])
def test_pipeline_device_push_equals_host_push(kw, fmt):
    """I then two P of 62x46 in a 64x48 context: push_device of the RGB picture == push of the YUV
    picture converted and padded on the host: results, reconstruction, deblocked planes"""
    bd = kw.get("bit_depth", 8)
    pics = rgb_seq(SW, SH, 3, 61 + fmt, fmt & 0xff)
    yuv = [rgb_ref.to_yuv(p, fmt, bd, W, H) for p in pics]
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    dev = []
    try:
        dev = resident(enc, pics, fmt)
        got = chain(enc, 3, lambda i, st: enc.push_device(dev[i], st, QP, deblock=DBK))
        want = chain(ref, 3, lambda i, st: ref.push(*yuv[i], st, QP, deblock=DBK))
        assert_chains_equal(got, want, f"format {fmt:#x}")
        assert enc.input_clamped() == 0
    finally:
        for d in dev:
            enc.device_free(d.base)
        enc.close()
        ref.close()


# ---- 4 ----
def test_coded_device_push_with_heads_equals_coded_host_push():
    """push_coded_device(..., heads=...) of RGBA == push_coded(..., heads=...) of the converted YUV:
    the access unit's bytes, every where field, the three SSDs, no fallback"""
    from test_nal_gpu import heads_for
    fmt = RGBA8 | BT709
    kw = dict(search_range=8, slice_mbs=5)
    pics = rgb_seq(SW, SH, 3, 71, RGBA8)
    yuv = [rgb_ref.to_yuv(p, fmt, 8, W, H) for p in pics]
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    dev = []
    try:
        dev = resident(enc, pics, fmt, pad=0, mis=0)
        got = coded_chain(enc, 3, lambda i, st, d: enc.push_coded_device(dev[i], st, QP, d, crop=(SW, SH), deblock=DBK, heads=heads_for(i, len(d))), 5)
        want = coded_chain(ref, 3, lambda i, st, d: ref.push_coded(*yuv[i], st, QP, d, crop=(SW, SH), deblock=DBK, heads=heads_for(i, len(d))), 5)
        assert len(got) == len(want) == 3
        for i, ((data, where, stats), (rdata, rwhere, rstats)) in enumerate(zip(got, want)):
            assert len(data) == len(rdata) == 3 and data == rdata, f"picture {i}: access unit bytes"
            assert all(d.startswith(b"\x00\x00\x00\x01") for d in data), f"picture {i}: NAL units"
            assert where == rwhere, f"picture {i}: where"
            assert stats["ssd"] == rstats["ssd"] and len(stats["ssd"]) == 3 and stats["fallback"] == 0 == rstats["fallback"], f"picture {i}: {stats} vs {rstats}"
    finally:
        for d in dev:
            enc.device_free(d.base)
        enc.close()
        ref.close()


# ---- 5 ----
def test_one_device_buffer_overwritten_right_after_each_push():
    """Picture i is uploaded into the one buffer on the caller's stream and pushed naming that stream;
    picture i + 1 is uploaded into the same buffer as soon as the push returns (the library made the
    stream wait for the conversion kernel).  Six pictures: the results are those of the host pushes."""
    n = 6
    pics = rgb_seq(SW, SH, n, 81, BGRA8)
    yuv = [rgb_ref.to_yuv(p, BGRA8, 8, W, H) for p in pics]
    kw = dict(search_range=8)
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    layouts = [jmhip.to_device_rgb(p, BGRA8, pad_stride=12) for p in pics]
    base = stream = None
    try:
        base = enc.device_alloc(max(L.buf.nbytes for L in layouts))
        stream = enc.device_stream()
        enc.device_upload(base, layouts[0].buf, stream)

        def push(i, st):
            enc.push_device(layouts[i].at(base, stream), st, QP, deblock=DBK)
            if i + 1 < n:
                enc.device_upload(base, layouts[i + 1].buf, stream)
        got = chain(enc, n, push)
        want = chain(ref, n, lambda i, st: ref.push(*yuv[i], st, QP, deblock=DBK))
        assert_chains_equal(got, want, "reused buffer")
    finally:
        if stream:
            enc.device_stream_destroy(stream)
        if base:
            enc.device_free(base)
        enc.close()
        ref.close()


# ---- 6: lencod ----------------------------------------------------------------------------------
def test_lencod_rgb_input_identical():
    """a 3-frame 180x146 BGRA file (coded 192x160) against the .yuv rgb_ref makes from it, both with
    DeviceInput=1 DeviceCAVLC=1 DeviceWriterAsync=1 DeviceNAL=1: the same .264, the same recon file,
    the same bits, QP and SNR columns"""
    from test_coded_gpu import picture_columns
    w, h, n = 180, 146, 3
    pics = rgb_seq(w, h, n, 91, BGRA8)
    common = ["FramesToBeEncoded=3", f"SourceWidth={w}", f"SourceHeight={h}", "SearchRange=16", "DeviceInput=1", "DeviceCAVLC=1",
              "DeviceWriterAsync=1", "DeviceNAL=1"]
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        with open(f"{a}/in.bgra", "wb") as f:
            for p in pics:
                f.write(p.astype("<u4").tobytes())
        with open(f"{b}/in.yuv", "wb") as f:
            for p in pics:
                for plane in rgb_ref.convert(p, BGRA8 | BT709, 8):
                    f.write(plane.tobytes())
        la = run_lencod(LENCOD, a, common + [f"InputFile={a}/in.bgra", "DeviceInputFormat=16", "DeviceInputMatrix=1"])
        assert "the source is RGB, format 16" in la and "BT.709" in la and "pushed from device memory" in la
        lb = run_lencod(LENCOD, b, common + [f"InputFile={b}/in.yuv"])
        assert "the source is RGB" not in lb and "pushed from device memory" in lb
        assert open(f"{a}/a.264", "rb").read() == open(f"{b}/a.264", "rb").read()
        assert open(f"{a}/rec.yuv", "rb").read() == open(f"{b}/rec.yuv", "rb").read()
        ca, cb = picture_columns(la), picture_columns(lb)
        assert len(ca) == 3 and ca == cb
