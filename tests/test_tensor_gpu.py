"""RGB tensors pushed from the device (include/jmhip_tensor.h): k_ingest_tensor
quantises a (3, H, W) or (H, W, 3 or 4) tensor of uint8, uint16, float16, bfloat16 or float32,
converts it to 4:2:0, packs and pads it where k_ingest_rgb converts a picture of packed dwords.

The reference of the seam is tests/tensor_ref.py: numpy float64 quantisation (held against integer
arithmetic in tests/test_tensor_core.py), then rgb_ref's conversion of the packed words.  The
reference of every pipeline case is a second Encoder with the same configuration, fed the picture
tensor_ref converted and padded on the host through the ordinary push.  Every check is exact."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import rgb_ref
import tensor_ref as tr
from jmpaths import LENCOD, ensure_built, load_jmhip
from test_gpu_parity import run_lencod
from test_ingest_gpu import assert_chains_equal, chain, coded_chain

jmhip = load_jmhip()
pytestmark = pytest.mark.gpu

I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE
U8, U16, F16, BF16, F32 = tr.DTYPES
BT709, FULL = tr.BT709, tr.FULL_RANGE
DBK = (0, 0, 0)
# coded size -> source sizes: 48x32 has an odd number of macroblock columns (8-byte chroma rows) and a
# vector that straddles the width; 1056x32 is wider than one wave step of 512 pixels, with the
# straddling vector neither first nor last (1042) and with rows whose bytes are a multiple of 16 for
# every element size, so that the 16-byte loads run for more than one step too (1040)
SIZES = {(48, 32): [(34, 18)], (32, 32): [(2, 2), (30, 2), (2, 30), (32, 32)], (1056, 32): [(1042, 18), (1040, 18)]}
KINDS = ("chw", "hwc3", "hwc4", "bgr")


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


def layout_of(chans, dtype, kind, flags=0, pad=0, mis=0):
    """the TensorLayout of R, G, B element arrays in one of KINDS: planar, interleaved with 3 or 4
    channels (the fourth is noise that is never read), interleaved B, G, R"""
    r, g, b = chans
    if kind == "chw":
        arr, lay, order = np.stack([r, g, b]), "chw", "rgb"
    elif kind == "hwc3":
        arr, lay, order = np.stack([r, g, b], axis=-1), "hwc", "rgb"
    elif kind == "hwc4":
        alpha = np.frombuffer(b"\xa5" * r.nbytes, dtype=r.dtype).reshape(r.shape)
        arr, lay, order = np.stack([r, g, b, alpha], axis=-1), "hwc", "rgb"
    else:
        arr, lay, order = np.stack([b, g, r], axis=-1), "hwc", "bgr"
    return jmhip.to_device_tensor(arr, lay, order=order, flags=flags, pad_stride=pad, misalign=mis, dtype=dtype)


# ---- 1: the seam --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,bd", tr.PAIRS, ids=[f"{tr.NAMES[d]}_{b}" for d, b in tr.PAIRS])
def test_seam_equals_reference(contexts, dtype, bd):
    """enc.ingest_tensor == tensor_ref.convert, bit-exactly.  Every source size in the four layouts,
    each with row strides tight / +es / +52 es crossed with channel bases 0 / es / 4 / 12 bytes off a
    256-byte boundary (the 16-byte loads, the dword loads and the element loads of the planar
    instance).  The four flag sets only change the coefficients in the kernel's arguments, not a load
    or store path, so they rotate through the stride x base combinations instead of multiplying them:
    every (size, layout) sees each flag set three times.  Random content that leaves [0, 1] on both
    sides with a NaN, a negative value, a value above 1 and the tie 1/2 in every float picture."""
    es = tr.ES[dtype]
    rng = np.random.default_rng(400 + 16 * dtype + bd)
    n = 0
    for (cw, ch), sources in SIZES.items():
        enc = contexts(cw, ch, bd)
        for w, h in sources:
            chans = tr.random_chans(rng, w, h, dtype)
            assert not dtype >= F16 or tr.holds_condition(chans, dtype)
            want = {fl: tr.convert(chans, dtype, fl, bd, cw, ch) for fl in tr.FLAGS}      # once per picture
            for kind in KINDS:
                combos = [(pad, mis) for pad in (0, es, 52 * es) for mis in sorted({0, es, 4, 12})]
                for i, (pad, mis) in enumerate(combos):
                    fl = tr.FLAGS[(i + i // 4) % 4]
                    t = enc.device_tensor(layout_of(chans, dtype, kind, fl, pad, mis))
                    try:
                        got = enc.ingest_tensor(t)
                    finally:
                        enc.device_free(t.base)
                    what = f"{tr.NAMES[dtype]} in {bd} bits, {kind}, flags {fl:#x}, {w}x{h} in {cw}x{ch}, stride +{pad}, base +{mis}"
                    for name, a, b in zip("YUV", got, want[fl]):
                        assert a.dtype == b.dtype and np.array_equal(a, b), f"{what}: plane {name} differs at {np.argwhere(a != b)[:4].tolist()}"
                    assert enc.input_clamped() == 0, what
                    n += 1
    assert n == 7 * 4 * 3 * len({0, es, 4, 12})


# ---- 2: the quantiser's edge sets through the kernel --------------------------------------------
@pytest.mark.parametrize("dtype", tr.FLOATS, ids=[tr.NAMES[d] for d in tr.FLOATS])
@pytest.mark.parametrize("bd", [8, 10])
def test_quantiser_edges_through_the_kernel(contexts, dtype, bd):
    """All 65,536 patterns of F16 / BF16, and for F32 the edge set of tests/test_tensor_core.py plus
    2^16 random patterns, as grey pixels: one plane serves as R, G and B, laid out as pictures of 2 rows
    x 1024 in a 1024x32 context, all uploaded once.  At full range the luma of a grey pixel is q itself
    (tensor_ref.grey_luma asserts that the map is injective over q), so Y names the q the kernel made."""
    if dtype == F32:
        bits = np.concatenate([tr.f32_edge_bits(bd), np.random.default_rng(7).integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)])
    else:
        bits = np.arange(65536, dtype=np.uint16)
    cw, chunk = 1024, 2048
    pad = -len(bits) % chunk
    elems = np.concatenate([bits, np.zeros(pad, bits.dtype)])
    want = tr.grey_luma(tr.quantise(elems, dtype, bd), FULL, bd)
    enc = contexts(cw, 32, bd)
    es = tr.ES[dtype]
    base = enc.device_alloc(elems.nbytes)
    try:
        enc.device_upload(base, elems)
        for k in range(len(elems) // chunk):
            at = base + k * chunk * es
            y, _, _ = enc.ingest_tensor(jmhip.DeviceTensor(dtype, FULL, cw, 2, [at, at, at], es, cw * es))
            got = y[:2].astype(np.int64).ravel()
            ref = want[k * chunk:(k + 1) * chunk]
            bad = np.flatnonzero(got != ref)
            assert not len(bad), f"{tr.NAMES[dtype]} at {bd} bits: bits {int(elems[k * chunk + bad[0]]):#x} gave {got[bad[0]]}, want {ref[bad[0]]}"
    finally:
        enc.device_free(base)


# ---- 3: status codes ----------------------------------------------------------------------------
def test_status_codes(contexts):
    """every argument rule of include/jmhip_tensor.h, in both contexts, through the seam and the push
    alike; nothing is queued by a refused tensor: an ordinary push / pop afterwards is unaffected"""
    e8, e9, e10 = contexts(32, 32, 8), contexts(32, 32, 9), contexts(32, 32, 10)
    UNSUP, INVAL, OK = jmhip.JMH_E_UNSUPPORTED_CFG, jmhip.JMH_E_INVALID_ARG, jmhip.JMH_OK
    rng = np.random.default_rng(5)
    base = e8.device_alloc(3 * 32 * 32 * 4 + 64)
    try:
        e8.device_upload(base, rng.integers(0, 256, 3 * 32 * 32 * 4 + 64, dtype=np.uint8))

        def good(dtype):
            es = tr.ES[dtype]
            return jmhip.DeviceTensor(dtype, 0, 30, 18, [base + i * 32 * 32 * es for i in range(3)], es, 32 * es)

        def status(enc, dt, /, **change):
            t = good(dt)
            for k, v in change.items():
                setattr(t, k, v)
            codes = []
            for push in (False, True):
                try:
                    if push:
                        enc.push_tensor(t, I, 28)
                        enc.pop()
                    else:
                        enc.ingest_tensor(t)
                    codes.append(OK)
                except jmhip.JmhError as e:
                    codes.append(e.status)
            assert codes[0] == codes[1], codes          # the seam and the push answer alike
            return codes[0]
        # a valid tensor in the wrong context
        assert status(e10, U8) == UNSUP and status(e8, U16) == UNSUP
        for dt in tr.DTYPES:
            assert status(e9, dt) == UNSUP, dt
        assert status(e8, U8) == OK and status(e10, U16) == OK
        for dt in tr.FLOATS:
            assert status(e8, dt) == OK and status(e10, dt, flags=BT709 | FULL) == OK
        # the argument rules, before the bit depth is looked at
        for enc in (e8, e10):
            for dt in tr.DTYPES:
                es = tr.ES[dt]
                ch = good(dt).chans
                assert status(enc, dt, dtype=5) == INVAL and status(enc, dt, dtype=-1) == INVAL            # outside the enum
                for fl in (1, 1 << 7, 1 << 10, 16, BT709 | 1, -1):                                            # any bit but the two
                    assert status(enc, dt, flags=fl) == INVAL, fl
                assert status(enc, dt, width=29) == INVAL and status(enc, dt, height=17) == INVAL           # odd
                assert status(enc, dt, width=0) == INVAL and status(enc, dt, height=0) == INVAL
                assert status(enc, dt, width=34, stride_y=64 * es) == INVAL and status(enc, dt, height=34) == INVAL   # beyond the coded size
                assert status(enc, dt, stride_x=0) == INVAL and status(enc, dt, stride_x=-es, stride_y=64 * es) == INVAL
                assert status(enc, dt, stride_y=29 * es) == INVAL                                           # (w - 1) stride_x + es - es
                assert status(enc, dt, stride_x=3 * es, stride_y=29 * 3 * es) == INVAL
                assert status(enc, dt, stride_y=-32 * es) == INVAL                                          # negative
                for i in range(3):
                    assert status(enc, dt, chans=[None if j == i else c for j, c in enumerate(ch)]) == INVAL   # a null channel
                    if es > 1:
                        assert status(enc, dt, chans=[c + 1 if j == i else c for j, c in enumerate(ch)]) == INVAL   # address + 1
                if es > 1:
                    assert status(enc, dt, stride_y=32 * es + 1) == INVAL and status(enc, dt, stride_x=es + 1, stride_y=64 * es) == INVAL
                if es > 2:
                    assert status(enc, dt, chans=[ch[0] + 2, ch[1], ch[2]]) == INVAL and status(enc, dt, stride_y=32 * es + 2) == INVAL
        # what is valid: the least row stride, one address three times, any multiple of es
        assert status(e8, U8, stride_y=30) == OK and status(e8, U8, chans=[base + 1] * 3) == OK
        assert status(e8, F16, stride_x=6, stride_y=29 * 6 + 2, chans=[base, base + 2, base + 4]) == OK
        assert status(e10, F32, chans=[base + 4, base + 8, base + 12], stride_x=16, stride_y=29 * 16 + 4) == OK
        # nothing is left queued: an ordinary picture goes through
        y = rng.integers(0, 256, (32, 32), dtype=np.uint8)
        c = rng.integers(0, 256, (16, 16), dtype=np.uint8)
        e8.push(y, c, c, I, 28)
        res, rec = e8.pop()
        ref = jmhip.Encoder(32, 32, search_range=8, bit_depth=8, pipeline_depth=2)
        try:
            ref.push(y, c, c, I, 28)
            rres, rrec = ref.pop()
        finally:
            ref.close()
        assert res.tobytes() == rres.tobytes() and all(np.array_equal(a, b) for a, b in zip(rec, rrec))
    finally:
        e8.device_free(base)


# ---- the pipeline -------------------------------------------------------------------------------
W, H, SW, SH, QP = 64, 48, 50, 34, 28


def tensor_seq(w, h, n, seed, dtype):
    """n pictures as R, G, B element arrays: a moving smooth texture per component plus noise, so that
    P pictures find motion; floats leave [0, 1] a little and carry the specials"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h + 4 * n, 0:w + 4 * n]
    comps = [0.5 + 0.45 * np.sin(xx / a) * np.cos(yy / b) for a, b in ((5.0, 7.0), (6.0, 4.0), (9.0, 5.0))]
    out = []
    for i in range(n):
        c = [p[2 * i:2 * i + h, 3 * i:3 * i + w] + rng.uniform(-0.07, 0.07, (h, w)) for p in comps]
        if dtype == U8:
            out.append([np.clip(np.rint(a * 255), 0, 255).astype(np.uint8) for a in c])
        elif dtype == U16:
            out.append([np.clip(np.rint(a * 1023), 0, 1023).astype(np.uint16) for a in c])
        else:
            ch = [tr.from_float32(a.astype(np.float32), dtype) for a in c]
            for j, v in enumerate(tr.float_specials(dtype)):
                ch[j % 3][h - 1, w - 1 - j // 3] = v
            assert tr.holds_condition(ch, dtype)
            out.append(ch)
    return out


SOURCES = [("f16_chw", F16, "chw", 0), ("u8_hwc3", U8, "hwc3", BT709)]


# ---- 4 ----
@pytest.mark.parametrize("dtype,kind,flags", [s[1:] for s in SOURCES], ids=[s[0] for s in SOURCES])
def test_push_tensor_equals_host_push(dtype, kind, flags):
    """I + P + P of 50x34 in a 64x48 context: push_tensor == push of the YUV picture tensor_ref converted
    and padded on the host: results, reconstruction, deblocked planes"""
    pics = tensor_seq(SW, SH, 3, 61 + dtype, dtype)
    yuv = [tr.convert(p, dtype, flags, 8, W, H) for p in pics]
    kw = dict(search_range=8)
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    dev = []
    try:
        dev = [enc.device_tensor(layout_of(p, dtype, kind, flags, pad=4, mis=4)) for p in pics]
        got = chain(enc, 3, lambda i, st: enc.push_tensor(dev[i], st, QP, deblock=DBK))
        want = chain(ref, 3, lambda i, st: ref.push(*yuv[i], st, QP, deblock=DBK))
        assert_chains_equal(got, want, f"{tr.NAMES[dtype]} {kind}")
        assert enc.input_clamped() == 0
    finally:
        for d in dev:
            enc.device_free(d.base)
        enc.close()
        ref.close()


# ---- 5 ----
@pytest.mark.parametrize("dtype,kind,flags", [s[1:] for s in SOURCES], ids=[s[0] for s in SOURCES])
def test_push_coded_tensor_with_heads_equals_coded_host_push(dtype, kind, flags):
    """push_coded_tensor(..., heads=...) == push_coded(..., heads=...) of the converted YUV: the access
    unit's bytes, every where field, the three SSDs, no fallback"""
    from test_nal_gpu import heads_for
    kw = dict(search_range=8, slice_mbs=5)
    pics = tensor_seq(SW, SH, 3, 71 + dtype, dtype)
    yuv = [tr.convert(p, dtype, flags, 8, W, H) for p in pics]
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    dev = []
    try:
        dev = [enc.device_tensor(layout_of(p, dtype, kind, flags)) for p in pics]
        got = coded_chain(enc, 3, lambda i, st, d: enc.push_coded_tensor(dev[i], st, QP, d, crop=(SW, SH), deblock=DBK, heads=heads_for(i, len(d))), 5)
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


# ---- 6 ----
def test_one_source_overwritten_right_after_each_push():
    """Picture i is uploaded into the one buffer on the caller's stream and pushed naming that stream;
    picture i + 1 is uploaded over it as soon as the push returns (the library made the stream wait for
    the kernel).  Five pictures: the results are those of the host pushes of the originals."""
    n = 5
    pics = tensor_seq(SW, SH, n, 81, BF16)
    yuv = [tr.convert(p, BF16, FULL, 8, W, H) for p in pics]
    kw = dict(search_range=8)
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    layouts = [layout_of(p, BF16, "chw", FULL, pad=12) for p in pics]
    base = stream = None
    try:
        base = enc.device_alloc(max(L.buf.nbytes for L in layouts))
        stream = enc.device_stream()
        enc.device_upload(base, layouts[0].buf, stream)

        def push(i, st):
            enc.push_tensor(layouts[i].at(base, stream), st, QP, deblock=DBK)
            if i + 1 < n:
                enc.device_upload(base, layouts[i + 1].buf, stream)
        got = chain(enc, n, push)
        want = chain(ref, n, lambda i, st: ref.push(*yuv[i], st, QP, deblock=DBK))
        assert_chains_equal(got, want, "reused source")
    finally:
        if stream:
            enc.device_stream_destroy(stream)
        if base:
            enc.device_free(base)
        enc.close()
        ref.close()


# ---- 7 ----
def test_alternating_with_host_device_picture_and_rgb_pushes():
    """one context takes, in turn, a host picture, a tensor (F32 HWC4), an NV12 device picture, a tensor
    (U8 CHW) and a BGRA8 picture: the results are those of the host pushes of the same YUV pictures"""
    pics = tensor_seq(SW, SH, 5, 91, U8)
    yuv_src = [tr.convert_source_size(p, U8, 0, 8) for p in pics]
    yuv = [rgb_ref.pad(p, W, H) for p in yuv_src]
    as_f32 = [(c.astype(np.float32) / np.float32(255)) for c in pics[1]]            # quantises back to the bytes
    assert all(np.array_equal(tr.quantise(a, F32, 8), c) for a, c in zip(as_f32, pics[1]))
    bgra = pics[4][2].astype(np.uint32) | pics[4][1].astype(np.uint32) << 8 | pics[4][0].astype(np.uint32) << 16 | 0x5A000000
    kw = dict(search_range=8)
    enc, ref = jmhip.Encoder(W, H, **kw), jmhip.Encoder(W, H, **kw)
    dev = {}
    try:
        dev[1] = enc.device_tensor(layout_of(as_f32, F32, "hwc4", 0, pad=4, mis=4))
        dev[2] = enc.device_picture(jmhip.to_device(yuv_src[2], jmhip.JMH_PIX_NV12, pad_stride=1, misalign=1))
        dev[3] = enc.device_tensor(layout_of(pics[3], U8, "chw", 0, pad=1, mis=1))
        dev[4] = enc.device_picture(jmhip.to_device_rgb(bgra, jmhip.JMH_PIX_BGRA8))

        def push(i, st):
            if i == 0:
                enc.push(*yuv[0], st, QP, deblock=DBK)
            elif i in (1, 3):
                enc.push_tensor(dev[i], st, QP, deblock=DBK)
            else:
                enc.push_device(dev[i], st, QP, deblock=DBK)
        got = chain(enc, 5, push)
        want = chain(ref, 5, lambda i, st: ref.push(*yuv[i], st, QP, deblock=DBK))
        assert_chains_equal(got, want, "alternating")
        assert enc.input_clamped() == 0
    finally:
        for d in dev.values():
            enc.device_free(d.base)
        enc.close()
        ref.close()


def test_seam_clamp_count_is_reset_by_seams_that_do_not_count():
    """one 10-bit context of 16x16, seams of 16x16 sources in turn: an I010 picture with a known number of samples
    above 1023 (the count), a u16 tensor (0), an RGB10A2 picture (0), the I010 picture again (the count again)"""
    rng = np.random.default_rng(77)
    planes = [rng.integers(0, 1024, s).astype(np.uint16) for s in ((16, 16), (8, 8), (8, 8))]
    for pl, where, val in ((0, (3, 5), 1024), (0, (15, 15), 65535), (0, (0, 0), 4000), (1, (7, 0), 1024), (2, (2, 6), 2048)):
        planes[pl][where] = val
    over = sum(int((p > 1023).sum()) for p in planes)
    assert over == 5
    chans = [rng.integers(0, 1024, (16, 16)).astype(np.uint16) for _ in range(3)]
    words = rng.integers(0, 1 << 32, (16, 16), dtype=np.uint64).astype(np.uint32)
    enc = jmhip.Encoder(16, 16, search_range=8, bit_depth=10)
    dev = []
    try:
        dev.append(enc.device_picture(jmhip.to_device(tuple(planes), jmhip.JMH_PIX_I010)))
        dev.append(enc.device_tensor(layout_of(chans, U16, "chw")))
        dev.append(enc.device_picture(jmhip.to_device_rgb(words, jmhip.JMH_PIX_RGB10A2)))
        for src, want in ((dev[0], over), (dev[1], 0), (dev[2], 0), (dev[0], over)):
            enc.ingest_tensor(src) if src is dev[1] else enc.ingest(src)
            assert enc.input_clamped() == want
    finally:
        for d in dev:
            enc.device_free(d.base)
        enc.close()


# ---- 8: a torch tensor --------------------------------------------------------------------------
def test_torch_tensor_through_from_torch():
    """A float16 (3, H, W) torch tensor made by torch ops on a non-default torch stream, and its
    .permute(1, 2, 0) view, pushed through Encoder.from_torch with no synchronisation between the
    producer and the push: the results equal the reference computed from t.cpu().  It runs in a child
    process (tests/tensor_torch_child.py) because that is what it is about: torch must be imported
    before libjmhip.so is loaded for the two to share one HIP runtime, and this process has loaded
    the library long ago."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tensor_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    if r.returncode == 0 and "SKIP:" in r.stdout:
        pytest.skip(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and "torch tensor: OK" in r.stdout, (r.stdout + r.stderr)[-4000:]


# ---- 9: lencod ----------------------------------------------------------------------------------
def test_lencod_tensor_input_identical():
    """3 QCIF frames from an rgb24 file (DeviceInputTensor=1) and from a gbrpf32le file of the same
    quantised picture (DeviceInputTensor=4) against the .yuv tensor_ref makes from it, all with
    DeviceInput=1 DeviceCAVLC=1 DeviceWriterAsync=1 DeviceNAL=1: the same .264 and recon file"""
    w, h, n = 176, 144, 3
    pics = tensor_seq(w, h, n, 101, U8)
    common = ["FramesToBeEncoded=3", f"SourceWidth={w}", f"SourceHeight={h}", "SearchRange=16", "DeviceInput=1", "DeviceCAVLC=1",
              "DeviceWriterAsync=1", "DeviceNAL=1"]
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b, tempfile.TemporaryDirectory() as c:
        with open(f"{a}/in.rgb", "wb") as f:
            for p in pics:
                f.write(np.stack(p, axis=-1).tobytes())
        with open(f"{b}/in.gbrpf32le", "wb") as f:
            for p in pics:
                planes = [(p[i].astype(np.float32) / np.float32(255)) for i in (1, 2, 0)]          # G, B, R
                assert all(np.array_equal(tr.quantise(x, F32, 8), p[i]) for x, i in zip(planes, (1, 2, 0)))
                for x in planes:
                    f.write(x.astype("<f4").tobytes())
        with open(f"{c}/in.yuv", "wb") as f:
            for p in pics:
                for plane in tr.convert_source_size(p, U8, BT709, 8):
                    f.write(plane.tobytes())
        la = run_lencod(LENCOD, a, common + [f"InputFile={a}/in.rgb", "DeviceInputTensor=1", "DeviceInputMatrix=1"])
        assert "the source is an RGB tensor, rgb24" in la and "BT.709" in la and "pushed from device memory" in la
        lb = run_lencod(LENCOD, b, common + [f"InputFile={b}/in.gbrpf32le", "DeviceInputTensor=4", "DeviceInputMatrix=1"])
        assert "the source is an RGB tensor, gbrpf32le" in lb
        lc = run_lencod(LENCOD, c, common + [f"InputFile={c}/in.yuv"])
        assert "RGB tensor" not in lc and "pushed from device memory" in lc
        want = open(f"{c}/a.264", "rb").read()
        assert len(want) > 100 and open(f"{a}/a.264", "rb").read() == want and open(f"{b}/a.264", "rb").read() == want
        rec = open(f"{c}/rec.yuv", "rb").read()
        assert open(f"{a}/rec.yuv", "rb").read() == rec and open(f"{b}/rec.yuv", "rb").read() == rec
