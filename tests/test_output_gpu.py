"""Decoded pictures pulled on the device (include/jmhip_output.h): k_pull_picture and
k_pull_tensor write the top-left crop of the current picture, deblocked or not, into device memory of
the caller as YUV planes, packed RGB or an RGB tensor.

The reference is tests/output_ref.py: numpy from the formulas (coefficients by Fraction, int64
conversion, float32 division), held against csrc/jmh_output.h in tests/test_output_core.py.  Every
check is exact.  Every destination is filled with a canary first; after the call every byte that is
not a destination element must still be the canary: row padding, the fourth channel of HWC4, 64 bytes
in front and 64 bytes behind."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import output_ref as oref
import tensor_ref as tr
from jmpaths import LENCOD, ensure_built, load_jmhip
from test_gpu_parity import run_lencod
from test_ingest_gpu import seq
from test_output_core import KINDS, SIZES, expected_block, tensor_layout

jmhip = load_jmhip()
pytestmark = pytest.mark.gpu

I, P = jmhip.JMH_I_SLICE, jmhip.JMH_P_SLICE
DBK_OUT, REC_OUT = jmhip.JMH_OUT_DEBLOCKED, jmhip.JMH_OUT_RECON
DBK = (0, 0, 0)
CANARY, GUARD = 0xA5, 64
PICTURE_CASES = [(fmt, bd) for bd in (8, 9, 10) for fmt in oref.YUV_FORMATS[bd] + oref.RGB_FORMATS.get(bd, ())]


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


@pytest.fixture(scope="module")
def content():
    """the random full-range-of-code YUV planes of every (coded size, bit depth), made once"""
    rng = np.random.default_rng(77)
    return {(cw, ch, bd): oref.random_yuv(rng, cw, ch, bd) for (cw, ch) in SIZES for bd in (8, 9, 10)}


class Block:
    """a device block of a layout's bytes, filled with the canary"""

    def __init__(self, enc, layout, stream=None):
        self.enc, self.layout = enc, layout
        self.base = enc.device_alloc(layout.nbytes)
        enc.device_upload(self.base, np.full(layout.nbytes, CANARY, np.uint8), stream)

    def dst(self, stream=None):
        return self.layout.at(self.base, stream)

    def read(self, stream=None):
        return self.enc.device_download(self.base, self.layout.nbytes, stream)

    def free(self):
        self.enc.device_free(self.base)


def assert_block(got, layout, ref, what):
    """the block holds the reference in its elements and the canary everywhere else"""
    want = expected_block(layout, ref, CANARY)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        stray = bad[~layout.mask()[bad]]
        assert False, f"{what}: {len(bad)} bytes differ, first at {bad[:6].tolist()}; {len(stray)} of them are not destination elements ({stray[:6].tolist()})"


def many_blocks(w, h):
    """a crop that can clamp every component on both sides: one chroma pair cannot (at full range
    R = Y + 1.4 f leaves [0, M] on one side only, whatever Y is); from two blocks up the planted blocks
    of output_ref.random_yuv do"""
    return (w // 2) * (h // 2) >= 2


# ---- 1: the seam --------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,bd", PICTURE_CASES, ids=[f"{oref.NAMES[f]}_{b}" for f, b in PICTURE_CASES])
def test_picture_seam_equals_reference(contexts, content, fmt, bd):
    """enc.convert == output_ref.picture, bit-exactly, and nothing else is written.  Every crop with
    row strides tight / +es / +52 es crossed with plane bases 0 / es / 4 / 12 bytes off a 256-byte
    boundary (the 16-byte stores, the dword stores, the element stores); for RGB the four flag sets
    rotate through the combinations: they only change the kernel's arguments.  Condition, asserted on
    the reference alone: in every RGB case a sample clamped at 0 and one clamped at M in each of R, G
    and B (a 2x2 crop has one chroma pair and cannot hold it at full range: there, R, G and B each
    clamp on one side)."""
    rgb = fmt >= oref.BGRA8
    es = 4 if rgb else 2 if fmt >= oref.I010 else 1
    n = 0
    for (cw, ch), crops in SIZES.items():
        enc, pics = contexts(cw, ch, bd), content[(cw, ch, bd)]
        for w, h in crops:
            want = {}
            for fl in (oref.FLAGS if rgb else (0,)):
                counts = {}
                want[fl] = oref.picture(pics, w, h, fmt | fl, bd, counts)
                if rgb:
                    assert oref.clamps_everywhere(counts) if many_blocks(w, h) else all(a + b > 0 for a, b in zip(counts["lo"], counts["hi"])), (w, h, fl, counts)
            combos = [(pad, mis) for pad in (0, es, 52 * es) for mis in sorted({0, es, 4, 12})]
            for i, (pad, mis) in enumerate(combos):
                fl = oref.FLAGS[(i + i // 4) % 4] if rgb else 0
                blk = Block(enc, jmhip.out_layout(fmt | fl, w, h, pad_stride=pad, misalign=mis, guard=GUARD))
                try:
                    enc.convert(*pics, blk.dst())
                    got = blk.read()
                finally:
                    blk.free()
                assert_block(got, blk.layout, want[fl], f"{oref.NAMES[fmt]} at {bd} bits, flags {fl:#x}, {w}x{h} of {cw}x{ch}, stride +{pad}, base +{mis}")
                n += 1
    assert n == 7 * 3 * len({0, es, 4, 12})


@pytest.mark.parametrize("dtype,bd", tr.PAIRS, ids=[f"{tr.NAMES[d]}_{b}" for d, b in tr.PAIRS])
def test_tensor_seam_equals_reference(contexts, content, dtype, bd):
    """enc.convert_tensor == output_ref.tensor, bit-exactly, in CHW, HWC3, HWC4 and BGR, with the same
    strides, bases, rotation of the flag sets and condition; the fourth channel of HWC4 keeps the canary"""
    es = tr.ES[dtype]
    n = 0
    for (cw, ch), crops in SIZES.items():
        enc, pics = contexts(cw, ch, bd), content[(cw, ch, bd)]
        for w, h in crops:
            want = {}
            for fl in oref.FLAGS:
                counts = {}
                want[fl] = oref.tensor(pics, w, h, dtype, fl, bd, counts)
                assert oref.clamps_everywhere(counts) if many_blocks(w, h) else all(a + b > 0 for a, b in zip(counts["lo"], counts["hi"])), (w, h, fl, counts)
            for kind in KINDS:
                combos = [(pad, mis) for pad in (0, es, 52 * es) for mis in sorted({0, es, 4, 12})]
                for i, (pad, mis) in enumerate(combos):
                    fl = oref.FLAGS[(i + i // 4) % 4]
                    blk = Block(enc, tensor_layout(jmhip, dtype, w, h, kind, fl, pad, mis, GUARD))
                    try:
                        enc.convert_tensor(*pics, blk.dst())
                        got = blk.read()
                    finally:
                        blk.free()
                    assert_block(got, blk.layout, want[fl], f"{tr.NAMES[dtype]} at {bd} bits, {kind}, flags {fl:#x}, {w}x{h} of {cw}x{ch}, stride +{pad}, base +{mis}")
                    n += 1
    assert n == 7 * 4 * 3 * len({0, es, 4, 12})


# ---- 2: every level through the kernel ----------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_every_level_through_the_kernel(bd):
    """Y = 0..M along the rows of a 1024x16 picture, U = V = Co, full range: iy = 16384, so R = G = B
    = Y exactly.  Every float type returns the M + 1 bit patterns of jmh_tensor_dequantise (which are
    those of the numpy definition), U8 / U16 return q."""
    m = (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8
    q = (np.arange(1024 * 16) % (m + 1)).reshape(16, 1024)
    y, c = q.astype(dt), np.full((8, 512), 1 << (bd - 1), dt)
    enc = jmhip.Encoder(1024, 16, search_range=8, bit_depth=bd)
    try:
        for dtype, dbd in tr.PAIRS:
            if dbd != bd:
                continue
            level = jmhip.tensor_dequantise(np.arange(m + 1, dtype=np.int32), dtype, bd)
            assert level.tobytes() == oref.dequantise(np.arange(m + 1), dtype, bd).tobytes()
            blk = Block(enc, jmhip.out_tensor_layout(dtype, 1024, 16, flags=oref.FULL_RANGE, guard=GUARD))
            try:
                enc.convert_tensor(y, c, c, blk.dst())
                got = blk.read()
            finally:
                blk.free()
            assert_block(got, blk.layout, [level[q]] * 3, f"{tr.NAMES[dtype]} at {bd} bits")
    finally:
        enc.close()


# ---- 3: the argument rules on a live context ----------------------------------------------------
def test_argument_rules_on_a_live_context(contexts):
    """every rule of include/jmhip_output.h with its status, through the pull and the seam alike; the
    canary destination stays untouched, and a valid pull afterwards works"""
    e8, e9, e10 = contexts(32, 32, 8), contexts(32, 32, 9), contexts(32, 32, 10)
    UNSUP, INVAL, STATE, OK = jmhip.JMH_E_UNSUPPORTED_CFG, jmhip.JMH_E_INVALID_ARG, jmhip.JMH_E_STATE, jmhip.JMH_OK
    rng = np.random.default_rng(5)
    pics = {8: oref.random_yuv(rng, 32, 32, 8), 9: oref.random_yuv(rng, 32, 32, 9), 10: oref.random_yuv(rng, 32, 32, 10)}
    nbytes = 3 * 32 * 32 * 4 + 256
    bases = {enc: enc.device_alloc(nbytes) for enc in (e8, e9, e10)}
    try:
        for enc, base in bases.items():
            enc.device_upload(base, np.full(nbytes, CANARY, np.uint8))

        def good_tensor(enc, dtype):
            es = tr.ES[dtype]
            return jmhip.DeviceTensorOut(dtype, 0, 30, 18, [bases[enc] + i * 32 * 32 * es for i in range(3)], es, 32 * es)

        def good_picture(enc, fmt):
            es = 4 if fmt >= 16 else 2 if fmt >= 2 else 1
            return jmhip.DevicePictureOut(fmt, 30, 18, [bases[enc], bases[enc] + 4096, bases[enc] + 8192], [32 * es] * 3)

        def status(enc, d, which=DBK_OUT, seam=True, **change):
            for k, v in change.items():
                setattr(d, k, v)
            tensor = isinstance(d, jmhip.DeviceTensorOut)
            codes = []
            for pull in (True, False) if seam else (True,):
                try:
                    if pull:
                        (enc.pull_tensor if tensor else enc.pull)(d, which)
                    else:
                        (enc.convert_tensor if tensor else enc.convert)(*pics[enc.cfg.bit_depth], d)
                    codes.append(OK)
                except jmhip.JmhError as e:
                    codes.append(e.status)
            return codes

        # before the first pop there is no current picture: an invalid descriptor is still INVALID_ARG, a valid one STATE
        assert status(e8, good_tensor(e8, tr.U8)) == [STATE, OK] and status(e8, good_picture(e8, oref.NV12)) == [STATE, OK]
        assert status(e8, good_tensor(e8, tr.U8), width=29) == [INVAL, INVAL]
        for enc in (e8, e9, e10):
            enc.device_upload(bases[enc], np.full(nbytes, CANARY, np.uint8))
            enc.push(*pics[enc.cfg.bit_depth], I, 28, deblock=DBK)
            enc.pop()
        both = lambda c: [c, c]
        # a valid destination in the wrong context
        assert status(e10, good_tensor(e10, tr.U8)) == both(UNSUP) and status(e8, good_tensor(e8, tr.U16)) == both(UNSUP)
        for dt in tr.DTYPES:
            assert status(e9, good_tensor(e9, dt)) == both(UNSUP), dt
        for fmt in (oref.BGRA8, oref.RGBA8, oref.RGB10A2, oref.BGR10A2, oref.I420, oref.NV12, oref.P010):
            assert status(e9, good_picture(e9, fmt)) == both(UNSUP), fmt
        for fmt in (oref.I010, oref.P010, oref.RGB10A2, oref.BGR10A2):
            assert status(e8, good_picture(e8, fmt)) == both(UNSUP), fmt
        for fmt in (oref.I420, oref.NV12, oref.BGRA8, oref.RGBA8):
            assert status(e10, good_picture(e10, fmt)) == both(UNSUP), fmt
        # the argument rules, before the bit depth is looked at
        for enc in (e8, e10):
            for dt in tr.DTYPES:
                es = tr.ES[dt]
                g = lambda: good_tensor(enc, dt)
                ch = g().chans
                assert status(enc, g(), dtype=5) == both(INVAL) and status(enc, g(), dtype=-1) == both(INVAL)
                for fl in (1, 1 << 7, 1 << 10, 16, oref.BT709 | 1, -1):
                    assert status(enc, g(), flags=fl) == both(INVAL), fl
                assert status(enc, g(), width=29) == both(INVAL) and status(enc, g(), height=17) == both(INVAL)
                assert status(enc, g(), width=0) == both(INVAL) and status(enc, g(), height=0) == both(INVAL)
                assert status(enc, g(), width=34, stride_y=64 * es) == both(INVAL) and status(enc, g(), height=34) == both(INVAL)
                assert status(enc, g(), stride_x=0) == both(INVAL) and status(enc, g(), stride_x=-es, stride_y=64 * es) == both(INVAL)
                assert status(enc, g(), stride_y=29 * es) == both(INVAL) and status(enc, g(), stride_y=-32 * es) == both(INVAL)
                assert status(enc, g(), stride_x=3 * es, stride_y=29 * 3 * es) == both(INVAL)
                for i in range(3):
                    assert status(enc, g(), chans=[None if j == i else c for j, c in enumerate(ch)]) == both(INVAL)
                    if es > 1:
                        assert status(enc, g(), chans=[c + 1 if j == i else c for j, c in enumerate(ch)]) == both(INVAL)
                if es > 1:
                    assert status(enc, g(), stride_y=32 * es + 1) == both(INVAL) and status(enc, g(), stride_x=es + 1, stride_y=64 * es) == both(INVAL)
                if es > 2:
                    assert status(enc, g(), chans=[ch[0] + 2, ch[1], ch[2]]) == both(INVAL)
                assert status(enc, g(), which=2, seam=False) == [INVAL] and status(enc, g(), which=-1, seam=False) == [INVAL]
            for fmt in (oref.I420, oref.NV12, oref.I010, oref.P010, oref.BGRA8, oref.RGBA8, oref.RGB10A2, oref.BGR10A2):
                g = lambda: good_picture(enc, fmt)
                es, b = (4 if fmt >= 16 else 2 if fmt >= 2 else 1), bases[enc]
                assert status(enc, g(), width=29) == both(INVAL) and status(enc, g(), height=17) == both(INVAL) and status(enc, g(), width=0) == both(INVAL)
                assert status(enc, g(), width=34, strides=[256] * 3) == both(INVAL) and status(enc, g(), height=34) == both(INVAL)
                assert status(enc, g(), planes=[None, b, b]) == both(INVAL) and status(enc, g(), strides=[30 * es - es, 256, 256]) == both(INVAL)
                assert status(enc, g(), strides=[-256, 256, 256]) == both(INVAL) and status(enc, g(), format=fmt | 1 << 10) == both(INVAL)
                if fmt < 16:
                    assert status(enc, g(), format=fmt | oref.BT709) == both(INVAL) and status(enc, g(), format=fmt | oref.FULL_RANGE) == both(INVAL)
                    assert status(enc, g(), planes=[b, None, b]) == both(INVAL)
                    assert status(enc, g(), strides=[256, (30 if fmt in (oref.NV12, oref.P010) else 15) * es - es, 256]) == both(INVAL)
                    if fmt in (oref.I420, oref.I010):
                        assert status(enc, g(), planes=[b, b, None]) == both(INVAL)
                if es > 1:
                    assert status(enc, g(), planes=[b + 1, b + 4096, b + 8192]) == both(INVAL) and status(enc, g(), strides=[256 + 1] * 3) == both(INVAL)
                if es > 2:
                    assert status(enc, g(), planes=[b + 2, b, b]) == both(INVAL) and status(enc, g(), strides=[256 + 2] * 3) == both(INVAL)
                assert status(enc, g(), which=2, seam=False) == [INVAL]
            for fmt in (4, 15, 20, -1):
                assert status(enc, good_picture(enc, oref.I420), format=fmt) == both(INVAL), fmt
            # nothing was written by any of them
            assert (enc.device_download(bases[enc], nbytes) == CANARY).all()
        # what is valid: planes that are not read may be null, the least strides, one address three times
        assert status(e8, good_picture(e8, oref.NV12), planes=[bases[e8], bases[e8] + 4096, None], strides=[30, 30, 0]) == both(OK)
        assert status(e8, good_picture(e8, oref.BGRA8 | oref.BT709), planes=[bases[e8], None, None], strides=[120, 0, 0]) == both(OK)
        assert status(e10, good_picture(e10, oref.P010), planes=[bases[e10], bases[e10] + 4096, None], strides=[60, 60, -1]) == both(OK)
        assert status(e9, good_picture(e9, oref.I010)) == both(OK)
        assert status(e8, good_tensor(e8, tr.F16), stride_x=6, stride_y=29 * 6 + 2, chans=[bases[e8], bases[e8] + 2, bases[e8] + 4]) == both(OK)
        assert status(e10, good_tensor(e10, tr.U16), which=REC_OUT) == both(OK)
        # and a valid pull still gives the picture
        L = jmhip.out_tensor_layout(tr.U8, 30, 18, guard=GUARD)
        blk = Block(e8, L)
        try:
            e8.pull_tensor(blk.dst())
            assert_block(blk.read(), L, oref.tensor(e8.deblocked(), 30, 18, tr.U8, 0, 8), "a valid pull after the refused ones")
        finally:
            blk.free()
    finally:
        for enc, base in bases.items():
            enc.device_free(base)


# ---- 4: the pipeline ----------------------------------------------------------------------------
W, H, QP = 64, 48, 28


def run_pipeline(coded, pull):
    """I, P, P of 64x48 at depth 2.  coded: push_coded_tensor + pop_coded, else push + pop.  Returns
    the stream (per picture: the slices' bytes, or the results' bytes); with pull, after each pop the
    deblocked picture as F16 CHW and the reconstruction as NV12 are checked against output_ref."""
    pics = seq(W, H, 3, 23)
    kw = dict(search_range=8, pipeline_depth=2)
    enc = jmhip.Encoder(W, H, **kw)
    LT = jmhip.out_tensor_layout(tr.F16, 50, 34, flags=oref.BT709, pad_stride=4, guard=GUARD)
    LP = jmhip.out_layout(oref.NV12, 64, 48, misalign=1, guard=GUARD)
    out, pending, blocks, src, stream = [], 0, [], [], None

    def check(i):
        bt, bp = Block(enc, LT, stream), Block(enc, LP)
        blocks.extend([bt, bp])
        enc.pull_tensor(bt.dst(stream))                       # the deblocked picture, on a stream of the caller's
        enc.pull(bp.dst(), REC_OUT)                           # the reconstruction, complete on return
        got_p, got_t = bp.read(), bt.read(stream)
        assert_block(got_t, LT, oref.tensor(enc.deblocked(), 50, 34, tr.F16, oref.BT709, 8), f"picture {i}: deblocked as F16 CHW")
        assert_block(got_p, LP, oref.picture(enc.recon(), 64, 48, oref.NV12, 8), f"picture {i}: recon as NV12")

    def pop(i):
        if coded:
            data, where, stats = enc.pop_coded()
            assert stats["fallback"] == 0
            out.append(b"".join(data))
        else:
            res, _ = enc.pop()
            out.append(res.tobytes())
        if pull:
            check(i)
    try:
        if pull:
            stream = enc.device_stream()
            spare = Block(enc, LP)
            blocks.append(spare)
            for call in (lambda: enc.pull_tensor(jmhip.out_tensor_layout(tr.U8, 2, 2).at(spare.base)), lambda: enc.pull(spare.dst(), REC_OUT)):   # before the first pop
                with pytest.raises(jmhip.JmhError) as e:
                    call()
                assert e.value.status == jmhip.JMH_E_STATE
        if coded:                                             # the same pictures as RGB tensors: what codes them is not the point
            rgb = [[np.ascontiguousarray(a.astype(np.uint8)) for a in oref.to_rgb(*p, 0, 8)] for p in pics]
            src = [enc.device_tensor(jmhip.to_device_tensor(np.stack(c), "chw")) for c in rgb]
        popped = 0
        for i in range(3):
            if i:
                enc.set_reference_slot(-2)
            if pending == enc.depth:
                pop(popped)
                popped, pending = popped + 1, pending - 1
            st = I if i == 0 else P
            if coded:
                enc.push_coded_tensor(src[i], st, QP, jmhip.coded_slice_descs(enc.mbw * enc.mbh, st, QP, 5), deblock=DBK)
            else:
                enc.push(*pics[i], st, QP, deblock=DBK)
            pending += 1
        while pending:
            pop(popped)
            popped, pending = popped + 1, pending - 1
        if pull:                                              # a picture pushed without deblocking has no deblocked picture
            enc.push(*pics[0], I, QP)
            enc.pop()
            with pytest.raises(jmhip.JmhError) as e:
                enc.pull(spare.dst())
            assert e.value.status == jmhip.JMH_E_STATE
            enc.pull(spare.dst(), REC_OUT)
            assert_block(spare.read(), LP, oref.picture(enc.recon(), 64, 48, oref.NV12, 8), "recon of a picture that was not deblocked")
            enc.output_wait()
        return out
    finally:
        if stream:
            enc.device_stream_destroy(stream)
        for b in blocks:
            b.free()
        for s in src:
            enc.device_free(s.base)
        enc.close()


@pytest.mark.parametrize("coded", [True, False], ids=["coded_tensor", "ordinary"])
def test_pipeline_pulls_equal_reference_and_leave_the_stream_alone(coded):
    with_pull, without = run_pipeline(coded, True), run_pipeline(coded, False)
    assert len(with_pull) == 3 and with_pull == without and all(len(b) > 50 for b in without)


# ---- 5: reuse of the entry ----------------------------------------------------------------------
def test_entry_is_not_rewritten_under_a_pull():
    """a pull queued on a caller's stream, then ring_entries further pictures pushed and popped
    without output_wait (the entry the pull read gets its next occupant on the way), then the
    download: the bytes are the reference of the pulled picture.  The claim's wait on the entry's event
    is exercised here; that it orders the two is argued in DESIGN.md §5.10."""
    pics = seq(W, H, 4, 29)
    enc = jmhip.Encoder(W, H, search_range=8, pipeline_depth=2)
    L = jmhip.out_tensor_layout(tr.F32, 64, 48, "hwc", channels=4, guard=GUARD)
    blk = stream = None
    try:
        stream = enc.device_stream()
        blk = Block(enc, L, stream)
        enc.push(*pics[0], I, QP, deblock=DBK)
        enc.pop()
        want = oref.tensor(enc.deblocked(), 64, 48, tr.F32, 0, 8)
        enc.pull_tensor(blk.dst(stream))
        n = enc.ring_entries
        assert n >= 2
        for i in range(1, n + 1):
            enc.set_reference_slot(-2)
            enc.push(*pics[i % len(pics)], P, QP, deblock=DBK)
            enc.pop()
        assert_block(blk.read(stream), L, want, "the pulled picture after its entry was claimed again")
    finally:
        if stream:
            enc.device_stream_destroy(stream)
        if blk:
            blk.free()
        enc.close()


# ---- 6: torch -----------------------------------------------------------------------------------
def test_torch_tensors_through_to_torch_and_into_torch():
    """enc.to_torch(torch.float16, "chw") and enc.into_torch of a strided HWC view equal the reference,
    and the returned tensor pushed again with enc.from_torch gives, through ingest_tensor, the planes
    tensor_ref.convert gives for the reference tensor.  In a child process (tests/output_torch_child.py):
    torch must be imported before libjmhip.so is loaded for the two to share one HIP runtime."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "output_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    if r.returncode == 0 and "SKIP:" in r.stdout:
        pytest.skip(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and "torch output: OK" in r.stdout, (r.stdout + r.stderr)[-4000:]


# ---- 7: lencod ----------------------------------------------------------------------------------
def test_lencod_device_recon_file():
    """3 frames of 64x48 with DeviceReconFormat=16 and with DeviceReconTensor=2: ReconFile equals
    output_ref applied to the YUV ReconFile of the same run without the key; the .264 files are identical"""
    w, h, n = 64, 48, 3
    common = ["InputFile=synthetic:5", f"FramesToBeEncoded={n}", f"SourceWidth={w}", f"SourceHeight={h}", "SearchRange=8"]
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b, tempfile.TemporaryDirectory() as c:
        la = run_lencod(LENCOD, a, common + ["DeviceReconFormat=16", "DeviceReconMatrix=1"])
        assert "ReconFile holds RGB, format 16" in la and "BT.709" in la
        lb = run_lencod(LENCOD, b, common + ["DeviceReconTensor=2", "DeviceReconFullRange=1"])
        assert "ReconFile holds an RGB tensor, gbrp" in lb and "full range" in lb
        lc = run_lencod(LENCOD, c, common)
        assert "ReconFile holds" not in lc
        stream = open(f"{c}/a.264", "rb").read()
        assert len(stream) > 100 and open(f"{a}/a.264", "rb").read() == stream and open(f"{b}/a.264", "rb").read() == stream
        yuv = np.fromfile(f"{c}/rec.yuv", np.uint8)
        assert yuv.size == n * w * h * 3 // 2
        bgra, gbrp = np.fromfile(f"{a}/rec.yuv", np.uint32), np.fromfile(f"{b}/rec.yuv", np.uint8)
        assert bgra.size == n * w * h and gbrp.size == n * 3 * w * h
        for i in range(n):
            f = yuv[i * w * h * 3 // 2:(i + 1) * w * h * 3 // 2]
            pics = (f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2))
            assert np.array_equal(bgra[i * w * h:(i + 1) * w * h].reshape(h, w), oref.picture(pics, w, h, oref.BGRA8 | oref.BT709, 8)[0]), f"frame {i}: BGRA8"
            r, g, bl = oref.tensor(pics, w, h, tr.U8, oref.FULL_RANGE, 8)
            assert np.array_equal(gbrp[i * 3 * w * h:(i + 1) * 3 * w * h].reshape(3, h, w), np.stack([g, bl, r])), f"frame {i}: gbrp"


@pytest.mark.parametrize("keys,recon", [
    (["DeviceCAVLC=1", "DeviceWriterAsync=1"], "DeviceReconTensor=1"),
    (["PipelineDepth=1"], "DeviceReconFormat=17"),
], ids=["coded_pop_rgb24", "one_picture_at_a_time_rgba8"])
def test_lencod_device_recon_file_on_the_other_frame_loops(keys, recon):
    """the same through the frame loop of coded pictures (the pop returns bytes and SSDs only) and through
    the unpipelined one: ReconFile == output_ref of the YUV ReconFile of the run without the key"""
    w, h, n = 64, 48, 3
    common = ["InputFile=synthetic:6", f"FramesToBeEncoded={n}", f"SourceWidth={w}", f"SourceHeight={h}", "SearchRange=8"] + keys
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as c:
        run_lencod(LENCOD, a, common + [recon])
        run_lencod(LENCOD, c, common)
        assert open(f"{a}/a.264", "rb").read() == open(f"{c}/a.264", "rb").read()
        yuv = np.fromfile(f"{c}/rec.yuv", np.uint8).reshape(n, w * h * 3 // 2)
        got = np.fromfile(f"{a}/rec.yuv", np.uint8).reshape(n, -1)
        for i, f in enumerate(yuv):
            pics = (f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2))
            if recon.endswith("Tensor=1"):
                want = np.stack(oref.tensor(pics, w, h, tr.U8, 0, 8), axis=-1)
            else:
                want = oref.picture(pics, w, h, oref.RGBA8, 8)[0]
            assert got[i].tobytes() == np.ascontiguousarray(want).tobytes(), f"frame {i}"
