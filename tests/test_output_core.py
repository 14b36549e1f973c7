"""Decoded pictures pulled on the device (include/jmhip_output.h), the parts that need
no GPU: the coefficients against their derivation by Fraction, the dequantiser against its numpy
definition on every level, the inverse conversion against the forward one over the RGB cube, the
reference walk of csrc/jmh_output.h against tests/output_ref.py, the additive ABI, the lencod keys.

tests/harness/output_check.c is a stand-alone C program built from the header with
-fsanitize=address,undefined -fno-sanitize-recover and run directly: it walks every case into a malloc
block of exactly the destination's bytes, so one stray byte is a report, and runs the argument rules."""
import ctypes
import fcntl
import os
import re
import subprocess

import numpy as np
import pytest

import output_ref as oref
import tensor_ref as tr
from jmpaths import HARNESS, HEADER, LENCOD, LENCOD_CPU, LIBJMHIP, ensure_built, load_jmhip

ASAN = os.path.join(HARNESS, "_build_asan")
CHECK = os.path.join(ASAN, "output_check")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
# coded size -> crops: the sizes of tests/test_output_gpu.py
SIZES = {(48, 32): [(34, 18)], (32, 32): [(2, 2), (30, 2), (2, 30), (32, 32)], (1056, 32): [(1042, 18), (1040, 18)]}
KINDS = ("chw", "hwc3", "hwc4", "bgr")


def tensor_layout(jm, dtype, w, h, kind, flags=0, pad=0, mis=0, guard=0):
    """the OutTensorLayout of one of KINDS: planar, interleaved with 3 or 4 channels, interleaved B, G, R"""
    lay, order, ch = {"chw": ("chw", "rgb", 3), "hwc3": ("hwc", "rgb", 3), "hwc4": ("hwc", "rgb", 4), "bgr": ("hwc", "bgr", 3)}[kind]
    return jm.out_tensor_layout(dtype, w, h, lay, order, ch, flags, pad, mis, guard)


def expected_block(layout, arrays, canary=0xA5):
    """the bytes of a destination block that holds the reference arrays and the canary everywhere else"""
    buf = np.full(layout.nbytes, canary, np.uint8)
    if hasattr(layout, "stride_x"):
        es = arrays[0].dtype.itemsize
        for o, a in zip(layout.offsets, arrays):
            view = np.lib.stride_tricks.as_strided(buf[o:], (layout.height, layout.width, es), (layout.stride_y, layout.stride_x, 1))
            view[:] = np.ascontiguousarray(a).view(np.uint8).reshape(layout.height, layout.width, es)
    else:
        for o, st, a in zip(layout.offsets, layout.strides, arrays):
            rb = a.shape[1] * a.dtype.itemsize
            np.lib.stride_tricks.as_strided(buf[o:], (a.shape[0], rb), (st, 1))[:] = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], rb)
    return buf


@pytest.fixture(scope="module")
def checker():
    with open(os.path.join(HARNESS, ".sanitize.lock"), "w") as lk:       # one sanitizer build at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", HARNESS, "-f", "output.mk"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("output_check build failed:\n" + r.stdout + r.stderr)
    return CHECK


# ---- 1: the coefficients ----
def test_coefficients_equal_the_fraction_derivation_and_the_table():
    ensure_built()
    jm = load_jmhip()
    n = 0
    for matrix in (0, 1):
        for full in (0, 1):
            for bd in (8, 10):
                flags = (oref.BT709 if matrix else 0) | (oref.FULL_RANGE if full else 0)
                got = jm.yuv_coefficients(flags, bd)
                m = (1 << bd) - 1
                assert got == oref.coefficients(flags, bd), (matrix, full, bd)
                assert got[:5] == oref.TABLE[(matrix, bd, full)] and got[5:] == [0 if full else 16 << (bd - 8), 1 << (bd - 1), m]
                assert max(abs(c) for c in got[:5]) <= 34711
                n += 1
    assert n == 8
    lib, out = jm.load(), (ctypes.c_int32 * 8)()
    INVAL = jm.JMH_E_INVALID_ARG
    assert lib.jmh_yuv_coefficients(0, 9, out) == INVAL and lib.jmh_yuv_coefficients(0, 12, out) == INVAL and lib.jmh_yuv_coefficients(0, 0, out) == INVAL
    for fl in (1, 1 << 7, 1 << 10, 16, oref.BT709 | 1, -1):
        assert lib.jmh_yuv_coefficients(fl, 8, out) == INVAL, fl
    assert lib.jmh_yuv_coefficients(0, 8, None) == INVAL
    assert lib.jmh_yuv_coefficients(oref.BT709 | oref.FULL_RANGE, 10, out) == jm.JMH_OK


# ---- 2: the dequantiser ----
@pytest.mark.parametrize("dtype,bd", tr.PAIRS, ids=[f"{tr.NAMES[d]}_{b}" for d, b in tr.PAIRS])
def test_dequantiser_every_level(dtype, bd):
    """jmh_tensor_dequantise == the numpy definition bit for bit on every q in 0..M; the round trip
    through jmh_tensor_quantise is the identity for every pair but (BF16, 10), which is not"""
    ensure_built()
    jm = load_jmhip()
    m = (1 << bd) - 1
    q = np.arange(m + 1, dtype=np.int32)
    got = jm.tensor_dequantise(q, dtype, bd)
    want = oref.dequantise(q, dtype, bd)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert np.array_equal(tr.quantise(want, dtype, bd), jm.tensor_quantise(got, dtype, bd))
    back = jm.tensor_quantise(got, dtype, bd)
    if (dtype, bd) == (tr.BF16, 10):
        assert int((back != q).sum()) == 511                   # eight significand bits do not hold 1024 levels
    else:
        assert np.array_equal(back, q)
    # out-of-range components are clamped, not wrapped
    assert jm.tensor_dequantise(np.array([-5, m + 7], np.int32), dtype, bd).tobytes() == want[[0, m]].tobytes()


def test_dequantiser_status_codes():
    ensure_built()
    jm = load_jmhip()
    lib = jm.load()
    q, e = (ctypes.c_int32 * 4)(), (ctypes.c_uint32 * 4)()
    UNSUP, INVAL, OK = jm.JMH_E_UNSUPPORTED_CFG, jm.JMH_E_INVALID_ARG, jm.JMH_OK
    for dt, bd, want in ((0, 10, UNSUP), (1, 8, UNSUP), (0, 9, UNSUP), (2, 9, UNSUP), (4, 9, UNSUP), (4, 12, UNSUP), (5, 8, INVAL), (-1, 8, INVAL),
                         (0, 8, OK), (1, 10, OK), (2, 8, OK), (3, 10, OK), (4, 8, OK), (4, 10, OK)):
        assert lib.jmh_tensor_dequantise(dt, bd, q, 4, e) == want, (dt, bd)
    assert lib.jmh_tensor_dequantise(4, 8, None, 4, e) == INVAL and lib.jmh_tensor_dequantise(4, 8, q, 4, None) == INVAL
    assert lib.jmh_tensor_dequantise(4, 8, None, 0, None) == OK


# ---- 3: the inverse inverts ----
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("flags", oref.FLAGS, ids=["601", "709", "601full", "709full"])
def test_inverse_inverts_the_forward_conversion(flags, bd):
    """forward: jmh_rgb_coefficients on flat 2x2 blocks (the sums are 4 R, 4 G, 4 B); inverse:
    jmh_yuv_coefficients; both from the library.  The whole 8-bit cube, the lattice {0, 9, ..., 1017,
    1023}^3 at 10 bits: |error| <= 2 per channel at limited range, <= 1 at full range."""
    ensure_built()
    jm = load_jmhip()
    m = (1 << bd) - 1
    c = jm.rgb_coefficients((jm.JMH_PIX_RGBA8 if bd == 8 else jm.JMH_PIX_RGB10A2) | flags, bd)
    iy, irv, igu, igv, ibu, yo, co, mm = jm.yuv_coefficients(flags, bd)
    assert mm == m == c[11] and yo == c[9] and co == c[10]
    v = np.arange(0, m + 1, 1 if bd == 8 else 9, dtype=np.int64)
    if v[-1] != m:
        v = np.append(v, m)
    R, G, B = np.meshgrid(v, v, v, indexing="ij")
    Y = np.clip(yo + ((c[0] * R + c[1] * G + c[2] * B + (1 << 13)) >> 14), 0, m)
    U = np.clip(co + ((c[3] * 4 * R + c[4] * 4 * G + c[5] * 4 * B + (1 << 15)) >> 16), 0, m)
    V = np.clip(co + ((c[6] * 4 * R + c[7] * 4 * G + c[8] * 4 * B + (1 << 15)) >> 16), 0, m)
    r = np.clip((iy * (Y - yo) + irv * (V - co) + (1 << 13)) >> 14, 0, m)
    g = np.clip((iy * (Y - yo) + igu * (U - co) + igv * (V - co) + (1 << 13)) >> 14, 0, m)
    b = np.clip((iy * (Y - yo) + ibu * (U - co) + (1 << 13)) >> 14, 0, m)
    bound = 1 if flags & oref.FULL_RANGE else 2
    errs = [int(np.abs(a - A).max()) for a, A in ((r, R), (g, G), (b, B))]
    print(f"flags {flags:#x}, {bd} bits: max |error| R, G, B = {errs}")
    assert max(errs) <= bound, errs


# ---- 4: the reference walk of csrc/jmh_output.h ----
def walk_cases(jm):
    """(record header words, source planes, layout, reference arrays) for every case"""
    rng = np.random.default_rng(2024)
    n = 0
    for (cw, ch), crops in SIZES.items():
        for bd in (8, 9, 10):
            pics = oref.random_yuv(rng, cw, ch, bd)
            for w, h in crops:
                for pad_i, pad in enumerate((0, 1, 52)):
                    for fmt in oref.YUV_FORMATS[bd]:
                        es = 2 if fmt >= oref.I010 else 1
                        L = jm.out_layout(fmt, w, h, pad_stride=pad * es)
                        yield (0, fmt, 0, bd, cw, ch, w, h), pics, L, oref.picture(pics, w, h, fmt, bd)
                    for fmt in oref.RGB_FORMATS.get(bd, ()):
                        fl = oref.FLAGS[(n + pad_i) % 4]
                        n += 1
                        L = jm.out_layout(fmt | fl, w, h, pad_stride=4 * pad)
                        yield (0, fmt | fl, 0, bd, cw, ch, w, h), pics, L, oref.picture(pics, w, h, fmt | fl, bd)
                    for dtype, dbd in tr.PAIRS:
                        if dbd != bd:
                            continue
                        for kind in KINDS:
                            fl = oref.FLAGS[(n + pad_i) % 4]
                            n += 1
                            L = tensor_layout(jm, dtype, w, h, kind, fl, pad * tr.ES[dtype])
                            yield (1, dtype, fl, bd, cw, ch, w, h), pics, L, oref.tensor(pics, w, h, dtype, fl, bd)


def test_reference_walk_equals_output_ref(checker, tmp_path):
    """jmout_picture / jmout_tensor, under ASan into exact-size blocks, == output_ref; every byte that
    is not a destination element keeps the canary"""
    jm = load_jmhip()
    cases, want = [], []
    with open(tmp_path / "cases.bin", "wb") as f:
        for head, pics, L, ref in walk_cases(jm):
            tensor = hasattr(L, "stride_x")
            offs = list(L.offsets) + [-1] * (3 - len(L.offsets))
            strides = [L.stride_x, L.stride_y, 0] if tensor else list(L.strides) + [0] * (3 - len(L.strides))
            f.write(np.array(list(head) + offs + strides + [L.nbytes] + [0] * 9, "<i8").tobytes())
            for p in pics:
                f.write(p.tobytes())
            cases.append((head, L))
            want.append(expected_block(L, ref))
    r = subprocess.run([checker, "walk", str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, env=ENV)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in log and "Sanitizer" not in log, log[-4000:]
    # 7 crops x 3 strides x (8 bits: 2 YUV + 2 RGB + 4 dtypes x 4 layouts; 9 bits: 1; 10 bits: 2 + 2 + 16)
    assert f"output walk: {len(cases)} cases" in log and len(cases) == 7 * 3 * (20 + 1 + 20)
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    assert got.size == sum(b.size for b in want)
    at = 0
    for (head, L), b in zip(cases, want):
        g = got[at:at + b.size]
        at += b.size
        assert np.array_equal(g, b), f"case {head}: bytes {np.flatnonzero(g != b)[:8].tolist()} of {b.size} differ"


def test_argument_rules_and_hand_worked_values(checker):
    r = subprocess.run([checker, "rules"], capture_output=True, text=True, timeout=120, env=ENV)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in log and "Sanitizer" not in log, log[-4000:]
    m = re.search(r"output rules: (\d+) checks, (\d+) differ", log)
    assert m and int(m.group(1)) >= 100 and int(m.group(2)) == 0, log[-2000:]


def test_reference_values_worked_by_hand():
    """output_ref on values worked out by hand"""
    y = np.full((2, 2), 235, np.uint8)
    c = np.full((1, 1), 128, np.uint8)
    assert [a.tolist() for a in oref.to_rgb(y, c, c, 0, 8)] == [[[255, 255], [255, 255]]] * 3           # white, limited range
    assert [a.tolist() for a in oref.to_rgb(y - 219, c, c, 0, 8)] == [[[0, 0], [0, 0]]] * 3             # black
    # V at its top over mid grey, BT.601 limited: R = (19077 * 110 + 26149 * 127 + 8192) >> 14 = 331 -> 255, G = 25, B = 128
    counts = {}
    r, g, b = oref.to_rgb(np.full((2, 2), 126, np.uint8), c, c + 127, 0, 8, counts)
    assert (r == 255).all() and (g == 25).all() and (b == 128).all() and counts == {"lo": [0, 0, 0], "hi": [4, 0, 0]}
    # full range, grey: R = G = B = Y
    y10 = np.arange(4, dtype=np.uint16).reshape(2, 2) * 300
    c10 = np.full((1, 1), 512, np.uint16)
    assert all(np.array_equal(a, y10) for a in oref.to_rgb(y10, c10, c10, oref.FULL_RANGE | oref.BT709, 10))
    # 1/3: float32 0x3eaaaaab, float16 0x3555, bfloat16 0x3eab
    assert oref.dequantise(np.array([85]), oref.F32, 8).view(np.uint32)[0] == 0x3eaaaaab
    assert oref.dequantise(np.array([341]), oref.F16, 10).view(np.uint16)[0] == 0x3555 and oref.dequantise(np.array([85]), oref.BF16, 8)[0] == 0x3eab
    # the packers
    pics = (np.full((16, 16), 126, np.uint8), np.full((8, 8), 128, np.uint8), np.full((8, 8), 255, np.uint8))
    assert oref.picture(pics, 2, 2, oref.BGRA8, 8)[0].tolist() == [[0xffff1980] * 2] * 2 and oref.picture(pics, 2, 2, oref.RGBA8, 8)[0][0, 0] == 0xff8019ff
    p10 = tuple(a.astype(np.uint16) for a in pics)
    assert oref.picture(p10, 4, 2, oref.P010, 10)[0][0, 0] == 126 << 6 and oref.picture(p10, 4, 2, oref.P010, 10)[1].tolist() == [[128 << 6, 255 << 6] * 2]
    assert oref.picture(pics, 4, 2, oref.NV12, 8)[1].tolist() == [[128, 255, 128, 255]] and oref.picture(p10, 4, 2, oref.I010, 10)[2].tolist() == [[255, 255]]
    word = int(oref.picture(p10, 2, 2, oref.RGB10A2 | oref.FULL_RANGE, 10)[0][0, 0])
    assert word >> 30 == 3 and word & 1023 == 0 and word >> 20 & 1023 == 0                             # U, V far below mid grey at 10 bits
    # uniformly random YUV clamps every component on both sides from 16 x 2 pixels up
    rng = np.random.default_rng(1)
    for bd in (8, 10):
        for w, h in ((34, 18), (32, 32), (30, 2)):
            counts = {}
            oref.to_rgb(*oref.crop(oref.random_yuv(rng, 48, 32, bd), w, h), oref.BT709, bd, counts)
            assert oref.clamps_everywhere(counts), (bd, w, h, counts)


# ---- the additive ABI ----
def test_abi_is_additive(tmp_path):
    """every declaration of include/jmhip_output.h is exported; jmhip.h includes it last; the ABI
    version stays 14; the two descriptors have the layouts of their input twins"""
    ensure_built()
    jm = load_jmhip()
    lib = ctypes.CDLL(LIBJMHIP)
    inc = os.path.dirname(HEADER)
    declared = lambda name: set(re.findall(r"\b(jmh_[a-z0-9_]+)\s*\(", open(os.path.join(inc, name)).read()))
    assert declared("jmhip_output.h") == set(jm.EXPORTED_OUTPUT) == {"jmh_pull_picture", "jmh_pull_tensor", "jmh_convert_picture", "jmh_convert_tensor",
                                                                     "jmh_device_output_wait", "jmh_device_download", "jmh_yuv_coefficients",
                                                                     "jmh_tensor_dequantise"}
    out = subprocess.run(["nm", "-D", "--defined-only", LIBJMHIP], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r" T (jmh_[a-z0-9_]+)$", out, re.M))
    for name in jm.EXPORTED_OUTPUT:
        assert name in defined and hasattr(lib, name), name
    text = open(HEADER).read()
    includes = re.findall(r'#include "(jmhip_[a-z_]+\.h)"', text)
    assert includes[-1] == "jmhip_output.h" and includes.count("jmhip_output.h") == 1
    assert len(declared("jmhip.h")) == 37 and len(jm.EXPORTED) == 37
    for other in (jm.EXPORTED, jm.EXPORTED_INPUT, jm.EXPORTED_RGB, jm.EXPORTED_TENSOR, jm.EXPORTED_NAL, jm.EXPORTED_CODED):
        assert set(other).isdisjoint(jm.EXPORTED_OUTPUT)
    assert lib.jmh_abi_version() == 14 == jm.JMH_ABI_VERSION
    assert ctypes.sizeof(jm.JmhDeviceTensorOut) == 64 and ctypes.sizeof(jm.JmhDevicePictureOut) == 72
    src = tmp_path / "hdr.c"
    src.write_text('#include <stddef.h>\n#include "jmhip.h"\n'
                   "typedef char sizes[sizeof(jmh_device_tensor_out) == sizeof(jmh_device_tensor) && sizeof(jmh_device_picture_out) == sizeof(jmh_device_picture) ? 1 : -1];\n"
                   "typedef char offsets[offsetof(jmh_device_tensor_out, chan) == 16 && offsetof(jmh_device_tensor_out, stride_x) == 40 && "
                   "offsetof(jmh_device_tensor_out, stream) == 56 && offsetof(jmh_device_picture_out, plane) == 16 && "
                   "offsetof(jmh_device_picture_out, stride) == 40 && offsetof(jmh_device_picture_out, stream) == 64 ? 1 : -1];\n"
                   "typedef char values[JMH_OUT_DEBLOCKED == 0 && JMH_OUT_RECON == 1 && JMH_ABI_VERSION == 14 ? 1 : -1];\n"
                   "int use(jmh_ctx *c, const jmh_device_tensor_out *t, const jmh_device_picture_out *p, int32_t *q) {\n"
                   "    return jmh_pull_tensor(c, JMH_OUT_RECON, t) + jmh_pull_picture(c, JMH_OUT_DEBLOCKED, p) + jmh_yuv_coefficients(0, 8, q); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "hdr.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_out_layouts():
    """layouts, strides, offsets and masks of jmhip.out_layout and jmhip.out_tensor_layout"""
    jm = load_jmhip()
    L = jm.out_layout(jm.JMH_PIX_I420, 6, 4)
    assert (L.offsets, L.strides, L.nbytes) == ([0, 256, 512], [6, 3, 3], 512 + 3 + 3) and int(L.mask().sum()) == 24 + 6 + 6
    L = jm.out_layout(jm.JMH_PIX_P010, 6, 4, pad_stride=4, misalign=2, guard=64)
    assert (L.offsets, L.strides) == ([258, 512 + 2], [16, 16]) and L.nbytes == 514 + 16 + 12 + 64 and not L.mask()[:258].any()
    L = jm.out_layout(jm.JMH_PIX_BGRA8 | jm.JMH_PIX_BT709, 6, 4, pad_stride=8)
    assert (L.format, L.offsets, L.strides, L.nbytes) == (16 | 256, [0], [32], 3 * 32 + 24)
    s = L.at(0x1000, stream=5).struct()
    assert isinstance(s, jm.JmhDevicePictureOut) and (s.format, s.width, s.height, s.plane[0], s.stride[0], s.stream) == (272, 6, 4, 0x1000, 32, 5)
    T = jm.out_tensor_layout(jm.JMH_T_F16, 6, 4)
    assert (T.offsets, T.stride_x, T.stride_y, T.nbytes) == ([0, 256, 512], 2, 12, 512 + 48)
    T = jm.out_tensor_layout(jm.JMH_T_F32, 6, 4, "hwc", "bgr", 4, pad_stride=8, misalign=4, guard=64)
    assert (T.offsets, T.stride_x, T.stride_y) == ([256 + 4 + 8, 256 + 4 + 4, 256 + 4], 16, 104)
    assert T.nbytes == 260 + 3 * 104 + (5 * 4 + 3) * 4 + 64 and int(T.mask().sum()) == 6 * 4 * 3 * 4
    assert not T.mask()[260 + 12:260 + 16].any()                              # the fourth channel is not the library's
    t = T.at(0x2000, stream=9).struct()
    assert isinstance(t, jm.JmhDeviceTensorOut) and (t.dtype, t.chan[2], t.stride_x, t.stream) == (4, 0x2000 + 260, 16, 9)
    for bad in (dict(layout="nchw"), dict(order="rgx"), dict(channels=5), dict(layout="chw", channels=4), dict(misalign=2), dict(pad_stride=6)):
        with pytest.raises(ValueError):
            jm.out_tensor_layout(jm.JMH_T_F32, 6, 4, **bad)


# ---- 5: the lencod keys ----
def run(binary, *kv):
    ensure_built()
    args = []
    for e in kv:
        args += ["-p", e]
    return subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)


def test_device_recon_key_rejections():
    """the product binary rejects the keys in PatchInp, before any device is touched; the CPU build has
    no device output"""
    r = run(LENCOD, "DeviceReconFormat=16")                                                   # ReconFile is not set
    assert r.returncode != 0 and "DeviceReconFormat=16" in r.stderr and "needs ReconFile" in r.stderr
    r = run(LENCOD, "DeviceReconTensor=2")
    assert r.returncode != 0 and "DeviceReconTensor=2" in r.stderr and "needs ReconFile" in r.stderr
    rec = "ReconFile=rec.out"
    r = run(LENCOD, rec, "DeviceReconFormat=16", "DeviceReconTensor=1")                       # two layouts for one file
    assert r.returncode != 0 and "DeviceReconFormat=16" in r.stderr and "DeviceReconTensor=1" in r.stderr and "set one of them" in r.stderr
    r = run(LENCOD, rec, "DeviceReconFormat=20")
    assert r.returncode != 0 and "out of range" in r.stderr
    r = run(LENCOD, rec, "DeviceReconTensor=5")
    assert r.returncode != 0 and "out of range" in r.stderr
    r = run(LENCOD, rec, "DeviceReconFormat=3")
    assert r.returncode != 0 and "DeviceReconFormat=3 not supported" in r.stderr
    # the bit depth does not match
    ten = ["ProfileIDC=110", "SourceBitDepthLuma=10", "SourceBitDepthChroma=10"]
    for fmt in (16, 17):
        r = run(LENCOD, rec, f"DeviceReconFormat={fmt}", *ten)
        assert r.returncode != 0 and f"DeviceReconFormat={fmt}" in r.stderr and "SourceBitDepthLuma=8" in r.stderr
    for fmt in (18, 19):
        r = run(LENCOD, rec, f"DeviceReconFormat={fmt}")
        assert r.returncode != 0 and f"DeviceReconFormat={fmt}" in r.stderr and "SourceBitDepthLuma=10" in r.stderr
    for kind in (1, 2):
        r = run(LENCOD, rec, f"DeviceReconTensor={kind}", *ten)
        assert r.returncode != 0 and f"DeviceReconTensor={kind}" in r.stderr and "SourceBitDepthLuma=8" in r.stderr
    r = run(LENCOD, rec, "DeviceReconTensor=3")
    assert r.returncode != 0 and "DeviceReconTensor=3" in r.stderr and "SourceBitDepthLuma=10" in r.stderr
    r = run(LENCOD, rec, "DeviceReconTensor=4", "ProfileIDC=110", "SourceBitDepthLuma=9", "SourceBitDepthChroma=9")
    assert r.returncode != 0 and "DeviceReconTensor=4" in r.stderr and "8 or 10" in r.stderr
    # the matrix and range keys need one of the two
    r = run(LENCOD, rec, "DeviceReconMatrix=1")
    assert r.returncode != 0 and "DeviceReconMatrix" in r.stderr and "DeviceReconFormat=16..19" in r.stderr
    r = run(LENCOD, rec, "DeviceReconFullRange=1")
    assert r.returncode != 0 and "DeviceReconFullRange" in r.stderr and "DeviceReconTensor=1..4" in r.stderr
    # taken with one of them: the next rejection is another key's
    r = run(LENCOD, rec, "DeviceReconTensor=1", "DeviceReconMatrix=1", "DeviceReconFullRange=1", "SearchRange=99")
    assert r.returncode != 0 and "SearchRange" in r.stderr and "DeviceRecon" not in r.stderr
    # 0 asks for nothing
    r = run(LENCOD, "DeviceReconFormat=0", "DeviceReconTensor=0", "SearchRange=99")
    assert r.returncode != 0 and "SearchRange" in r.stderr and "DeviceRecon" not in r.stderr
    # a build without the device backend
    for key in ("DeviceReconFormat=16", "DeviceReconTensor=4"):
        r = run(LENCOD_CPU, rec, key)
        assert r.returncode != 0 and key in r.stderr and "needs the device backend" in r.stderr and "no device output" in r.stderr
