"""The device-tensor core (csrc/jmh_tensor.h, the text k_ingest_tensor of csrc/jmh_tensor.hip compiles)
against integer arithmetic, the RGB formulas and host/yuv.c's padding, on the CPU.

tests/harness/tensor_check.c is a stand-alone C program built from the header and host/yuv.c with
-fsanitize=address,undefined -fno-sanitize-recover and run directly.  Its header comment lists what
it holds: every valid (dtype, bit depth) pair in four layouts with both matrices and both ranges, six
size pairs and three row strides, every channel in a malloc block of exactly its bytes; the quantiser
over all F16 and BF16 patterns and the F32 edge sets; jmt_check against the argument rules.

Also here (no GPU needed): jmh_tensor_quantise and tests/tensor_ref.py (the reference of the GPU
tests) against each other and against integer arithmetic; hand-worked values; the additive ABI; the
rejections of the lencod key; the layouts of jmhip.to_device_tensor."""
import ctypes
import fcntl
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import rgb_ref
import tensor_ref as tr
from jmpaths import HARNESS, HEADER, LENCOD, LIBJMHIP, ensure_built, load_jmhip

ASAN = os.path.join(HARNESS, "_build_asan")
CHECK = os.path.join(ASAN, "tensor_check")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")


@pytest.fixture(scope="module")
def checker():
    with open(os.path.join(HARNESS, ".sanitize.lock"), "w") as lk:       # one sanitizer build at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", HARNESS, "-f", "tensor.mk"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("tensor_check build failed:\n" + r.stdout + r.stderr)
    return CHECK


def test_core_equals_integer_arithmetic_formulas_and_pad(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=300, env=ENV)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in log and "Sanitizer" not in log, log[-4000:]
    m = re.search(r"tensor check: (\d+) pictures, (\d+) quantiser values, (\d+) differ", log)
    assert m, log[-2000:]
    pictures, values, bad = (int(g) for g in m.groups())
    # 8 (dtype, depth) pairs x 4 layouts x 4 flag sets, 6 size pairs, 3 strides
    assert pictures == 8 * 4 * 4 * 6 * 3 and bad == 0
    # both depths: all F16 and BF16 patterns, the F32 random patterns, at least 9 values per k
    assert values >= 2 * (2 * 65536 + (1 << 20)) + 9 * (256 + 1024)


# ---- the quantiser: the library, the numpy reference and integer arithmetic ----
@pytest.mark.parametrize("bd", [8, 10])
def test_quantiser_f16_bf16_every_pattern(bd):
    """all 65,536 bit patterns of F16 and of BF16: jmh_tensor_quantise == tensor_ref.quantise (numpy
    float64) == integer arithmetic on the decoded mantissa and exponent"""
    ensure_built()
    jm = load_jmhip()
    bits = np.arange(65536, dtype=np.uint16)
    for dt, jdt in ((tr.F16, jm.JMH_T_F16), (tr.BF16, jm.JMH_T_BF16)):
        ref = tr.quantise(bits, dt, bd)
        assert np.array_equal(jm.tensor_quantise(bits, jdt, bd), ref), tr.NAMES[dt]
        assert np.array_equal(tr.quantise_exact(tr.bits32(bits, dt), bd), ref), tr.NAMES[dt]
        assert ref.min() == 0 and ref.max() == (1 << bd) - 1
    # a float16 array travels as well as its bits
    assert np.array_equal(jm.tensor_quantise(bits.view(np.float16), jm.JMH_T_F16, bd), tr.quantise(bits, tr.F16, bd))


@pytest.mark.parametrize("bd", [8, 10])
def test_quantiser_f32_edges_and_random(bd):
    """F32: the edge set (every k / M and (k + 1/2) / M with two neighbours a side, +-0, denormals,
    +-inf, NaNs, just outside [0, 1]) three ways; 2^20 random bit patterns library against numpy"""
    ensure_built()
    jm = load_jmhip()
    m = (1 << bd) - 1
    edges = tr.f32_edge_bits(bd)
    assert len(edges) >= 10 * (m + 1)
    ref = tr.quantise(edges, tr.F32, bd)
    assert np.array_equal(jm.tensor_quantise(edges, jm.JMH_T_F32, bd), ref)
    assert np.array_equal(tr.quantise_exact(edges, bd), ref)
    assert set(ref.tolist()) == set(range(m + 1))                      # every level is reached
    # Fraction on a sample of the edge set: a third statement, with no shifts in it
    for b in edges[:: max(1, len(edges) // 500)].tolist():
        x = np.array([b], np.uint32).view(np.float32)[0]
        want = 0 if not x > 0 else m if x >= 1 else int((Fraction(float(x)) * m + Fraction(1, 2)).__floor__())
        assert int(tr.quantise(np.array([b], np.uint32), tr.F32, bd)[0]) == want, hex(b)
    rnd = np.random.default_rng(1000 + bd).integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(jm.tensor_quantise(rnd, jm.JMH_T_F32, bd), tr.quantise(rnd, tr.F32, bd))
    assert np.array_equal(jm.tensor_quantise(rnd.view(np.float32), jm.JMH_T_F32, bd), tr.quantise(rnd, tr.F32, bd))


def test_quantiser_integers_and_status_codes():
    ensure_built()
    jm = load_jmhip()
    u8 = np.arange(256, dtype=np.uint8)
    assert np.array_equal(jm.tensor_quantise(u8, jm.JMH_T_U8, 8), u8.astype(np.int32)) and np.array_equal(tr.quantise(u8, tr.U8, 8), u8)
    u16 = np.arange(65536, dtype=np.uint16)
    assert np.array_equal(jm.tensor_quantise(u16, jm.JMH_T_U16, 10), np.minimum(u16, 1023).astype(np.int32))
    assert np.array_equal(tr.quantise(u16, tr.U16, 10), np.minimum(u16, 1023))
    assert (jm.JMH_T_U8, jm.JMH_T_U16, jm.JMH_T_F16, jm.JMH_T_BF16, jm.JMH_T_F32) == tr.DTYPES
    lib = jm.load()
    q, e = (ctypes.c_int32 * 4)(), (ctypes.c_uint32 * 4)()
    UNSUP, INVAL = jm.JMH_E_UNSUPPORTED_CFG, jm.JMH_E_INVALID_ARG
    for dt, bd, want in ((0, 10, UNSUP), (1, 8, UNSUP), (0, 9, UNSUP), (1, 9, UNSUP), (2, 9, UNSUP), (3, 9, UNSUP), (4, 9, UNSUP), (4, 12, UNSUP),
                         (5, 8, INVAL), (-1, 8, INVAL), (0, 8, jm.JMH_OK), (1, 10, jm.JMH_OK), (2, 8, jm.JMH_OK), (3, 10, jm.JMH_OK),
                         (4, 8, jm.JMH_OK), (4, 10, jm.JMH_OK)):
        assert lib.jmh_tensor_quantise(dt, bd, e, 4, q) == want, (dt, bd)
    assert lib.jmh_tensor_quantise(4, 8, None, 4, q) == INVAL and lib.jmh_tensor_quantise(4, 8, e, 4, None) == INVAL
    assert lib.jmh_tensor_quantise(4, 8, None, 0, None) == jm.JMH_OK
    with pytest.raises(ValueError):
        jm.tensor_quantise(np.zeros(4, np.float32), jm.JMH_T_F16, 8)


def test_reference_values_worked_by_hand():
    """tensor_ref on values worked out by hand, and its tie to rgb_ref"""
    f = lambda *v: np.array(v, np.float32).reshape(1, -1)
    assert tr.quantise(f(0.5), tr.F32, 8).tolist() == [[128]]                    # 127.5 is a tie: up
    assert tr.quantise(f(0.5), tr.F32, 10).tolist() == [[512]]
    assert tr.quantise(np.array([0x3800], np.uint16), tr.F16, 8).tolist() == [128] == tr.quantise(np.array([0x3F00], np.uint16), tr.BF16, 8).tolist()
    assert tr.quantise(f(np.nan, -0.0, -1e-30, -np.inf, 1.0, 1.0000001, np.inf, 0.0019607, 0.0019608), tr.F32, 8).tolist() == [[0, 0, 0, 0, 255, 255, 255, 0, 1]]
    # pure blue, full range, BT.601, 8 bits: Y = (1868 * 255 + 8192) >> 14 = 29, U = 128 + 128 clamped to 255, V = 107
    z, o = np.zeros((2, 2), np.float32), np.ones((2, 2), np.float32)
    y, u, v = tr.convert((z, z, o), tr.F32, tr.FULL_RANGE, 8, 16, 16)
    assert y.dtype == np.uint8 and y.shape == (16, 16) and (y == 29).all() and (u == 255).all() and (v == 107).all()
    # white over black, limited range, BT.709, 10 bits: 940 and 64, chroma 512
    wb = np.array([[1.0, 1.0], [0.0, 0.0]], np.float16)
    y, u, v = tr.convert_source_size((wb, wb, wb), tr.F16, tr.BT709, 10)
    assert y.dtype == np.uint16 and y.tolist() == [[940, 940], [64, 64]] and int(u[0, 0]) == 512 == int(v[0, 0])
    # U16 above M is M; U8 passes through: the same picture as the packed words give
    rng = np.random.default_rng(3)
    ch = tr.random_chans(rng, 6, 4, tr.U8)
    words = ch[0].astype(np.uint32) | ch[1].astype(np.uint32) << 8 | ch[2].astype(np.uint32) << 16 | 0xFF000000
    for a, b in zip(tr.convert(ch, tr.U8, tr.BT709, 8, 16, 16), rgb_ref.to_yuv(words, rgb_ref.RGBA8 | rgb_ref.BT709, 8, 16, 16)):
        assert np.array_equal(a, b)
    # the condition on float content holds down to 2x2, for every float dtype
    for dt in tr.FLOATS:
        for w, h in ((2, 2), (30, 2), (2, 30), (34, 18)):
            assert tr.holds_condition(tr.random_chans(rng, w, h, dt), dt)
    # grey luma: injective at full range, and the reference says so where it is not
    assert tr.grey_luma(np.arange(256), tr.FULL_RANGE, 8).tolist() == list(range(256))
    assert tr.grey_luma(np.arange(1024), tr.FULL_RANGE | tr.BT709, 10).tolist() == list(range(1024))
    with pytest.raises(AssertionError):
        tr.grey_luma(np.arange(256), 0, 8)


def test_abi_is_additive(tmp_path):
    """every declaration of include/jmhip_tensor.h is exported; jmhip.h includes it after jmhip_rgb.h;
    the ABI version stays 14, jmh_device_tensor is 64 bytes, the other headers keep their declarations"""
    ensure_built()
    jm = load_jmhip()
    lib = ctypes.CDLL(LIBJMHIP)
    inc = os.path.dirname(HEADER)
    declared = lambda name: set(re.findall(r"\b(jmh_[a-z0-9_]+)\s*\(", open(os.path.join(inc, name)).read()))
    assert declared("jmhip_tensor.h") == set(jm.EXPORTED_TENSOR) == {"jmh_frame_push_tensor", "jmh_frame_push_coded_tensor", "jmh_ingest_tensor",
                                                                     "jmh_tensor_quantise"}
    out = subprocess.run(["nm", "-D", "--defined-only", LIBJMHIP], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r" T (jmh_[a-z0-9_]+)$", out, re.M))
    for name in jm.EXPORTED_TENSOR:
        assert name in defined and hasattr(lib, name), name
    text = open(HEADER).read()
    assert text.index('#include "jmhip_rgb.h"') < text.index('#include "jmhip_tensor.h"')
    assert len(declared("jmhip.h")) == 37 and len(jm.EXPORTED) == 37
    assert declared("jmhip_input.h") == set(jm.EXPORTED_INPUT) and len(jm.EXPORTED_INPUT) == 10
    assert declared("jmhip_rgb.h") == set(jm.EXPORTED_RGB) == {"jmh_rgb_coefficients"}
    for other in (jm.EXPORTED, jm.EXPORTED_INPUT, jm.EXPORTED_RGB, jm.EXPORTED_NAL, jm.EXPORTED_CODED):
        assert set(other).isdisjoint(jm.EXPORTED_TENSOR)
    assert lib.jmh_abi_version() == 14 == jm.JMH_ABI_VERSION
    assert ctypes.sizeof(jm.JmhDeviceTensor) == 64 and ctypes.sizeof(jm.JmhDevicePicture) == 72
    src = tmp_path / "hdr.c"
    src.write_text('#include <stddef.h>\n#include "jmhip.h"\n#include "jmhip_tensor.h"\n'
                   "typedef char size_is_64[sizeof(jmh_device_tensor) == 64 ? 1 : -1];\n"
                   "typedef char picture_is_72[sizeof(jmh_device_picture) == 72 ? 1 : -1];\n"
                   "typedef char offsets[offsetof(jmh_device_tensor, chan) == 16 && offsetof(jmh_device_tensor, stride_x) == 40 && "
                   "offsetof(jmh_device_tensor, stream) == 56 ? 1 : -1];\n"
                   "typedef char values[JMH_T_U8 == 0 && JMH_T_U16 == 1 && JMH_T_F16 == 2 && JMH_T_BF16 == 3 && JMH_T_F32 == 4 && "
                   "JMH_PIX_BT709 == 256 && JMH_PIX_FULL_RANGE == 512 && JMH_ABI_VERSION == 14 ? 1 : -1];\n"
                   "int use(jmh_ctx *c, const jmh_device_tensor *t, const jmh_frame_params *fp, int32_t *q) {\n"
                   "    return jmh_frame_push_tensor(c, t, fp) + jmh_tensor_quantise(JMH_T_F32, 8, q, 0, q); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "hdr.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def run(binary, *args):
    ensure_built()
    return subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)


def params(*kv):
    out = []
    for e in kv:
        out += ["-p", e]
    return out


def test_device_input_tensor_key_rejections():
    """the product binary rejects the key in PatchInp, before any device is touched"""
    r = run(LENCOD, *params("DeviceInputTensor=1"))                                           # without DeviceInput=1
    assert r.returncode != 0 and "DeviceInputTensor=1" in r.stderr and "needs DeviceInput=1" in r.stderr
    base = ["DeviceInput=1", "DeviceCAVLC=1", "DeviceWriterAsync=1", "InputFile=missing.rgb"]
    r = run(LENCOD, *params(*base, "DeviceInputTensor=5"))
    assert r.returncode != 0 and "out of range" in r.stderr
    r = run(LENCOD, *params(*base, "DeviceInputTensor=2", "DeviceInputFormat=16"))            # two layouts for one file
    assert r.returncode != 0 and "DeviceInputTensor=2" in r.stderr and "DeviceInputFormat=16" in r.stderr
    # a file and a bit depth that do not match
    ten = ["ProfileIDC=110", "SourceBitDepthLuma=10", "SourceBitDepthChroma=10"]
    r = run(LENCOD, *params(*base, "DeviceInputTensor=3"))
    assert r.returncode != 0 and "SourceBitDepthLuma=10" in r.stderr and "DeviceInputTensor=3" in r.stderr
    for kind in (1, 2):
        r = run(LENCOD, *params(*base, f"DeviceInputTensor={kind}", *ten))
        assert r.returncode != 0 and "SourceBitDepthLuma=8" in r.stderr and f"DeviceInputTensor={kind}" in r.stderr
    r = run(LENCOD, *params(*base, "DeviceInputTensor=4", "ProfileIDC=110", "SourceBitDepthLuma=9", "SourceBitDepthChroma=9"))
    assert r.returncode != 0 and "DeviceInputTensor=4" in r.stderr and "8 or 10" in r.stderr
    # a synthetic source
    r = run(LENCOD, *params("DeviceInput=1", "DeviceCAVLC=1", "DeviceWriterAsync=1", "DeviceInputTensor=1", "InputFile=synthetic:3"))
    assert r.returncode != 0 and "synthetic" in r.stderr and "DeviceInputTensor=1" in r.stderr
    # without DeviceWriterAsync=1
    r = run(LENCOD, *params("DeviceInput=1", "DeviceCAVLC=1", "DeviceInputTensor=1", "InputFile=missing.rgb"))
    assert r.returncode != 0 and "DeviceWriterAsync=1" in r.stderr and "DeviceInputTensor=1" in r.stderr
    # the matrix and range keys are taken with a tensor; with neither source key they still name DeviceInputFormat=16..19
    r = run(LENCOD, *params(*base, "DeviceInputTensor=1", "DeviceInputMatrix=1", "DeviceInputFullRange=1", "SearchRange=99"))
    assert r.returncode != 0 and "SearchRange" in r.stderr and "DeviceInput" not in r.stderr
    r = run(LENCOD, *params("DeviceInputFullRange=1", "DeviceInput=1"))
    assert r.returncode != 0 and "DeviceInputFullRange" in r.stderr and "DeviceInputFormat=16..19" in r.stderr
    # 0 asks for nothing
    r = run(LENCOD, *params("DeviceInputTensor=0", "SearchRange=99"))
    assert r.returncode != 0 and "SearchRange" in r.stderr and "DeviceInput" not in r.stderr


def test_to_device_tensor_layouts():
    """layouts, strides and offsets of jmhip.to_device_tensor, with nothing behind the last row"""
    jm = load_jmhip()
    a = np.arange(3 * 4 * 6, dtype=np.uint8).reshape(3, 4, 6)
    L = jm.to_device_tensor(a)
    assert (L.dtype, L.flags, L.width, L.height, L.stride_x, L.stride_y, L.offsets) == (jm.JMH_T_U8, 0, 6, 4, 1, 6, [0, 256, 512])
    assert L.buf.nbytes == 512 + 24 and bytes(L.buf[256:256 + 24]) == a[1].tobytes()
    L = jm.to_device_tensor(a, order="gbr", flags=jm.JMH_PIX_BT709, pad_stride=52, misalign=12)      # the array's planes are G, B, R
    assert (L.flags, L.stride_x, L.stride_y) == (256, 1, 58) and L.offsets == [512 + 12, 12, 256 + 12]
    assert L.buf.nbytes == 512 + 12 + 3 * 58 + 6                                 # nothing behind the last row
    assert bytes(L.buf[12 + 2 * 58:12 + 2 * 58 + 6]) == a[0, 2].tobytes() and L.buf[12 + 6] == 0xA5
    f = np.arange(4 * 6 * 4, dtype=np.float32).reshape(4, 6, 4)
    L = jm.to_device_tensor(f, "hwc", order="bgr", pad_stride=8, misalign=4)
    assert (L.dtype, L.stride_x, L.stride_y, L.offsets) == (jm.JMH_T_F32, 16, 96 + 8, [4 + 8, 4 + 4, 4])
    assert L.buf.nbytes == 4 + 3 * 104 + (5 * 4 + 3) * 4                         # the last pixel's fourth channel is not there
    assert L.buf[4 + 104 + 16 * 2 + 4:][:4].view(np.float32)[0] == f[1, 2, 1]
    h = np.zeros((2, 2, 3), np.float16)
    L = jm.to_device_tensor(h, "hwc")
    assert (L.dtype, L.stride_x, L.stride_y, L.offsets, L.buf.nbytes) == (jm.JMH_T_F16, 6, 12, [0, 2, 4], 24)
    b = jm.to_device_tensor(np.zeros((3, 2, 2), np.uint16), dtype=jm.JMH_T_BF16)
    assert b.dtype == jm.JMH_T_BF16 and jm.to_device_tensor(np.zeros((3, 2, 2), np.uint16)).dtype == jm.JMH_T_U16
    for bad in (dict(misalign=2), dict(pad_stride=6), dict(order="rgx"), dict(layout="nchw")):
        with pytest.raises(ValueError):
            jm.to_device_tensor(f, **{"layout": "hwc", **bad})
    with pytest.raises(ValueError):
        jm.to_device_tensor(np.zeros((3, 2, 2), np.float64))
    t = L.at(0x10000, stream=7)
    s = t.struct()
    assert (s.dtype, s.width, s.height, s.chan[0], s.chan[1], s.chan[2], s.stride_x, s.stride_y, s.stream) == (2, 2, 2, 0x10000, 0x10002, 0x10004, 6, 12, 7)
