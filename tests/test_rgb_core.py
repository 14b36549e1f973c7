"""The RGB device-picture core (csrc/jmh_rgb.h, the text k_ingest_rgb of csrc/jmh_rgb.hip compiles)
against its formulas and host/yuv.c's padding, on the CPU.

tests/harness/rgb_check.c is a stand-alone C program built from the header and host/yuv.c with
-fsanitize=address,undefined -fno-sanitize-recover and run directly.  For BGRA8, RGBA8, RGB10A2 and
BGR10A2, each with both matrices and both ranges, it builds the source plane in a malloc block of
exactly its bytes, so an offset outside it is an ASan error, converts it through the core and
compares with a plain restatement (unpack, the formulas at the source size, jm_pad_picture): coded
32x32 from 32x32, 18x18, 30x2, 2x30 and 2x2, coded 48x32 from 34x18; strides tight, +4, +52.  It also
holds every coefficient row against its float64 derivation, every sample before its clamp within
0.5 + 3 M 2^-15 of the real-valued formula, the full-range chroma clamp as exercised in every
full-range picture, and jmr_check against the argument rules of include/jmhip_rgb.h.

Also here (no GPU needed): tests/rgb_ref.py (the reference of the GPU tests) against the table, the
core and jmh_rgb_coefficients; the additive ABI; the rejections of the lencod keys."""
import ctypes
import fcntl
import os
import re
import subprocess

import numpy as np
import pytest

import rgb_ref
from jmpaths import HARNESS, HEADER, LENCOD, LIBJMHIP, ensure_built, load_jmhip

ASAN = os.path.join(HARNESS, "_build_asan")
CHECK = os.path.join(ASAN, "rgb_check")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
FLAGS = (0, rgb_ref.BT709, rgb_ref.FULL_RANGE, rgb_ref.BT709 | rgb_ref.FULL_RANGE)


@pytest.fixture(scope="module")
def checker():
    with open(os.path.join(HARNESS, ".sanitize.lock"), "w") as lk:       # one sanitizer build at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", HARNESS, "-f", "rgb.mk"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("rgb_check build failed:\n" + r.stdout + r.stderr)
    return CHECK


def test_core_equals_formulas_and_pad(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=300, env=ENV)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in log and "Sanitizer" not in log, log[-4000:]
    m = re.search(r"rgb check: (\d+) pictures, (\d+) clamped samples, worst ([0-9.]+) of the bound, (\d+) differ", log)
    assert m, log[-2000:]
    pictures, clamped, bad = int(m.group(1)), int(m.group(2)), int(m.group(4))
    # 4 layouts x 2 matrices x 2 ranges, 6 size pairs, 3 strides
    assert pictures == 4 * 4 * 6 * 3 and bad == 0
    assert clamped >= pictures // 2          # every full-range picture clamps at least one chroma sample
    assert float(m.group(3)) <= 1.0


def test_reference_coefficients_are_the_table_and_the_library():
    """rgb_ref derives the coefficients from (Kr, Kb) in float64: they equal the table of DESIGN.md §5.8
    (kept as literals in rgb_ref.TABLE) and what jmh_rgb_coefficients returns, for every format"""
    ensure_built()
    jm = load_jmhip()
    n = 0
    for layout in rgb_ref.LAYOUTS:
        bd = rgb_ref.depth_of(layout)
        for fl in FLAGS:
            c = rgb_ref.coefficients(layout | fl, bd)
            assert c[:9] == rgb_ref.TABLE[(int(bool(fl & rgb_ref.BT709)), bd, int(bool(fl & rgb_ref.FULL_RANGE)))]
            assert c[9:] == [0 if fl & rgb_ref.FULL_RANGE else 16 << (bd - 8), 1 << (bd - 1), (1 << bd) - 1]
            assert c == jm.rgb_coefficients(layout | fl, bd)
            # black, white, grey
            assert c[0] + c[1] + c[2] == int(np.rint((c[11] if fl & rgb_ref.FULL_RANGE else 219 << (bd - 8)) / c[11] * 16384))
            assert c[3] + c[4] + c[5] == 0 == c[6] + c[7] + c[8]
            n += 1
    assert n == 16
    assert (jm.JMH_PIX_BGRA8, jm.JMH_PIX_RGBA8, jm.JMH_PIX_RGB10A2, jm.JMH_PIX_BGR10A2) == rgb_ref.LAYOUTS
    assert (jm.JMH_PIX_BT709, jm.JMH_PIX_FULL_RANGE) == (rgb_ref.BT709, rgb_ref.FULL_RANGE)
    # the status codes of the call
    lib = jm.load()
    out = (ctypes.c_int32 * 12)()
    for fmt, bd, want in ((16, 10, jm.JMH_E_UNSUPPORTED_CFG), (18, 8, jm.JMH_E_UNSUPPORTED_CFG), (17, 9, jm.JMH_E_UNSUPPORTED_CFG),
                          (19, 9, jm.JMH_E_UNSUPPORTED_CFG), (0, 8, jm.JMH_E_INVALID_ARG), (1 | 256, 8, jm.JMH_E_INVALID_ARG),
                          (4, 8, jm.JMH_E_INVALID_ARG), (15, 8, jm.JMH_E_INVALID_ARG), (20, 8, jm.JMH_E_INVALID_ARG),
                          (16 | 1 << 10, 8, jm.JMH_E_INVALID_ARG), (-1, 8, jm.JMH_E_INVALID_ARG)):
        assert lib.jmh_rgb_coefficients(fmt, bd, out) == want, (fmt, bd)
    assert lib.jmh_rgb_coefficients(16, 8, None) == jm.JMH_E_INVALID_ARG


def test_reference_layout_and_values():
    """rgb_ref and jmhip.to_device_rgb on values worked out by hand: the byte order of every layout,
    the one-plane layout with nothing behind the last row, the padding, the live chroma clamp"""
    jm = load_jmhip()
    r, g, b = rgb_ref.unpack(np.array([[0xAA332211]], np.uint32), rgb_ref.BGRA8)
    assert (int(r[0, 0]), int(g[0, 0]), int(b[0, 0])) == (0x33, 0x22, 0x11)
    r, g, b = rgb_ref.unpack(np.array([[0xAA332211]], np.uint32), rgb_ref.RGBA8)
    assert (int(r[0, 0]), int(g[0, 0]), int(b[0, 0])) == (0x11, 0x22, 0x33)
    word = np.array([[3 << 30 | 0x3A1 << 20 | 0x155 << 10 | 0x2C3]], np.uint32)
    assert [int(a[0, 0]) for a in rgb_ref.unpack(word, rgb_ref.RGB10A2)] == [0x2C3, 0x155, 0x3A1]
    assert [int(a[0, 0]) for a in rgb_ref.unpack(word, rgb_ref.BGR10A2)] == [0x3A1, 0x155, 0x2C3]
    # pure blue, full range, BT.601: Y = (1868 * 255 + 8192) >> 14 = 29, U = 128 + 128 clamped, V = 128 + ((-1332 * 1020 + 32768) >> 16) = 107
    blue = np.full((2, 2), 0xFFFF0000, np.uint32)
    y, u, v = rgb_ref.convert(blue, rgb_ref.RGBA8 | rgb_ref.FULL_RANGE, 8)
    assert y.dtype == np.uint8 and (y == 29).all() and int(u[0, 0]) == 255 and int(v[0, 0]) == 107
    # white and black, limited range, 10 bits
    y, u, v = rgb_ref.convert(np.array([[0x3FFFFFFF, 0x3FFFFFFF], [0, 0]], np.uint32), rgb_ref.RGB10A2 | rgb_ref.BT709, 10)
    assert y.dtype == np.uint16 and y.tolist() == [[940, 940], [64, 64]] and int(u[0, 0]) == 512 == int(v[0, 0])
    py, pu, pv = rgb_ref.to_yuv(rgb_ref.random_words(np.random.default_rng(1), 34, 18, rgb_ref.BGRA8), rgb_ref.BGRA8, 8, 48, 32)
    assert py.shape == (32, 48) and pu.shape == pv.shape == (16, 24)
    assert (py[:18, 34:] == py[:18, 33:34]).all() and (py[18:] == py[17]).all() and (pv[:9, 17:] == pv[:9, 16:17]).all() and (pu[9:] == pu[8]).all()
    # the layout
    words = rgb_ref.random_words(np.random.default_rng(2), 6, 4, rgb_ref.BGRA8)
    L = jm.to_device_rgb(words, jm.JMH_PIX_BGRA8 | jm.JMH_PIX_BT709, pad_stride=52, misalign=12)
    assert (L.format, L.width, L.height, L.offsets, L.strides) == (16 | 256, 6, 4, [12], [24 + 52])
    assert L.buf.nbytes == 12 + 3 * 76 + 24                                   # nothing behind the last row
    assert bytes(L.buf[12 + 2 * 76 + 4 * 5:12 + 2 * 76 + 4 * 6]) == int(words[2, 5]).to_bytes(4, "little")
    L2 = jm.to_device_rgb(words.view(np.uint8).reshape(4, 6, 4), jm.JMH_PIX_BGRA8)
    assert L2.strides == [24] and L2.offsets == [0] and bytes(L2.buf) == words.astype("<u4").tobytes()
    for bad in (dict(misalign=2), dict(pad_stride=6)):
        with pytest.raises(ValueError):
            jm.to_device_rgb(words, jm.JMH_PIX_BGRA8, **bad)
    pic = L.at(0x10000)
    s = pic.struct()
    assert (s.plane[0], s.plane[1], s.plane[2], s.stride[0]) == (0x10000 + 12, None, None, 76)


def test_abi_is_additive(tmp_path):
    """jmh_rgb_coefficients is exported and declared in include/jmhip_rgb.h (which jmhip.h includes
    after jmhip_nal.h); the ABI version stays 14, jmh_device_picture keeps its 72 bytes, jmhip.h's
    own declarations are the 37 of ABI 14 and jmhip_input.h keeps its ten"""
    ensure_built()
    jm = load_jmhip()
    lib = ctypes.CDLL(LIBJMHIP)
    inc = os.path.dirname(HEADER)
    declared = lambda name: set(re.findall(r"\b(jmh_[a-z0-9_]+)\s*\(", open(os.path.join(inc, name)).read()))
    assert declared("jmhip_rgb.h") == set(jm.EXPORTED_RGB) == {"jmh_rgb_coefficients"}
    out = subprocess.run(["nm", "-D", "--defined-only", LIBJMHIP], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r" T (jmh_[a-z0-9_]+)$", out, re.M))
    for name in jm.EXPORTED_RGB:
        assert name in defined and hasattr(lib, name), name
    # every declaration of every header is exported
    headers = ("jmhip.h", "jmhip_cavlc.h", "jmhip_cabac.h", "jmhip_coded.h", "jmhip_cabac_split.h", "jmhip_input.h", "jmhip_nal.h", "jmhip_rgb.h")
    assert defined >= set().union(*(declared(h) for h in headers))
    text = open(HEADER).read()
    assert text.index('#include "jmhip_nal.h"') < text.index('#include "jmhip_rgb.h"')
    assert len(declared("jmhip.h")) == 37 and set(jm.EXPORTED).isdisjoint(jm.EXPORTED_RGB)
    assert declared("jmhip_input.h") == set(jm.EXPORTED_INPUT) and len(jm.EXPORTED_INPUT) == 10
    assert lib.jmh_abi_version() == 14 == jm.JMH_ABI_VERSION
    assert ctypes.sizeof(jm.JmhDevicePicture) == 72
    src = tmp_path / "hdr.c"
    src.write_text('#include "jmhip.h"\n#include "jmhip_rgb.h"\n'
                   "_Static_assert(sizeof(jmh_device_picture) == 72, \"layout\");\n"
                   "_Static_assert(JMH_PIX_BGRA8 == 16 && JMH_PIX_RGBA8 == 17 && JMH_PIX_RGB10A2 == 18 && JMH_PIX_BGR10A2 == 19, \"values\");\n"
                   "_Static_assert(JMH_PIX_BT709 == 256 && JMH_PIX_FULL_RANGE == 512 && JMH_PIX_P010 == 3 && JMH_ABI_VERSION == 14, \"values\");\n"
                   "int use(int32_t *out) { return jmh_rgb_coefficients(JMH_PIX_BGRA8 | JMH_PIX_BT709, 8, out); }\n")
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


def test_device_input_format_key_rejections():
    """the product binary rejects the keys in PatchInp, before any device is touched"""
    r = run(LENCOD, *params("DeviceInputFormat=16"))                                          # without DeviceInput=1
    assert r.returncode != 0 and "DeviceInputFormat=16" in r.stderr and "needs DeviceInput=1" in r.stderr
    r = run(LENCOD, *params("DeviceInputMatrix=1"))
    assert r.returncode != 0 and "DeviceInputMatrix" in r.stderr and "DeviceInput=1" in r.stderr
    r = run(LENCOD, *params("DeviceInputFullRange=1", "DeviceInput=1"))                       # the flags describe an RGB source
    assert r.returncode != 0 and "DeviceInputFullRange" in r.stderr and "DeviceInputFormat=16..19" in r.stderr
    base = ["DeviceInput=1", "DeviceCAVLC=1", "DeviceWriterAsync=1", "InputFile=missing.rgb"]
    for fmt in (4, 15):                                                                       # 4..15 stay invalid
        r = run(LENCOD, *params(*base, f"DeviceInputFormat={fmt}"))
        assert r.returncode != 0 and f"DeviceInputFormat={fmt} not supported" in r.stderr
    r = run(LENCOD, *params(*base, "DeviceInputFormat=20"))
    assert r.returncode != 0 and "out of range" in r.stderr
    # a format and a bit depth that do not match
    r = run(LENCOD, *params(*base, "DeviceInputFormat=18"))
    assert r.returncode != 0 and "SourceBitDepthLuma=10" in r.stderr and "DeviceInputFormat=18" in r.stderr
    r = run(LENCOD, *params(*base, "DeviceInputFormat=17", "ProfileIDC=110", "SourceBitDepthLuma=10", "SourceBitDepthChroma=10"))
    assert r.returncode != 0 and "SourceBitDepthLuma=8" in r.stderr and "DeviceInputFormat=17" in r.stderr
    # a synthetic source
    r = run(LENCOD, *params("DeviceInput=1", "DeviceCAVLC=1", "DeviceWriterAsync=1", "DeviceInputFormat=16", "InputFile=synthetic:3"))
    assert r.returncode != 0 and "synthetic" in r.stderr and "DeviceInputFormat=16" in r.stderr
    # without DeviceWriterAsync=1
    r = run(LENCOD, *params("DeviceInput=1", "DeviceCAVLC=1", "DeviceInputFormat=16", "InputFile=missing.rgb"))
    assert r.returncode != 0 and "DeviceWriterAsync=1" in r.stderr and "DeviceInputFormat=16" in r.stderr
    # format 0 asks for nothing: the keys at their defaults pass PatchInp (the run then fails on the missing file or device)
    r = run(LENCOD, *params("DeviceInputFormat=0", "DeviceInputMatrix=0", "DeviceInputFullRange=0", "SearchRange=99"))
    assert r.returncode != 0 and "SearchRange" in r.stderr and "DeviceInput" not in r.stderr
