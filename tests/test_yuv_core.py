"""The 4:2:2 / 4:4:4 device-picture core (csrc/jmh_yuv.h, the text k_ingest_yuv of csrc/jmh_yuv.hip
compiles) against the formulas of include/jmhip_yuv.h and host/yuv.c's padding, on the CPU.

tests/harness/yuv_check.c is a stand-alone C program built from the header and host/yuv.c with
-fsanitize=address,undefined -fno-sanitize-recover.  For each of the 11 formats, and for both
sitings of the four 4:4:4 ones, it builds the source planes in malloc blocks of exactly their bytes,
so an offset outside a plane is an ASan error, reduces them through the core and compares with a
plain restatement (planar samples, clamp, the three formulas written out, jm_pad_picture): coded
32x32 from 32x32, 18x18, 30x2, 2x30 and 2x2 (chroma 1x1), coded 48x32 from 34x18; strides tight, +1
(the formats of single bytes), +4, +28.  The I210 / I410 sources (bit depths 10 and 9) hold 0, maxv,
maxv + 1 and 65535 and the clamp count is the number of source samples above maxv.  jmy_check is
compared with the argument rules of include/jmhip_yuv.h.

Also here (no GPU needed): jmhip.yuv_reduce (what the GPU tests compare the kernel with) against
hand-computed 4x4 cases, the replication identity, to_device_yuv's layouts, the DeviceInputYUV
key's rejections, the additive ABI."""
import ctypes
import fcntl
import os
import re
import subprocess

import numpy as np
import pytest

from jmpaths import HARNESS, HEADER, LENCOD, LENCOD_CPU, LIBJMHIP, ensure_built, load_jmhip

ASAN = os.path.join(HARNESS, "_build_asan")
CHECK = os.path.join(ASAN, "yuv_check")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")


@pytest.fixture(scope="module")
def checker():
    with open(os.path.join(HARNESS, ".sanitize.lock"), "w") as lk:       # one sanitizer build at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", HARNESS, "-f", "yuv.mk"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("yuv_check build failed:\n" + r.stdout + r.stderr)
    return CHECK


def test_core_equals_unpack_reduce_and_pad(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=300, env=ENV)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in log and "Sanitizer" not in log, log[-4000:]
    m = re.search(r"yuv check: (\d+) pictures, (\d+) clamped samples, (\d+) differ", log)
    assert m, log[-2000:]
    pictures, clamped, bad = (int(v) for v in m.groups())
    # 6 size pairs; 15 variants (11 formats, the four 4:4:4 ones at both sitings): the 6 of single bytes (I422, NV16,
    # YUYV, UYVY, I444 x 2) at 4 strides, the other 9 at 3; the 3 that clamp (I210, I410 x 2) once more at 9 bits
    assert pictures == 6 * (6 * 4 + 9 * 3 + 3 * 3) and bad == 0
    assert clamped >= 6 * 3 * 3 * 2 * 2          # every I210 / I410 picture holds maxv + 1 and 65535 in each plane (2x2: chroma may share them)


# ---- jmhip.yuv_reduce: the numpy reference of the GPU tests -------------------------------------
C4 = np.array([[10, 20, 30, 41],
               [12, 23, 35, 47],
               [100, 0, 255, 254],
               [1, 2, 3, 9]], np.uint8)
Y4 = np.arange(16, dtype=np.uint8).reshape(4, 4) * 15


def test_yuv_reduce_hand_computed():
    jm = load_jmhip()
    # 4:2:2: chroma is 4 rows x 2 columns; rows are merged in pairs, (a + b + 1) >> 1
    c422 = C4[:, :2]
    y, u, v = jm.yuv_reduce(Y4, c422, c422[:, ::-1], jm.JMH_PIX_UYVY, 8)
    assert np.array_equal(y, Y4) and y.dtype == np.uint8
    assert u.tolist() == [[11, 22], [51, 1]]                     # (10+12+1)>>1, (20+23+1)>>1 / (100+1+1)>>1, (0+2+1)>>1
    assert v.tolist() == [[22, 11], [1, 51]]
    # the flag has no effect on 4:2:2
    assert all(np.array_equal(a, b) for a, b in zip(jm.yuv_reduce(Y4, c422, c422, jm.JMH_PIX_I422 | jm.JMH_PIX_CHROMA_LEFT, 8),
                                                    jm.yuv_reduce(Y4, c422, c422, jm.JMH_PIX_I422, 8)))
    # 4:4:4 centred: the rounded mean of each 2x2 block
    y, u, v = jm.yuv_reduce(Y4, C4, C4.T, jm.JMH_PIX_I444, 8)
    assert u.tolist() == [[(10 + 20 + 12 + 23 + 2) >> 2, (30 + 41 + 35 + 47 + 2) >> 2], [(100 + 0 + 1 + 2 + 2) >> 2, (255 + 254 + 3 + 9 + 2) >> 2]]
    assert u.tolist() == [[16, 38], [26, 130]]
    assert v.tolist() == [[(10 + 12 + 20 + 23 + 2) >> 2, (100 + 1 + 0 + 2 + 2) >> 2], [(30 + 35 + 41 + 47 + 2) >> 2, (255 + 3 + 254 + 9 + 2) >> 2]]
    # 4:4:4 left-sited: column 0 takes C[r][0] as its own left neighbour (max(2i - 1, 0) = 0), column 1 takes C[r][1]
    y, u, v = jm.yuv_reduce(Y4, C4, C4, jm.JMH_PIX_VUYA8 | jm.JMH_PIX_CHROMA_LEFT, 8)
    h = lambda r, i: int(C4[r, max(2 * i - 1, 0)]) + 2 * int(C4[r, 2 * i]) + int(C4[r, 2 * i + 1])
    assert [h(0, 0), h(1, 0), h(0, 1), h(1, 1)] == [10 + 20 + 20, 12 + 24 + 23, 20 + 60 + 41, 23 + 70 + 47]
    assert u.tolist() == [[(50 + 59 + 4) >> 3, (121 + 140 + 4) >> 3], [(h(2, 0) + h(3, 0) + 4) >> 3, (h(2, 1) + h(3, 1) + 4) >> 3]]
    assert u.tolist() == [[14, 33], [38, 98]] and np.array_equal(u, v)
    # 16 bits: I410 clamps to maxv before the sum, Y410 has nothing to clamp; the result is uint16
    big = np.array([[1023, 1024], [65535, 0]], np.uint16)
    y, u, v = jm.yuv_reduce(big, big, big, jm.JMH_PIX_I410, 10)
    assert y.dtype == np.uint16 and y.tolist() == [[1023, 1023], [1023, 0]] and u.tolist() == [[(3 * 1023 + 2) >> 2]] == [[767]]
    y, u, v = jm.yuv_reduce(big, big, big, jm.JMH_PIX_I410, 9)
    assert y.tolist() == [[511, 511], [511, 0]] and u.tolist() == [[(3 * 511 + 2) >> 2]]
    y, u, v = jm.yuv_reduce(big, big, big, jm.JMH_PIX_I410 | jm.JMH_PIX_CHROMA_LEFT, 10)
    assert u.tolist() == [[(1023 + 2 * 1023 + 1023 + 1023 + 2 * 1023 + 0 + 4) >> 3]]
    y, u, v = jm.yuv_reduce(big[:, :1].repeat(2, 1), big[:, :1], big[:, 1:], jm.JMH_PIX_I210, 10)
    assert u.tolist() == [[(1023 + 1023 + 1) >> 1]] and v.tolist() == [[(1023 + 0 + 1) >> 1]]


def test_yuv_reduce_gives_a_replicated_420_picture_back():
    """a 4:2:2 or centred 4:4:4 source whose chroma is the replication of a 4:2:0 picture's chroma"""
    jm = load_jmhip()
    rng = np.random.default_rng(9)
    for bd, fmts in ((8, (jm.JMH_PIX_I422, jm.JMH_PIX_NV16, jm.JMH_PIX_YUYV, jm.JMH_PIX_UYVY, jm.JMH_PIX_I444, jm.JMH_PIX_VUYA8)),
                     (10, (jm.JMH_PIX_I210, jm.JMH_PIX_P210, jm.JMH_PIX_Y210, jm.JMH_PIX_I410, jm.JMH_PIX_Y410))):
        y = rng.integers(0, 1 << bd, (34, 50))
        u, v = rng.integers(0, 1 << bd, (17, 25)), rng.integers(0, 1 << bd, (17, 25))
        for fmt in fmts:
            rep = (lambda c: c.repeat(2, 0).repeat(2, 1)) if fmt in jm.YUV_444 else (lambda c: c.repeat(2, 0))
            got = jm.yuv_reduce(y, rep(u), rep(v), fmt, bd)
            assert all(np.array_equal(a, b) for a, b in zip(got, (y, u, v))), fmt
    # left-sited is another filter: it does not
    got = jm.yuv_reduce(y, u.repeat(2, 0).repeat(2, 1), v.repeat(2, 0).repeat(2, 1), jm.JMH_PIX_I410 | jm.JMH_PIX_CHROMA_LEFT, 10)
    assert not np.array_equal(got[1], u)


def test_to_device_yuv_layouts():
    """the packed layouts byte by byte, strides, offsets, nothing behind the last row"""
    jm = load_jmhip()
    rng = np.random.default_rng(5)
    y = rng.integers(0, 256, (4, 6), dtype=np.uint8)
    u2, v2 = rng.integers(0, 256, (4, 3), dtype=np.uint8), rng.integers(0, 256, (4, 3), dtype=np.uint8)
    u4, v4 = rng.integers(0, 256, (4, 6), dtype=np.uint8), rng.integers(0, 256, (4, 6), dtype=np.uint8)
    L = jm.to_device_yuv((y, u2, v2), jm.JMH_PIX_YUYV, pad_stride=4, misalign=3)
    assert L.strides == [16] and L.offsets == [3] and L.buf.nbytes == 3 + 3 * 16 + 12 and (L.format, L.width, L.height) == (34, 6, 4)
    row = L.buf[3 + 16:3 + 16 + 12].tolist()
    assert row == [y[1, 0], u2[1, 0], y[1, 1], v2[1, 0], y[1, 2], u2[1, 1], y[1, 3], v2[1, 1], y[1, 4], u2[1, 2], y[1, 5], v2[1, 2]]
    L = jm.to_device_yuv((y, u2, v2), jm.JMH_PIX_UYVY)
    assert L.buf[:4].tolist() == [u2[0, 0], y[0, 0], v2[0, 0], y[0, 1]]
    L = jm.to_device_yuv((y, u2, v2), jm.JMH_PIX_NV16, pad_stride=1)
    assert L.strides == [7, 7] and L.offsets == [0, 256] and L.buf[256:262].tolist() == [u2[0, 0], v2[0, 0], u2[0, 1], v2[0, 1], u2[0, 2], v2[0, 2]]
    L = jm.to_device_yuv((y, u2, v2), jm.JMH_PIX_I422)
    assert L.strides == [6, 3, 3] and L.buf.nbytes == 512 + 12
    L = jm.to_device_yuv((y, u4, v4), jm.JMH_PIX_VUYA8 | jm.JMH_PIX_CHROMA_LEFT)
    assert L.format == 37 | 1024 and L.strides == [24] and L.buf[4:7].tolist() == [v4[0, 1], u4[0, 1], y[0, 1]]
    L = jm.to_device_yuv((y, u4, v4), jm.JMH_PIX_I444, misalign=1)
    assert L.strides == [6, 6, 6] and L.offsets == [1, 257, 513]
    y16, u16, v16 = (a.astype(np.uint16) * 4 + 1 for a in (y, u4, v4))
    L = jm.to_device_yuv((y16, u16, v16), jm.JMH_PIX_Y410)
    d = L.buf[:L.strides[0]].view("<u4")
    assert L.strides == [24] and (int(d[2]) & 1023, int(d[2]) >> 10 & 1023, int(d[2]) >> 20 & 1023) == (u16[0, 2], y16[0, 2], v16[0, 2])
    assert any(int(x) >> 30 for x in d)
    L = jm.to_device_yuv((y16, u16[:, :3], v16[:, :3]), jm.JMH_PIX_Y210)
    wds = L.buf[:L.strides[0]].view("<u2")
    assert L.strides == [24] and [int(x) >> 6 for x in wds[:4]] == [y16[0, 0], u16[0, 0], y16[0, 1], v16[0, 0]] and any(int(x) & 63 for x in wds)
    L = jm.to_device_yuv((y16, u16[:, :3], v16[:, :3]), jm.JMH_PIX_P210)
    assert L.strides == [12, 12] and int(L.buf[256:258].view("<u2")[0]) >> 6 == u16[0, 0] and int(L.buf[258:260].view("<u2")[0]) >> 6 == v16[0, 0]
    L = jm.to_device_yuv((y16, u16[:, :3], v16[:, :3]), jm.JMH_PIX_I210)
    assert L.strides == [12, 6, 6] and int(L.buf[256:258].view("<u2")[0]) == u16[0, 0]
    L = jm.to_device_yuv((y16, u16, v16), jm.JMH_PIX_I410)
    assert L.strides == [12, 12, 12]
    with pytest.raises(ValueError):
        jm.to_device_yuv((y, u4, v4), jm.JMH_PIX_I422)               # 4:4:4 planes for a 4:2:2 format
    with pytest.raises(ValueError):
        jm.to_device_yuv((y, u2, v2), jm.JMH_PIX_I420)


# ---- lencod -------------------------------------------------------------------------------------
def run(binary, *kv):
    ensure_built()
    args = []
    for e in kv:
        args += ["-p", e]
    return subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)


def test_device_input_yuv_key_rejections(tmp_path):
    """the product binary rejects the key in PatchInp, before any device is touched"""
    full = ["DeviceInput=1", "DeviceCAVLC=1", "DeviceWriterAsync=1", f"InputFile={tmp_path}/in.uyvy"]
    r = run(LENCOD, "DeviceInputYUV=35", "DeviceCAVLC=1", "DeviceWriterAsync=1")                   # DeviceInput is not set
    assert r.returncode != 0 and "DeviceInputYUV=35" in r.stderr and "needs DeviceInput=1" in r.stderr
    r = run(LENCOD, "DeviceInputYUV=35", "DeviceInput=1", f"InputFile={tmp_path}/in.uyvy")          # no async writer
    assert r.returncode != 0 and "DeviceInputYUV=35" in r.stderr and "needs DeviceWriterAsync=1" in r.stderr
    for code, depth in ((35, 10), (36, 9), (40, 8), (43, 8), (41, 9), (42, 8), (44, 9)):           # a wrong bit depth
        r = run(LENCOD, *full, f"DeviceInputYUV={code}", f"SourceBitDepthLuma={depth}", f"SourceBitDepthChroma={depth}", "ProfileIDC=110")
        assert r.returncode != 0 and f"DeviceInputYUV={code}" in r.stderr and "needs SourceBitDepthLuma=" in r.stderr, (code, depth)
    r = run(LENCOD, *full, "DeviceInputYUV=35", "DeviceInputFormat=16")
    assert r.returncode != 0 and "DeviceInputYUV=35 and DeviceInputFormat=16 both name the layout" in r.stderr
    r = run(LENCOD, *full, "DeviceInputYUV=35", "DeviceInputTensor=1")
    assert r.returncode != 0 and "DeviceInputYUV=35 and DeviceInputTensor=1 both name the layout" in r.stderr
    for code in (39, 38, 1, 31):
        r = run(LENCOD, *full, f"DeviceInputYUV={code}")
        assert r.returncode != 0 and f"DeviceInputYUV={code} not supported" in r.stderr, code
    r = run(LENCOD, *full, "DeviceInputYUV=45")
    assert r.returncode != 0 and "DeviceInputYUV" in r.stderr
    r = run(LENCOD, "DeviceInput=1", "DeviceCAVLC=1", "DeviceWriterAsync=1", "InputFile=synthetic:5", "DeviceInputYUV=35")
    assert r.returncode != 0 and "DeviceInputYUV=35" in r.stderr and "synthetic source" in r.stderr
    # DeviceInputChromaLeft without a scale: taken with a 4:4:4 layout only
    r = run(LENCOD, *full, "DeviceInputYUV=35", "DeviceInputChromaLeft=1")
    assert r.returncode != 0 and "need DeviceInputScale=1..3" in r.stderr
    # taken (4:2:2, 4:4:4 left-sited, 10 bits, with a scale): the next rejection is another key's
    for more in (["DeviceInputYUV=35"], ["DeviceInputYUV=36", "DeviceInputChromaLeft=1"],
                 ["DeviceInputYUV=44", "SourceBitDepthLuma=10", "SourceBitDepthChroma=10", "ProfileIDC=110"],
                 ["DeviceInputYUV=40", "SourceBitDepthLuma=9", "SourceBitDepthChroma=9", "ProfileIDC=110"],
                 ["DeviceInputYUV=34", "DeviceInputScale=2", "DeviceInputWidth=352", "DeviceInputHeight=288"]):
        r = run(LENCOD, *full, *more, "SearchRange=99")
        assert r.returncode != 0 and "SearchRange" in r.stderr and "DeviceInputYUV" not in r.stderr, more
    # 0 asks for nothing
    r = run(LENCOD, "DeviceInputYUV=0", "SearchRange=99")
    assert r.returncode != 0 and "SearchRange" in r.stderr and "DeviceInputYUV" not in r.stderr
    # a build without the device backend
    r = run(LENCOD_CPU, "DeviceInputYUV=35", "DeviceInput=1")
    assert r.returncode != 0 and "needs the device backend" in r.stderr


# ---- the additive ABI ---------------------------------------------------------------------------
def test_abi_is_additive(tmp_path):
    """include/jmhip_yuv.h declares values and no function; jmhip.h includes it once, directly behind
    jmhip_rgb.h; the ABI version stays 14, jmh_device_picture keeps its 72 bytes and the library
    exports what it exported"""
    ensure_built()
    jm = load_jmhip()
    lib = ctypes.CDLL(LIBJMHIP)
    inc = os.path.dirname(HEADER)
    declared = lambda name: set(re.findall(r"\b(jmh_[a-z0-9_]+)\s*\(", open(os.path.join(inc, name)).read()))
    assert declared("jmhip_yuv.h") == set()
    includes = re.findall(r'#include "(jmhip_[a-z_]+\.h)"', open(HEADER).read())
    assert includes.count("jmhip_yuv.h") == 1 and includes[includes.index("jmhip_rgb.h") + 1] == "jmhip_yuv.h"
    assert len(declared("jmhip.h")) == 37 and len(jm.EXPORTED) == 37
    assert declared("jmhip_input.h") == set(jm.EXPORTED_INPUT) and len(jm.EXPORTED_INPUT) == 10
    assert declared("jmhip_rgb.h") == set(jm.EXPORTED_RGB) == {"jmh_rgb_coefficients"}
    out = subprocess.run(["nm", "-D", "--defined-only", LIBJMHIP], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r" T (jmh_[a-z0-9_]+)$", out, re.M))
    known = set()
    for name in dir(jm):
        if name.startswith("EXPORTED"):
            known |= set(getattr(jm, name))
    assert defined == known, sorted(defined ^ known)                   # no new entry point
    assert lib.jmh_abi_version() == 14 == jm.JMH_ABI_VERSION
    assert ctypes.sizeof(jm.JmhDevicePicture) == 72
    assert (jm.JMH_PIX_I422, jm.JMH_PIX_NV16, jm.JMH_PIX_YUYV, jm.JMH_PIX_UYVY, jm.JMH_PIX_I444, jm.JMH_PIX_VUYA8) == (32, 33, 34, 35, 36, 37)
    assert (jm.JMH_PIX_I210, jm.JMH_PIX_P210, jm.JMH_PIX_Y210, jm.JMH_PIX_I410, jm.JMH_PIX_Y410, jm.JMH_PIX_CHROMA_LEFT) == (40, 41, 42, 43, 44, 1024)
    # jmhip_yuv.h compiles as C by itself and after jmhip.h, with the mirrored values
    src = tmp_path / "hdr.c"
    src.write_text('#include "jmhip.h"\n#include "jmhip_yuv.h"\n'
                   "typedef char picture_is_72[sizeof(jmh_device_picture) == 72 ? 1 : -1];\n"
                   "typedef char values[JMH_PIX_I422 == 32 && JMH_PIX_NV16 == 33 && JMH_PIX_YUYV == 34 && JMH_PIX_UYVY == 35 && JMH_PIX_I444 == 36 && "
                   "JMH_PIX_VUYA8 == 37 && JMH_PIX_I210 == 40 && JMH_PIX_P210 == 41 && JMH_PIX_Y210 == 42 && JMH_PIX_I410 == 43 && JMH_PIX_Y410 == 44 && "
                   "JMH_PIX_CHROMA_LEFT == 1024 && JMH_PIX_P010 == 3 && JMH_PIX_BGR10A2 == 19 && JMH_PIX_FULL_RANGE == 512 && JMH_ABI_VERSION == 14 ? 1 : -1];\n"
                   "int use(jmh_ctx *c, jmh_device_picture *p, const jmh_frame_params *fp) { p->format = JMH_PIX_I444 | JMH_PIX_CHROMA_LEFT; "
                   "return jmh_frame_push_device(c, p, fp); }\n")
    alone = tmp_path / "alone.c"
    alone.write_text('#include "jmhip_yuv.h"\ntypedef char v[JMH_PIX_Y410 == 44 ? 1 : -1];\n')
    for f in (src, alone):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, "-c", str(f), "-o", str(tmp_path / "hdr.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
