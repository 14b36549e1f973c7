"""Device pushes scaled to a chosen size (include/jmhip_scale.h), the parts that need
no GPU: the tap tables of jmh_scale_taps against their float64 restatement and the properties the
header states, the reference walk of csrc/jmh_scale.h against tests/scale_ref.py, the additive ABI, the
lencod keys.

tests/harness/scale_check.c is a stand-alone C program built from the header with
-fsanitize=address,undefined -fno-sanitize-recover and run directly: it walks every case of the GPU
test, at both bit depths, from a malloc block of exactly the source's bytes into one of exactly the
destination's, so one stray byte is a report, and runs the argument rules."""
import ctypes
import fcntl
import os
import re
import subprocess

import numpy as np
import pytest

import scale_ref as sr
from jmpaths import HARNESS, HEADER, LENCOD, LENCOD_CPU, LIBJMHIP, ensure_built, load_jmhip

ASAN = os.path.join(HARNESS, "_build_asan")
CHECK = os.path.join(ASAN, "scale_check")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
# n_src : n_dst of the table tests: 1:1, 2:1, 4:1, 1:2, 1:32, 125:31, 65:24
RATIOS = [(64, 64), (128, 64), (256, 64), (32, 64), (2, 64), (125, 31), (65, 24)]
FILTERS = (sr.BILINEAR, sr.BICUBIC, sr.LANCZOS3)


@pytest.fixture(scope="module")
def checker():
    with open(os.path.join(HARNESS, ".sanitize.lock"), "w") as lk:       # one sanitizer build at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", HARNESS, "-f", "scale.mk"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("scale_check build failed:\n" + r.stdout + r.stderr)
    return CHECK


# ---- 1: the tables ----
@pytest.mark.parametrize("filter", FILTERS, ids=[sr.NAMES[f] for f in FILTERS])
@pytest.mark.parametrize("left", (False, True), ids=("centred", "left"))
@pytest.mark.parametrize("n_src,n_dst", RATIOS, ids=[f"{a}to{b}" for a, b in RATIOS])
def test_tables(n_src, n_dst, filter, left):
    """jmh_scale_taps: T, first, the sums, sum(|q|) <= 32767, every tap against float64 numpy.  A tap is
    floor(x + 0.5) of a weight that two float64 evaluations give within far less than 1 of each other:
    the integers differ by at most 1.  The one tap that takes 16384 - sum(q) moves by at most T / 2 more
    (T roundings, each off by at most 1/2)."""
    jm = load_jmhip()
    S = sr.SUPPORT[filter]
    T = 2 * int(np.ceil(S * max(1.0, n_src / n_dst)))
    assert T == sr.ntaps(n_src, n_dst, filter)
    if T > sr.TAPS_MAX:                                        # 125:31 with Lanczos3: 26 taps
        with pytest.raises(jm.JmhError) as e:
            jm.scale_taps(n_src, n_dst, filter, left)
        assert e.value.status == jm.JMH_E_UNSUPPORTED_CFG
        nt = ctypes.c_int(0)
        assert jm.load().jmh_scale_taps(n_src, n_dst, filter, int(left), None, None, ctypes.byref(nt)) == jm.JMH_E_UNSUPPORTED_CFG and nt.value == T
        return
    first, taps = jm.scale_taps(n_src, n_dst, filter, left)
    assert first.dtype == np.int32 and taps.dtype == np.int16 and taps.shape == (n_dst, T)
    q = taps.astype(np.int64)
    assert (q.sum(axis=1) == sr.ONE).all()
    assert int(np.abs(q).sum(axis=1).max()) <= 32767
    want_first, want_q, real = sr.tables(n_src, n_dst, filter, left)
    assert np.array_equal(first, want_first)
    phi = 0.25 if left else 0.5
    c = (np.arange(n_dst) + phi) * (n_src / n_dst) - phi
    assert np.array_equal(first, np.floor(c - T / 2).astype(np.int64) + 1)
    off = np.abs(q - np.floor(real + 0.5).astype(np.int64))
    loose = off > 1
    assert (loose.sum(axis=1) <= 1).all() and int(off.max()) <= T // 2 + 1
    if n_src == n_dst:                                         # 1:1: the single tap 16384
        assert (np.sort(q, axis=1)[:, :-1] == 0).all() and (q.max(axis=1) == sr.ONE).all()
        assert np.array_equal(first + q.argmax(axis=1), np.arange(n_dst))


def test_tables_statuses():
    jm = load_jmhip()
    lib, nt = jm.load(), ctypes.c_int(0)
    assert lib.jmh_scale_taps(9, 2, sr.LANCZOS3, 0, None, None, ctypes.byref(nt)) == jm.JMH_E_UNSUPPORTED_CFG and nt.value == 28
    assert lib.jmh_scale_taps(9, 2, sr.BICUBIC, 0, None, None, ctypes.byref(nt)) == jm.JMH_OK and nt.value == 18
    for bad in ((0, 8, 1), (8, 0, 1), (8, 8, 0), (8, 8, 4), (sr.SRC_MAX + 1, 8, 1)):
        assert lib.jmh_scale_taps(*bad, 0, None, None, ctypes.byref(nt)) == jm.JMH_E_INVALID_ARG, bad
    assert lib.jmh_scale_taps(8, 8, 1, 0, None, None, None) == jm.JMH_E_INVALID_ARG


# ---- 2: the reference walk under the sanitizers ----
def lib_taps(jm):
    return lambda n_src, n_dst, filter, left: jm.scale_taps(n_src, n_dst, filter, left)


def test_scale_check_rules(checker):
    r = subprocess.run([checker, "rules"], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("case", sr.CASES, ids=[sr.case_id(c) for c in sr.CASES])
def test_walk_equals_the_restatement(checker, tmp_path, case, bd):
    """jms_scale over exact-size buffers == scale_ref on the library's tables, byte for byte, padding included"""
    jm = load_jmhip()
    W, H, w, h, ow, oh, filter, left = case
    rng = np.random.default_rng(w * 131 + h * 7 + ow + bd)
    pics = sr.random_yuv(rng, w, h, bd)
    (inp := tmp_path / "in.yuv").write_bytes(b"".join(a.tobytes() for a in pics))
    out = tmp_path / "out.yuv"
    r = subprocess.run([checker, "run", str(inp), str(out), *map(str, (w, h, ow, oh, W, H, filter, int(left), bd))],
                       capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want, peak = sr.scale_picture(pics, ow, oh, W, H, filter, left, bd, lib_taps(jm))
    assert peak <= 32767
    assert out.read_bytes() == b"".join(a.tobytes() for a in want)
    if (w, h) == (ow, oh):                                     # the identity: the source, padded
        assert all(np.array_equal(a, sr.pad(b, a.shape[1], a.shape[0])) for a, b in zip(want, pics))


@pytest.mark.parametrize("case", sr.REFUSED, ids=[sr.case_id(c) for c in sr.REFUSED])
def test_walk_refuses_more_than_24_taps(checker, tmp_path, case):
    W, H, w, h, ow, oh, filter, left = case
    (inp := tmp_path / "in.yuv").write_bytes(bytes(w * h * 3 // 2))
    r = subprocess.run([checker, "run", str(inp), str(tmp_path / "out.yuv"), *map(str, (w, h, ow, oh, W, H, filter, int(left), 8))],
                       capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 3 and "refused" in r.stderr


# ---- 3: the additive ABI ----
def test_abi_is_additive(tmp_path):
    """every declaration of include/jmhip_scale.h is exported; jmhip.h includes it once, directly before
    jmhip_output.h; the ABI version stays 14; the header compiles as C after jmhip.h"""
    ensure_built()
    jm = load_jmhip()
    lib = ctypes.CDLL(LIBJMHIP)
    inc = os.path.dirname(HEADER)
    declared = lambda name: set(re.findall(r"\b(jmh_[a-z0-9_]+)\s*\(", open(os.path.join(inc, name)).read()))
    assert declared("jmhip_scale.h") == set(jm.EXPORTED_SCALE) == {"jmh_input_scale", "jmh_scale_taps", "jmh_scale_info"}
    out = subprocess.run(["nm", "-D", "--defined-only", LIBJMHIP], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r" T (jmh_[a-z0-9_]+)$", out, re.M))
    for name in jm.EXPORTED_SCALE:
        assert name in defined and hasattr(lib, name), name
    includes = re.findall(r'#include "(jmhip_[a-z_]+\.h)"', open(HEADER).read())
    assert includes.count("jmhip_scale.h") == 1 and includes[-2:] == ["jmhip_scale.h", "jmhip_output.h"]
    assert len(declared("jmhip.h")) == 37 and len(jm.EXPORTED) == 37
    for other in (jm.EXPORTED, jm.EXPORTED_INPUT, jm.EXPORTED_RGB, jm.EXPORTED_TENSOR, jm.EXPORTED_NAL, jm.EXPORTED_CODED, jm.EXPORTED_OUTPUT):
        assert set(other).isdisjoint(jm.EXPORTED_SCALE)
    assert lib.jmh_abi_version() == 14 == jm.JMH_ABI_VERSION
    assert ctypes.sizeof(jm.JmhScale) == 16 and ctypes.sizeof(jm.JmhDevicePicture) == 72
    assert (jm.JMH_SCALE_OFF, jm.JMH_SCALE_BILINEAR, jm.JMH_SCALE_BICUBIC, jm.JMH_SCALE_LANCZOS3, jm.JMH_SCALE_CHROMA_LEFT) == (0, 1, 2, 3, 1)
    src = tmp_path / "hdr.c"
    src.write_text('#include "jmhip.h"\n#include "jmhip_scale.h"\n'
                   "typedef char sizes[sizeof(jmh_scale) == 16 ? 1 : -1];\n"
                   "typedef char values[JMH_SCALE_OFF == 0 && JMH_SCALE_LANCZOS3 == 3 && JMH_SCALE_CHROMA_LEFT == 1 && JMH_SCALE_TAPS_MAX == 24 && "
                   "JMH_SCALE_SRC_MAX == 8192 && JMH_ABI_VERSION == 14 ? 1 : -1];\n"
                   "int use(jmh_ctx *c, jmh_scale *s, int32_t *f, int16_t *t, int *n) {\n"
                   "    return jmh_input_scale(c, s) + jmh_scale_info(c, s, n) + jmh_scale_taps(4, 2, JMH_SCALE_BICUBIC, 0, f, t, n); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "hdr.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- 4: the lencod keys ----
def run(binary, *kv):
    ensure_built()
    args = []
    for e in kv:
        args += ["-p", e]
    return subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)


def test_device_input_scale_key_rejections(tmp_path):
    """the product binary rejects the keys in PatchInp, before any device is touched"""
    size = ["DeviceInputWidth=352", "DeviceInputHeight=288"]
    full = ["DeviceInput=1", "DeviceCAVLC=1", "DeviceWriterAsync=1", f"InputFile={tmp_path}/in.yuv"]
    r = run(LENCOD, "DeviceInputScale=3", *size)                                               # DeviceInput is not set
    assert r.returncode != 0 and "DeviceInputScale=3" in r.stderr and "needs DeviceInput=1" in r.stderr
    r = run(LENCOD, "DeviceInputScale=2", *size, "DeviceInput=1", f"InputFile={tmp_path}/in.yuv")
    assert r.returncode != 0 and "DeviceInputScale=2" in r.stderr and "needs DeviceWriterAsync=1" in r.stderr
    r = run(LENCOD, "DeviceInputScale=1", *size, "DeviceInput=1", "DeviceCAVLC=1", "DeviceWriterAsync=1", "InputFile=synthetic:5")
    assert r.returncode != 0 and "DeviceInputScale=1" in r.stderr and "synthetic source" in r.stderr
    for key in ("DeviceInputWidth=352", "DeviceInputHeight=288", "DeviceInputChromaLeft=1"):   # the keys without the filter
        r = run(LENCOD, *full, key)
        assert r.returncode != 0 and "need DeviceInputScale=1..3" in r.stderr, key
    r = run(LENCOD, *full, "DeviceInputScale=4", *size)
    assert r.returncode != 0 and "out of range" in r.stderr
    for bad in (["DeviceInputWidth=0", "DeviceInputHeight=288"], ["DeviceInputWidth=352"], ["DeviceInputWidth=8194", "DeviceInputHeight=288"],
                ["DeviceInputWidth=352", "DeviceInputHeight=8194"]):
        r = run(LENCOD, *full, "DeviceInputScale=3", *bad)
        assert r.returncode != 0 and "DeviceInputScale=3" in r.stderr and "out of range" in r.stderr and "2..8192" in r.stderr, bad
    for bad in (["DeviceInputWidth=351", "DeviceInputHeight=288"], ["DeviceInputWidth=352", "DeviceInputHeight=287"],
                [*size, "SourceWidth=175"], [*size, "SourceHeight=143"]):
        r = run(LENCOD, *full, "DeviceInputScale=3", *bad)
        assert r.returncode != 0 and "DeviceInputScale=3" in r.stderr and "must be even" in r.stderr, bad
    # taken with DeviceInput and the async writer: the next rejection is another key's; with RGB and tensors too
    for more in ([], ["DeviceInputFormat=16"], ["DeviceInputTensor=1"]):
        r = run(LENCOD, *full, "DeviceInputScale=3", *size, "DeviceInputChromaLeft=1", *more, "SearchRange=99")
        assert r.returncode != 0 and "SearchRange" in r.stderr and "DeviceInputScale" not in r.stderr, more
    # 0 asks for nothing
    r = run(LENCOD, "DeviceInputScale=0", "DeviceInputWidth=0", "DeviceInputChromaLeft=0", "SearchRange=99")
    assert r.returncode != 0 and "SearchRange" in r.stderr and "DeviceInputScale" not in r.stderr
    # a build without the device backend
    r = run(LENCOD_CPU, "DeviceInputScale=3", *size, "DeviceInput=1")
    assert r.returncode != 0 and "needs the device backend" in r.stderr
