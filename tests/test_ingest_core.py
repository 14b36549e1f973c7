"""The device-picture core (csrc/jmh_ingest.h, the text k_ingest of csrc/jmh_ingest.hip compiles)
against host/yuv.c's padding, on the CPU.

tests/harness/ingest_check.c is a stand-alone C program built from the header and host/yuv.c with
-fsanitize=address,undefined -fno-sanitize-recover.  For I420, NV12, I010 (bit depths 9 and 10)
and P010 it builds the source planes in malloc blocks of exactly their bytes, so an offset outside
a plane is an ASan error, ingests them through the core and compares with a plain restatement
(unpack to planar, clamp as read_hbd does, jm_pad_picture): coded 32x32 from 32x32, 18x18, 30x2,
2x30 and 2x2 (chroma 1x1), coded 48x32 from 34x18; strides tight, +1 (8-bit), +2, +26.  The I010
sources hold 0, maxv, maxv + 1 and 65535 and the clamp count is the number of source samples above
maxv.  The packed-word helpers (jmi_deint, jmi_value_x2) are compared with their per-sample meaning
and jmi_check with the argument rules of include/jmhip_input.h.

Also here (no GPU needed): the DeviceInput key's rejections, the additive ABI."""
import ctypes
import fcntl
import os
import re
import subprocess

import pytest

from jmpaths import HARNESS, HEADER, LENCOD, LENCOD_CPU, LIBJMHIP, ensure_built, load_jmhip

ASAN = os.path.join(HARNESS, "_build_asan")
CHECK = os.path.join(ASAN, "ingest_check")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")


@pytest.fixture(scope="module")
def checker():
    with open(os.path.join(HARNESS, ".sanitize.lock"), "w") as lk:       # one sanitizer build at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", HARNESS, "-f", "ingest.mk"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("ingest_check build failed:\n" + r.stdout + r.stderr)
    return CHECK


def test_core_equals_unpack_and_pad(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=300, env=ENV)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in log and "Sanitizer" not in log, log[-4000:]
    m = re.search(r"ingest check: (\d+) pictures, (\d+) clamped samples, (\d+) differ", log)
    assert m, log[-2000:]
    pictures, clamped, bad = (int(v) for v in m.groups())
    # 6 size pairs; I420 and NV12 at 4 strides, P010 at 3, I010 at 3 strides and 2 bit depths
    assert pictures == 6 * (4 + 4 + 3 + 6) and bad == 0
    assert clamped >= 6 * 6 * 2 * 3          # every I010 picture holds maxv + 1 and 65535 in each plane


def test_numpy_reference_is_the_core():
    """jmhip.to_device + pad_to_coded (what the GPU tests compare the kernel with) describe the same
    layout and padding as the core: spot-checked through the offsets jmi_src would give."""
    import numpy as np
    jm = load_jmhip()
    rng = np.random.default_rng(5)
    y = rng.integers(0, 256, (18, 34), dtype=np.uint8)
    u = rng.integers(0, 256, (9, 17), dtype=np.uint8)
    v = rng.integers(0, 256, (9, 17), dtype=np.uint8)
    L = jm.to_device((y, u, v), jm.JMH_PIX_NV12, pad_stride=26, misalign=3)
    assert L.strides == [34 + 26, 34 + 26] and [o % 256 for o in L.offsets] == [3, 3] and len(L.offsets) == 2
    assert L.buf.nbytes == L.offsets[1] + 8 * L.strides[1] + 34        # nothing behind the last row
    for (px, py) in ((0, 0), (16, 8), (5, 3)):
        assert L.buf[L.offsets[1] + py * L.strides[1] + 2 * px] == u[py, px]
        assert L.buf[L.offsets[1] + py * L.strides[1] + 2 * px + 1] == v[py, px]
    L = jm.to_device((y.astype(np.uint16) * 4, u, v), jm.JMH_PIX_P010)
    w0 = int(L.buf[L.offsets[0] + 2 * 7]) | int(L.buf[L.offsets[0] + 2 * 7 + 1]) << 8
    assert w0 >> 6 == int(y[0, 7]) * 4 and any(int(b) & 63 for b in L.buf[L.offsets[0]:L.offsets[0] + 68:2])
    py_, pu, pv = jm.pad_to_coded((y, u, v), 48, 32)
    assert py_.shape == (32, 48) and pu.shape == (16, 24)
    assert (py_[:18, :34] == y).all() and (py_[:18, 34:] == y[:, 33:34]).all() and (py_[18:] == py_[17]).all()
    assert (pv[:9, 17:] == v[:, 16:17]).all() and (pv[9:] == pv[8]).all()


def run(binary, *args):
    ensure_built()
    return subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)


def test_device_input_key_rejections():
    r = run(LENCOD_CPU, "-p", "DeviceInput=1")                                    # the CPU build has no device input
    assert r.returncode != 0 and "DeviceInput=1" in r.stderr and "device backend" in r.stderr
    r = run(LENCOD_CPU, "-p", "DeviceInput=2")
    assert r.returncode != 0 and "DeviceInput" in r.stderr
    r = run(LENCOD_CPU, "-p", "DeviceInput=0", "-p", "DeviceCAVLC=1")             # 0 asks for nothing: the writer's own rejection
    assert r.returncode != 0 and "DeviceInput" not in r.stderr
    # the product binary has a device input, and rejects the key without the pipelined path before any device is touched
    r = run(LENCOD, "-p", "DeviceInput=1", "-p", "PipelineDepth=1")
    assert r.returncode != 0 and "DeviceInput=1" in r.stderr and "pipelined path" in r.stderr


def test_abi_is_additive(tmp_path):
    """The entry points are exported and declared in include/jmhip_input.h (which jmhip.h includes
    last); the ABI version stays 14 and jmhip.h's own declarations are the 37 of ABI 14."""
    ensure_built()
    jm = load_jmhip()
    lib = ctypes.CDLL(LIBJMHIP)
    inc = os.path.dirname(HEADER)
    declared = lambda name: set(re.findall(r"\b(jmh_[a-z0-9_]+)\s*\(", open(os.path.join(inc, name)).read()))
    assert declared("jmhip_input.h") == set(jm.EXPORTED_INPUT) and len(jm.EXPORTED_INPUT) == 10
    out = subprocess.run(["nm", "-D", "--defined-only", LIBJMHIP], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r" T (jmh_[a-z0-9_]+)$", out, re.M))
    for name in jm.EXPORTED_INPUT:
        assert name in defined and hasattr(lib, name), name
    text = open(HEADER).read()
    assert text.index('#include "jmhip_cabac_split.h"') < text.index('#include "jmhip_input.h"')
    assert len(declared("jmhip.h")) == 37 and set(jm.EXPORTED).isdisjoint(jm.EXPORTED_INPUT)
    assert lib.jmh_abi_version() == 14 == jm.JMH_ABI_VERSION
    assert ctypes.sizeof(jm.JmhDevicePicture) == 72
    # jmhip_input.h compiles as C by itself after jmhip.h, and the struct has the mirrored size
    src = tmp_path / "hdr.c"
    src.write_text('#include "jmhip.h"\n#include "jmhip_input.h"\n'
                   "_Static_assert(sizeof(jmh_device_picture) == 72, \"layout\");\n"
                   "_Static_assert(JMH_PIX_P010 == 3 && JMH_ABI_VERSION == 14, \"values\");\n"
                   "int use(jmh_ctx *c, const jmh_device_picture *p, const jmh_frame_params *fp) { return jmh_frame_push_device(c, p, fp); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "hdr.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # without a context every call is rejected through its status code
    ld = jm.load()
    pic = jm.JmhDevicePicture()
    assert ld.jmh_frame_push_device(None, ctypes.byref(pic), None) == jm.JMH_E_INVALID_ARG
    assert ld.jmh_frame_push_coded_device(None, ctypes.byref(pic), None, 0, None, 0, 0) == jm.JMH_E_INVALID_ARG
    assert ld.jmh_ingest_picture(None, ctypes.byref(pic), None, None, None, 0, 0) == jm.JMH_E_INVALID_ARG
    assert ld.jmh_device_input_wait(None) == jm.JMH_E_INVALID_ARG
    assert ld.jmh_device_input_clamped(None, None) == jm.JMH_E_INVALID_ARG
    p = ctypes.c_void_p()
    assert ld.jmh_device_malloc(None, 16, ctypes.byref(p)) == jm.JMH_E_INVALID_ARG
    assert ld.jmh_device_free(None, None) == jm.JMH_E_INVALID_ARG
    assert ld.jmh_device_upload(None, None, None, 0, None) == jm.JMH_E_INVALID_ARG
    assert ld.jmh_device_stream_create(None, ctypes.byref(p)) == jm.JMH_E_INVALID_ARG
    assert ld.jmh_device_stream_destroy(None, None) == jm.JMH_E_INVALID_ARG
