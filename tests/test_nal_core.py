"""The device NAL stage's shared core (csrc/jmh_nal.h, the text the kernels of csrc/jmh_nal.hip
compile) against the product's serial packaging, on the CPU.

tests/harness/nal_core_check.c is a stand-alone C99 program built from the header and
host/bitstream.c with -fsanitize=address,undefined -fno-sanitize-recover: it runs the core's passes
serially (plan, count, scan, write) and compares every access unit's bytes, unit offsets and sizes
with jm_write_nal and the cabac_zero_words loop of encode_picture_slices.  Inputs: zero runs of 1..7
bytes ending at m * T - 3 .. m * T + 3 (T the tile and the chunk, m 1..3) before each of the
followers 0, 1, 2, 3, 4, 0xff, as payload alone and behind a 7-byte head; the same runs split by the
head / payload junction at every split point (a head holds at most 64 bytes, so these heads are
s .. s + 9 and 58 .. 64 bytes long: the junction meets the tile boundary at 64 and no other); units
of 0, 1, T - 1, T, T + 1 bytes; a middle chunk of zeros and two in a row; units in a row of which one
ends in 00 00 and the next begins with 00; 2,000 random units of 0..3 chunks over {0, 0, 0, 1, 2, 3,
4, 0xff}; bins for a zero-word excess of 0, 1, 96, 97 (and a negative one, and 41 words) at bit
depths 8 and 10.

Also here (no GPU needed): tests/nal_ref.py, the reference of the GPU tests, against the serial C
loop through libjmhost; the DeviceNAL key's rejections; the additive ABI."""
import ctypes
import fcntl
import os
import re
import subprocess

import numpy as np
import pytest

import nal_cases
import nal_ref
from jmpaths import HARNESS, HEADER, LENCOD_CPU, LIBJMHIP, LIBJMHOST, ensure_built, load_jmhip

ASAN = os.path.join(HARNESS, "_build_asan")
CHECK = os.path.join(ASAN, "nal_core_check")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")


@pytest.fixture(scope="module")
def checker():
    with open(os.path.join(HARNESS, ".sanitize.lock"), "w") as lk:       # one sanitizer build at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", HARNESS, "-f", "nal_core.mk"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("nal_core_check build failed:\n" + r.stdout + r.stderr)
    return CHECK


def test_nal_core_equals_serial_packaging(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=600, env=ENV)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in log and "Sanitizer" not in log, log[-4000:]
    m = re.search(r"nal core check: (\d+) access units, (\d+) units, (\d+) escapes, (\d+) zero-word cases, (\d+) differ; an escape's zero run "
                  r"crossed a tile boundary (\d+) times, a chunk boundary (\d+), the junction (\d+), a chunk of zeros (\d+)", log)
    assert m, log[-2000:]
    aus, units, escapes, zero_cases, differ, tile, chunk, junction, zero_chunk = (int(v) for v in m.groups())
    print(log.strip().splitlines()[-1])
    assert differ == 0
    assert units >= 2000 + 2 * 2 * 3 * 7 * 7 * 6 and aus < units and escapes > 0 and zero_cases == 12
    assert tile >= 1 and chunk >= 1 and junction >= 1 and zero_chunk >= 1


class _Bits(ctypes.Structure):
    _fields_ = [("buf", ctypes.POINTER(ctypes.c_uint8)), ("cap", ctypes.c_long), ("len", ctypes.c_long), ("acc", ctypes.c_uint64),
                ("nacc", ctypes.c_int)]


def serial_nal(host, ref_idc, typ, rbsp):
    """host/bitstream.c › jm_write_nal through libjmhost"""
    src = (ctypes.c_uint8 * max(len(rbsp), 1)).from_buffer_copy(bytes(rbsp) or b"\0")
    r = _Bits(ctypes.cast(src, ctypes.POINTER(ctypes.c_uint8)), len(rbsp), len(rbsp), 0, 0)
    out = _Bits()
    host.jm_bits_init(ctypes.byref(out))
    host.jm_write_nal(ctypes.byref(out), ref_idc, typ, ctypes.byref(r))
    got = ctypes.string_at(out.buf, out.len)
    host.jm_bits_free(ctypes.byref(out))
    return got


def test_python_reference_equals_serial_loop():
    ensure_built()
    host = ctypes.CDLL(LIBJMHOST)
    host.jm_bits_init.restype = host.jm_bits_free.restype = host.jm_write_nal.restype = None
    assert nal_ref.nal_unit(3, 5, b"") == b"\x00\x00\x00\x01\x65"
    assert nal_ref.nal_unit(2, 1, b"\x00\x00\x00") == b"\x00\x00\x00\x01\x41\x00\x00\x03\x00"
    assert nal_ref.nal_unit(2, 1, b"\x00\x00\x00\x00\x00") == b"\x00\x00\x00\x01\x41\x00\x00\x03\x00\x00\x03\x00"
    assert nal_ref.nal_unit(0, 1, b"\x07\x00\x00\x04\x00\x00\x03\x00\x01") == b"\x00\x00\x00\x01\x01\x07\x00\x00\x04\x00\x00\x03\x03\x00\x01"
    rng = np.random.default_rng(3)
    tile, chunk = load_jmhip().nal_geometry()
    units = nal_cases.random_units(300, chunk, rng) + nal_cases.runs_around(tile) + nal_cases.runs_across_junction() + nal_cases.units_in_a_row()
    escapes = 0
    for ref_idc, typ, head, pay in units:
        want = serial_nal(host, ref_idc, typ, head + pay)
        assert nal_ref.nal_unit(ref_idc, typ, head + pay) == want
        if len(head) + len(pay) < 200:
            assert nal_ref.nal_unit_bytewise(ref_idc, typ, head + pay) == want
        escapes += len(want) - 5 - len(head) - len(pay)
    assert nal_ref.census(units, tile, chunk)["escapes"] == escapes > 0
    # the zero words: the inequality of 7.4.2.10 solved by search == the closed form of encode_picture_slices
    for unit, bins, bd, words in nal_cases.zero_word_cases(12):
        au, where = nal_ref.access_unit([unit], bins, 12, bd)
        plain, _ = nal_ref.access_unit([unit])
        assert len(au) == len(plain) + 3 * words and where[-1] == (0, len(au))
        assert nal_ref.zero_words_closed_form(bins, len(plain) - 4, 12, bd) == words
    for bins in range(1, 4000, 7):
        assert nal_ref.zero_words(bins, 100, 2, 8) == nal_ref.zero_words_closed_form(bins, 100, 2, 8)


def run_cpu(*args):
    ensure_built()
    return subprocess.run([LENCOD_CPU, *args], capture_output=True, text=True, timeout=120)


def test_device_nal_key_rejections():
    r = run_cpu("-p", "DeviceNAL=1")                                      # without the queued writer
    assert r.returncode != 0 and "DeviceNAL=1" in r.stderr and "DeviceWriterAsync=1" in r.stderr
    r = run_cpu("-p", "DeviceNAL=1", "-p", "DeviceCAVLC=1")
    assert r.returncode != 0 and "DeviceNAL=1" in r.stderr and "DeviceWriterAsync=1" in r.stderr
    r = run_cpu("-p", "DeviceNAL=1", "-p", "DeviceWriterAsync=1", "-p", "DeviceCAVLC=1")   # the CPU build has no device backend
    assert r.returncode != 0 and "DeviceNAL=1" in r.stderr and "device backend" in r.stderr
    r = run_cpu("-p", "DeviceNAL=2")
    assert r.returncode != 0 and "DeviceNAL" in r.stderr
    # 0 is the default and asks for nothing: the writer's own rejection
    r = run_cpu("-p", "DeviceNAL=0", "-p", "DeviceWriterAsync=1", "-p", "DeviceCAVLC=1")
    assert r.returncode != 0 and "DeviceNAL" not in r.stderr and "device backend" in r.stderr


def test_abi_is_additive(tmp_path):
    """The three entry points are exported and declared in include/jmhip_nal.h (which jmhip.h
    includes after jmhip_input.h); the ABI version stays 14 and jmhip.h's own declarations are the 37
    of ABI 14"""
    ensure_built()
    jm = load_jmhip()
    lib = ctypes.CDLL(LIBJMHIP)
    inc = os.path.dirname(HEADER)
    declared = lambda name: set(re.findall(r"\b(jmh_[a-z0-9_]+)\s*\(", open(os.path.join(inc, name)).read()))
    assert declared("jmhip_nal.h") == set(jm.EXPORTED_NAL) == {"jmh_nal_geometry", "jmh_nal_wrap", "jmh_coded_nal_heads"}
    out = subprocess.run(["nm", "-D", "--defined-only", LIBJMHIP], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r" T (jmh_[a-z0-9_]+)$", out, re.M))
    for name in jm.EXPORTED_NAL:
        assert name in defined and hasattr(lib, name), name
    text = open(HEADER).read()
    assert text.index('#include "jmhip_input.h"') < text.index('#include "jmhip_nal.h"')
    assert len(declared("jmhip.h")) == 37 and set(jm.EXPORTED).isdisjoint(jm.EXPORTED_NAL)
    assert declared("jmhip_coded.h") == set(jm.EXPORTED_CODED) and declared("jmhip_input.h") == set(jm.EXPORTED_INPUT)
    assert lib.jmh_abi_version() == 14 == jm.JMH_ABI_VERSION
    assert ctypes.sizeof(jm.JmhNalHead) == 76 and ctypes.sizeof(jm.JmhNalRange) == 16
    src = tmp_path / "hdr.c"
    src.write_text('#include "jmhip.h"\n#include "jmhip_nal.h"\n'
                   "_Static_assert(sizeof(jmh_nal_head) == 76 && sizeof(jmh_nal_range) == 16, \"layout\");\n"
                   "_Static_assert(JMH_NAL_HEAD_MAX >= 64 && JMH_ABI_VERSION == 14, \"values\");\n"
                   "int use(jmh_ctx *c, const jmh_nal_head *h) { return jmh_coded_nal_heads(c, 1, h); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "hdr.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # without a context every call that takes one is rejected through its status code
    ld = jm.load()
    assert ld.jmh_nal_wrap(None, 0, None, None, None, 0, None, 0, None, None) == jm.JMH_E_INVALID_ARG
    assert ld.jmh_coded_nal_heads(None, 0, None) == jm.JMH_E_INVALID_ARG
    assert ld.jmh_nal_geometry(None, None) == jm.JMH_E_INVALID_ARG


def test_geometry_needs_no_device():
    tile, chunk = load_jmhip().nal_geometry()
    assert tile >= 64 and tile % 64 == 0 and chunk % tile == 0 and chunk > tile
