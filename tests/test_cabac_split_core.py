"""The split CABAC coder's shared core (csrc/jmh_cabac_split.h, the text the kernels of
csrc/jmh_cabac_split.hip compile) against the product's host writer (host/cabac.c), on the CPU.

tests/harness/cabac_split_check.c is a stand-alone C99 program built from the header, the host
library's sources and the oracle with -fsanitize=address,undefined -fno-sanitize-recover: it runs
the core's passes serially (context maps and their composition, resolved records, range tables and
their composition, every chunk coded from low = 0 on the slice's byte grid, tails, region sums, the
carry evaluation) and compares every slice's bytes and bin count with jm_cabac_ref
(host/cabac_ref.c) -- on the synthetic result sets of cabac_core_check (every level category at
+-1 .. +-32767 / -32768 with and without the 8x8 transform, the mvd extremes, all P_Skip, P_Skip
but the last, 200 random pictures) in four slice layouts (one slice, 1 MB, 7 MBs, one row per
slice), and on raw random record streams (bypass-heavy, LPS-heavy, terminate-sprinkled) against the
serial core coder.  Every slice of every input is coded at the chunk lengths 1, 2, 3, 7, 8, 64, 1000
and one longer than the slice, and at nbins (one chunk), nbins - 1 (the last chunk is the closing
terminate bin and the flush alone) and (nbins + 1) / 2: eleven codings per slice.

A carry must cross at least two chunk boundaries, and so must a run of 0xff bytes that no carry
reached: the multi-chunk case of what jmc_byte_out's held / nheld resolve inside one coder.  Only
boundaries between regions that hold bytes count (at small L many chunks shift nothing and own no
byte; a carry passing them proves nothing).  Required over all lengths and at L = 8 alone, where a
235-bit outstanding run (test_cabac_core.py) spans at least 34 bins, more than four chunks.  Found:
a carry across 3 such boundaries and a 0xff run across 28; at L = 8, 3 and 11.

Also here (no GPU needed): the DeviceCABACSplit key's rejections, the additive ABI."""
import ctypes
import fcntl
import os
import re
import subprocess

import pytest

from jmpaths import HARNESS, HEADER, LENCOD_CPU, LIBJMHIP, ensure_built, load_jmhip

ASAN = os.path.join(HARNESS, "_build_asan")
CHECK = os.path.join(ASAN, "cabac_split_check")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")


@pytest.fixture(scope="module")
def checker():
    with open(os.path.join(HARNESS, ".sanitize.lock"), "w") as lk:       # one sanitizer build at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", HARNESS, "-f", "cabac_split.mk"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("cabac_split_check build failed:\n" + r.stdout + r.stderr)
    return CHECK


def test_split_core_equals_host_writer(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=1500, env=ENV)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in log and "Sanitizer" not in log, log[-4000:]
    m = re.search(r"cabac split check: (\d+) slices, (\d+) codings, (\d+) chunks, (\d+) whole range tables, (\d+) differ; "
                  r"a carry crossed up to (\d+) chunk boundaries, a 0xff run that did not carry up to (\d+); at L = 8: (\d+) and (\d+)", log)
    assert m, log[-2000:]
    slices, codings, chunks, tables, bad, carry, ffrun, carry8, ffrun8 = (int(v) for v in m.groups())
    print(log.strip().splitlines()[-1])
    assert bad == 0
    # 228 result sets in 4 layouts of 1 + 12 + 2 + 3 slices, and 60 raw streams; 8 listed lengths and the slice's own 3 each
    assert slices == 228 * 18 + 60 and codings == 11 * slices and chunks > codings and tables > 0
    assert carry >= 2 and ffrun >= 2
    assert carry8 >= 2 and ffrun8 >= 2


def run_cpu(*args):
    ensure_built()
    return subprocess.run([LENCOD_CPU, *args], capture_output=True, text=True, timeout=120)


def test_device_cabac_split_key_rejections():
    cabac = ["-p", "SymbolMode=1", "-p", "ProfileIDC=77"]
    r = run_cpu("-p", "DeviceCABACSplit=64", *cabac)                     # without the device writer
    assert r.returncode != 0 and "DeviceCABACSplit=64" in r.stderr and "DeviceCABAC=1" in r.stderr
    r = run_cpu("-p", "DeviceCABACSplit=15", "-p", "DeviceCABAC=1", *cabac)
    assert r.returncode != 0 and "DeviceCABACSplit=15" in r.stderr and "DeviceCABAC=1" in r.stderr and "16" in r.stderr
    r = run_cpu("-p", "DeviceCABACSplit=65537", "-p", "DeviceCABAC=1", *cabac)
    assert r.returncode != 0 and "out of range" in r.stderr
    r = run_cpu("-p", "DeviceCABACSplit=-1", "-p", "DeviceCABAC=1", *cabac)
    assert r.returncode != 0 and "out of range" in r.stderr
    r = run_cpu("-p", "DeviceCABACSplit=64", "-p", "DeviceCABAC=1", *cabac)   # the CPU build has no device writer
    assert r.returncode != 0 and "DeviceCABACSplit=64" in r.stderr and "DeviceCABAC=1" in r.stderr and "device backend" in r.stderr
    # 0 is the default and asks for nothing: the device writer's own rejection
    r = run_cpu("-p", "DeviceCABACSplit=0", "-p", "DeviceCABAC=1", *cabac)
    assert r.returncode != 0 and "DeviceCABACSplit" not in r.stderr and "device backend" in r.stderr


def test_abi_is_additive():
    """The three entry points are exported and declared in include/jmhip_cabac_split.h (which jmhip.h
    includes after jmhip_coded.h); the ABI version stays 14 and jmhip.h's own declarations are the 37
    of ABI 14; the other writer headers declare what they declared."""
    ensure_built()
    jm = load_jmhip()
    lib = ctypes.CDLL(LIBJMHIP)
    inc = os.path.dirname(HEADER)
    declared = lambda name: set(re.findall(r"\b(jmh_[a-z0-9_]+)\s*\(", open(os.path.join(inc, name)).read()))
    assert declared("jmhip_cabac_split.h") == set(jm.EXPORTED_CABAC_SPLIT) == {"jmh_cabac_set_split", "jmh_cabac_get_split", "jmh_cabac_split_stats"}
    for name in jm.EXPORTED_CABAC_SPLIT:
        assert hasattr(lib, name), name
    text = open(HEADER).read()
    assert text.index('#include "jmhip_coded.h"') < text.index('#include "jmhip_cabac_split.h"')
    assert len(declared("jmhip.h")) == 37
    assert declared("jmhip_cabac.h") == set(jm.EXPORTED_CABAC) and declared("jmhip_coded.h") == set(jm.EXPORTED_CODED)
    assert declared("jmhip_cavlc.h") == set(jm.EXPORTED_CAVLC)
    assert lib.jmh_abi_version() == 14
    assert ctypes.sizeof(jm.JmhCabacSplitInfo) == 32
    # without a context every call is rejected through its status code
    assert jm.load().jmh_cabac_set_split(None, 64) == jm.JMH_E_INVALID_ARG
    assert jm.load().jmh_cabac_get_split(None) == jm.JMH_E_INVALID_ARG
    assert jm.load().jmh_cabac_split_stats(None, ctypes.byref(jm.JmhCabacSplitInfo())) == jm.JMH_E_INVALID_ARG
