"""The device CAVLC writer's shared per-macroblock core (csrc/jmh_cavlc_write.h, the text the kernels
of csrc/jmh_cavlc.hip compile) against the product's host writer (host/bitstream.c), on the CPU.

tests/harness/cavlc_core_check.c is a stand-alone C99 program built from the header, the host
library's sources and the oracle with -fsanitize=address,undefined -fno-sanitize-recover: it packs
the core's units serially, macroblock by macroblock, and compares every slice's bytes and bit count
with bitstream.c (through host/cavlc_ref.c) for four slice layouts (one slice, 1 MB, 7 MBs, one
row per slice) with varying lead bits -- on synthetic result sets (all-maximum levels, +-1 / 0
patterns, all P_Skip, P_Skip but the last, 200 random pictures, lead_nbits 0..7) and on the results
of the CPU encoder for the configurations below.  It also checks the documented per-macroblock bound
(JMW_MB_MAX_BITS) and that the counting sink and the writing sink agree.

Also here (no GPU needed): the DeviceCAVLC key's rejections, the additive ABI."""
import ctypes
import fcntl
import os
import re
import subprocess

import pytest

from jmpaths import HARNESS, HEADER, LENCOD_CPU, LIBJMHIP, ensure_built, load_jmhip

ASAN = os.path.join(HARNESS, "_build_asan")
CHECK = os.path.join(ASAN, "cavlc_core_check")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")

SMALL = ["FramesToBeEncoded=3", "SearchRange=8"]
ENCODED = [
    [],                                                                     # the synthetic sets only
    ["InputFile=synthetic:7", "SourceWidth=64", "SourceHeight=48", "QPFirstFrame=0", "QPRemainingFrame=0"] + SMALL,
    ["InputFile=synthetic:8", "SourceWidth=64", "SourceHeight=48", "QPFirstFrame=51", "QPRemainingFrame=51"] + SMALL,
    ["InputFile=synthetic:9", "QPFirstFrame=28", "QPRemainingFrame=28"] + SMALL,
    ["InputFile=synthetic:10", "SourceWidth=208", "SourceHeight=128", "ProfileIDC=100", "Transform8x8Mode=1", "SearchMode=3",
     "QPFirstFrame=30", "QPRemainingFrame=30"] + SMALL,
    ["InputFile=synthetic:11", "UseConstrainedIntraPred=1", "IntraPeriod=2"] + SMALL,
    ["InputFile=synthetic:12", "ProfileIDC=110", "SourceBitDepthLuma=10", "SourceBitDepthChroma=10", "QPFirstFrame=0",
     "QPRemainingFrame=0"] + SMALL,
    ["InputFile=synthetic:13", "RDOptimization=1", "SearchMode=3", "ProfileIDC=77"] + SMALL,
]


@pytest.fixture(scope="module")
def checker():
    with open(os.path.join(HARNESS, ".sanitize.lock"), "w") as lk:       # one sanitizer build at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", HARNESS, "-f", "cavlc_core.mk"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("cavlc_core_check build failed:\n" + r.stdout + r.stderr)
    return CHECK


@pytest.mark.parametrize("extra", ENCODED, ids=["synthetic"] + [c[0].split(":")[1] for c in ENCODED[1:]])
def test_core_equals_host_writer(checker, extra):
    args = [checker]
    for e in extra:
        args += ["-p", e]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600, env=ENV)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in log and "Sanitizer" not in log, log[-4000:]
    m = re.search(r"cavlc core check: (\d+) comparisons, (\d+) differ, largest macroblock (\d+) bits \(bound (\d+)\)", log)
    assert m, log[-2000:]
    n, bad, largest, bound = (int(v) for v in m.groups())
    assert bad == 0 and largest <= bound
    assert n >= 832 + (4 * 3 if extra else 0)             # every synthetic set, and every encoded picture in 4 layouts


def run_cpu(*args):
    ensure_built()
    return subprocess.run([LENCOD_CPU, *args], capture_output=True, text=True, timeout=120)


def test_device_cavlc_key_rejections():
    r = run_cpu("-p", "DeviceCAVLC=1", "-p", "SymbolMode=1", "-p", "ProfileIDC=77")
    assert r.returncode != 0 and "DeviceCAVLC=1" in r.stderr and "SymbolMode" in r.stderr
    r = run_cpu("-p", "DeviceCAVLC=1", "-p", "JMCallSurface=1")
    assert r.returncode != 0 and "DeviceCAVLC=1" in r.stderr and "JMCallSurface" in r.stderr
    r = run_cpu("-p", "DeviceCAVLC=2")
    assert r.returncode != 0 and "out of range" in r.stderr
    r = run_cpu("-p", "DeviceCAVLC=1")                     # the CPU build has no device writer
    assert r.returncode != 0 and "DeviceCAVLC=1" in r.stderr and "device backend" in r.stderr


def test_abi_is_additive():
    """The two entry points are exported and declared in include/jmhip_cavlc.h (which jmhip.h
    includes); the ABI version stays 14 and jmhip.h's own declarations are the 37 of ABI 14."""
    ensure_built()
    jm = load_jmhip()
    lib = ctypes.CDLL(LIBJMHIP)
    cavlc_h = open(os.path.join(os.path.dirname(HEADER), "jmhip_cavlc.h")).read()
    assert set(re.findall(r"\b(jmh_[a-z0-9_]+)\s*\(", cavlc_h)) == set(jm.EXPORTED_CAVLC) == {"jmh_cavlc_write_slices", "jmh_cavlc_write_results"}
    for name in jm.EXPORTED_CAVLC:
        assert hasattr(lib, name), name
    assert '#include "jmhip_cavlc.h"' in open(HEADER).read()
    assert lib.jmh_abi_version() == 14
    assert ctypes.sizeof(jm.JmhSliceDesc) == 20 and ctypes.sizeof(jm.JmhSliceBytes) == 24
    # without a context every call is rejected through its status code
    assert jm.load().jmh_cavlc_write_slices(None, 0, None, None, 0, None) == jm.JMH_E_INVALID_ARG
    assert jm.load().jmh_cavlc_write_results(None, None, 0, None, None, 0, None) == jm.JMH_E_INVALID_ARG


def test_host_reference_entry_checks_descriptors():
    """jm_cavlc_ref (libjmhost.so): the host writer behind the device call's arguments."""
    import numpy as np
    jm = load_jmhip()
    res = np.zeros(12, jm.MB_RESULT_DTYPE)                 # 64x48, all P_Skip
    one = jm.cavlc_ref(64, 48, 0, 0, res, jm.slice_descs(12, jm.JMH_P_SLICE))
    assert one == [bytes([0b00011011])]                    # ue(12) = 0001101, stop bit
    rows = jm.cavlc_ref(64, 48, 0, 0, res, jm.slice_descs(12, jm.JMH_P_SLICE, 4, lead=[(3, 0b101)]))
    assert rows == [bytes([0b10100101, 0b10000000])] * 3   # lead 101, ue(4) = 00101, stop bit
    gap = jm.slice_descs(12, jm.JMH_P_SLICE, 4)
    gap[1].first_mb = 5
    with pytest.raises(jm.JmhError) as e:
        jm.cavlc_ref(64, 48, 0, 0, res, gap)
    assert e.value.status == jm.JMH_E_INVALID_ARG
