"""The device CABAC writer's shared core (csrc/jmh_cabac_write.h, the text the kernels of
csrc/jmh_cabac.hip compile) against the product's host writer (host/cabac.c), on the CPU.

tests/harness/cabac_core_check.c is a stand-alone C99 program built from the header, the host
library's sources and the oracle with -fsanitize=address,undefined -fno-sanitize-recover: it
binarises every macroblock unit by unit into bin records (counting and storing sink), codes the
records with the core's arithmetic encoder and compares every slice's bytes and bin count with
cabac.c (through host/cabac_ref.c) for four slice layouts (one slice, 1 MB, 7 MBs, one row per
slice) -- on synthetic result sets (every level category at +-1, +-2, +-14, +-15, +-16 and
+-32767 / -32768 with and without the 8x8 transform, mvd steps of 8, 9, 10 and the int16_t
extremes over every partition type, all P_Skip, P_Skip but the last, 200 random pictures; slice QPs
cycle through 0, 26, 51) and on the results of the CPU encoder for the configurations below.  It
also checks the documented bounds (JMC_MB_MAX_BINS, JMC_SLICE_MAX_BYTES).

The longest run of outstanding bits the host writer resolved must reach 8 (a carry across a whole
output byte, where the core's byte output differs in method from PutBit).  Found: 235 bits in the
synthetic sets alone (the all-+-32767 pictures), so every invocation meets it.

Also here (no GPU needed): the DeviceCABAC key's rejections, the additive ABI, jm_cabac_ref's
descriptor checks."""
import ctypes
import fcntl
import os
import re
import subprocess

import pytest

from jmpaths import HARNESS, HEADER, LENCOD_CPU, LIBJMHIP, ensure_built, load_jmhip

ASAN = os.path.join(HARNESS, "_build_asan")
CHECK = os.path.join(ASAN, "cabac_core_check")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")

SMALL = ["FramesToBeEncoded=3", "SearchRange=8", "SymbolMode=1"]
ENCODED = [
    [],                                                                     # the synthetic sets only
    ["InputFile=synthetic:7", "SourceWidth=64", "SourceHeight=48", "QPFirstFrame=0", "QPRemainingFrame=0", "ProfileIDC=77"] + SMALL,
    ["InputFile=synthetic:8", "SourceWidth=64", "SourceHeight=48", "QPFirstFrame=51", "QPRemainingFrame=51", "ProfileIDC=77"] + SMALL,
    ["InputFile=synthetic:9", "QPFirstFrame=28", "QPRemainingFrame=28", "ProfileIDC=77"] + SMALL,
    ["InputFile=synthetic:10", "SourceWidth=208", "SourceHeight=128", "ProfileIDC=100", "Transform8x8Mode=1", "SearchMode=3",
     "QPFirstFrame=30", "QPRemainingFrame=30"] + SMALL,
    ["InputFile=synthetic:11", "UseConstrainedIntraPred=1", "IntraPeriod=2", "ProfileIDC=77"] + SMALL,
    ["InputFile=synthetic:12", "ProfileIDC=110", "SourceBitDepthLuma=10", "SourceBitDepthChroma=10", "QPFirstFrame=0",
     "QPRemainingFrame=0"] + SMALL,
    ["InputFile=synthetic:13", "RDOptimization=1", "SearchMode=3", "ProfileIDC=77"] + SMALL,
]


@pytest.fixture(scope="module")
def checker():
    with open(os.path.join(HARNESS, ".sanitize.lock"), "w") as lk:       # one sanitizer build at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", HARNESS, "-f", "cabac_core.mk"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("cabac_core_check build failed:\n" + r.stdout + r.stderr)
    return CHECK


@pytest.mark.parametrize("extra", ENCODED, ids=["synthetic"] + [c[0].split(":")[1] for c in ENCODED[1:]])
def test_core_equals_host_writer(checker, extra):
    args = [checker]
    for e in extra:
        args += ["-p", e]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600, env=ENV)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in log and "Sanitizer" not in log, log[-4000:]
    m = re.search(r"cabac core check: (\d+) comparisons, (\d+) differ, largest macroblock (\d+) bins \(bound (\d+)\), "
                  r"longest outstanding run (\d+) bits", log)
    assert m, log[-2000:]
    n, bad, largest, bound, run = (int(v) for v in m.groups())
    print(log.strip().splitlines()[-1])
    assert bad == 0 and largest <= bound
    assert run >= 8
    assert n >= 912 + (4 * 3 if extra else 0)             # every synthetic set, and every encoded picture in 4 layouts


def run_cpu(*args):
    ensure_built()
    return subprocess.run([LENCOD_CPU, *args], capture_output=True, text=True, timeout=120)


def test_device_cabac_key_rejections():
    r = run_cpu("-p", "DeviceCABAC=1", "-p", "SymbolMode=0")
    assert r.returncode != 0 and "DeviceCABAC=1" in r.stderr and "SymbolMode" in r.stderr
    r = run_cpu("-p", "DeviceCABAC=1", "-p", "SymbolMode=1", "-p", "ProfileIDC=77", "-p", "JMCallSurface=1")
    assert r.returncode != 0 and "DeviceCABAC=1" in r.stderr and "JMCallSurface" in r.stderr
    r = run_cpu("-p", "DeviceCABAC=2")
    assert r.returncode != 0 and "out of range" in r.stderr
    r = run_cpu("-p", "DeviceCABAC=1", "-p", "SymbolMode=1", "-p", "ProfileIDC=77")   # the CPU build has no device writer
    assert r.returncode != 0 and "DeviceCABAC=1" in r.stderr and "device backend" in r.stderr
    # the CAVLC key's rejection still names both of its keys
    r = run_cpu("-p", "DeviceCAVLC=1", "-p", "SymbolMode=1", "-p", "ProfileIDC=77")
    assert r.returncode != 0 and "DeviceCAVLC=1" in r.stderr and "SymbolMode" in r.stderr


def test_abi_is_additive():
    """The two entry points are exported and declared in include/jmhip_cabac.h (which jmhip.h includes
    after jmhip_cavlc.h); the ABI version stays 14 and jmhip.h's own declarations are the 37 of ABI 14."""
    ensure_built()
    jm = load_jmhip()
    lib = ctypes.CDLL(LIBJMHIP)
    cabac_h = open(os.path.join(os.path.dirname(HEADER), "jmhip_cabac.h")).read()
    assert set(re.findall(r"\b(jmh_[a-z0-9_]+)\s*\(", cabac_h)) == set(jm.EXPORTED_CABAC) == {"jmh_cabac_write_slices", "jmh_cabac_write_results"}
    for name in jm.EXPORTED_CABAC:
        assert hasattr(lib, name), name
    text = open(HEADER).read()
    assert text.index('#include "jmhip_cavlc.h"') < text.index('#include "jmhip_cabac.h"')
    assert len(set(re.findall(r"\b(jmh_[a-z0-9_]+)\s*\(", text))) == 37
    assert lib.jmh_abi_version() == 14
    assert ctypes.sizeof(jm.JmhCabacSliceDesc) == 16 and ctypes.sizeof(jm.JmhCabacSliceBytes) == 24
    # without a context every call is rejected through its status code
    assert jm.load().jmh_cabac_write_slices(None, 0, None, None, 0, None) == jm.JMH_E_INVALID_ARG
    assert jm.load().jmh_cabac_write_results(None, None, 0, None, None, 0, None) == jm.JMH_E_INVALID_ARG


def test_host_reference_entry_checks_descriptors():
    """jm_cabac_ref (libjmhost.so): the host writer behind the device call's arguments."""
    import numpy as np
    jm = load_jmhip()
    res = np.zeros(12, jm.MB_RESULT_DTYPE)                 # 64x48, all P_Skip
    P, I = jm.JMH_P_SLICE, jm.JMH_I_SLICE
    one, where = jm.cabac_ref(64, 48, 0, 0, res, jm.cabac_slice_descs(12, P, 26), with_where=True)
    # 12 mb_skip_flag, 11 end_of_slice_flag 0, one end_of_slice_flag 1
    assert where == [(0, len(one[0]), 24)] and one[0][-1] != 0   # the last byte holds the rbsp_stop_one_bit
    rows, where = jm.cabac_ref(64, 48, 0, 0, res, jm.cabac_slice_descs(12, P, (0, 26, 51), 4), with_where=True)
    assert [w[2] for w in where] == [8, 8, 8] and [w[0] for w in where] == [0, len(rows[0]), len(rows[0]) + len(rows[1])]
    same = jm.cabac_ref(64, 48, 0, 0, res, jm.cabac_slice_descs(12, P, 26, 4))
    assert same[0] == same[1] == same[2]                   # the same macroblocks at the same QP
    gap = jm.cabac_slice_descs(12, P, 26, 4)
    gap[1].first_mb = 5
    over = jm.cabac_slice_descs(12, P, 26, 4)
    over[2].n_mb = 5
    short = (jm.JmhCabacSliceDesc * 2)(*jm.cabac_slice_descs(12, P, 26, 4)[:2])
    btype = jm.cabac_slice_descs(12, P, 26)
    btype[0].slice_type = 1
    qp52, qpneg = jm.cabac_slice_descs(12, I, 52), jm.cabac_slice_descs(12, I, -1)
    for bad in (gap, over, short, btype, qp52, qpneg):
        with pytest.raises(jm.JmhError) as e:
            jm.cabac_ref(64, 48, 0, 0, res, bad)
        assert e.value.status == jm.JMH_E_INVALID_ARG
    total = sum(len(r) for r in rows)
    with pytest.raises(jm.JmhError) as e:                  # cap one byte short
        jm.cabac_ref(64, 48, 0, 0, res, jm.cabac_slice_descs(12, P, (0, 26, 51), 4), cap=total - 1)
    assert e.value.status == jm.JMH_E_INVALID_ARG
    assert jm.cabac_ref(64, 48, 0, 0, res, jm.cabac_slice_descs(12, P, (0, 26, 51), 4), cap=total) == rows
