"""Coded pictures, the parts that need no GPU: the DeviceWriterAsync key of lencod, the exported
entry points of include/jmhip_coded.h, and the PSNR that the frame loop derives from the device's
SSDs (host/encoder.c jm_psnr_from_ssd) against psnr_pl."""
import ctypes
import os
import re
import subprocess

import pytest

from jmpaths import HARNESS, LENCOD_CPU, LIBJMHIP, ROOT, ensure_built, load_jmhip

jmhip = load_jmhip()
CODED_HEADER = os.path.join(ROOT, "include", "jmhip_coded.h")
CHECK = os.path.join(HARNESS, "_build_asan", "psnr_ssd_check")


def run(*args):
    ensure_built()
    return subprocess.run([LENCOD_CPU, *args], capture_output=True, text=True, timeout=120)


def test_async_key_needs_a_device_writer():
    r = run("-p", "DeviceWriterAsync=1")
    assert r.returncode != 0
    assert "DeviceWriterAsync=1" in r.stderr and "DeviceCAVLC=1" in r.stderr and "DeviceCABAC=1" in r.stderr
    r = run("-p", "DeviceWriterAsync=2")
    assert r.returncode != 0 and "out of range" in r.stderr


def test_async_key_needs_the_pipelined_path():
    r = run("-p", "DeviceWriterAsync=1", "-p", "DeviceCAVLC=1", "-p", "PipelineDepth=1")
    assert r.returncode != 0 and "DeviceWriterAsync=1" in r.stderr and "PipelineDepth" in r.stderr


def test_async_key_rejected_on_the_cpu_build_like_the_device_writer():
    for key in ("DeviceCAVLC=1", "DeviceCABAC=1"):
        extra = ["-p", "SymbolMode=1", "-p", "ProfileIDC=77"] if "CABAC" in key else []
        alone = run("-p", key, *extra)
        both = run("-p", key, "-p", "DeviceWriterAsync=1", *extra)
        assert alone.returncode != 0 and "needs the device backend" in alone.stderr
        assert both.returncode == alone.returncode and "needs the device backend" in both.stderr


def test_exported_and_declared():
    ensure_built()
    src = open(CODED_HEADER).read()
    declared = sorted(set(re.findall(r"\b(jmh_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(jmhip.EXPORTED_CODED)
    assert {"jmh_frame_push_coded", "jmh_frame_push_coded_u16", "jmh_frame_pop_coded"} <= set(declared)
    lib = ctypes.CDLL(LIBJMHIP)
    for n in declared:
        assert hasattr(lib, n), n
    assert '#include "jmhip_coded.h"' in open(os.path.join(ROOT, "include", "jmhip.h")).read()
    assert jmhip.load().jmh_abi_version() == 14                    # additive
    # the mirrors' layouts (include/jmhip_coded.h)
    assert ctypes.sizeof(jmhip.JmhCodedSlice) == 24 and ctypes.sizeof(jmhip.JmhCodedBytes) == 32
    assert ctypes.sizeof(jmhip.JmhCodedStats) == 32 and jmhip.JmhCodedStats.fallback.offset == 24


def test_null_context_is_rejected():
    lib = jmhip.load()
    assert lib.jmh_frame_pop_coded(None, None, 0, None, None) == jmhip.JMH_E_INVALID_ARG
    assert lib.jmh_coded_ring_entries(None) == jmhip.JMH_E_INVALID_ARG


def test_descriptor_helpers():
    d = jmhip.coded_slice_descs(12, jmhip.JMH_P_SLICE, 30, 5, lead=[(3, 0b101), (0, 0)])
    assert [(x.first_mb, x.n_mb, x.slice_type, x.slice_qp, x.lead_nbits, x.lead_bits) for x in d] == \
        [(0, 5, 0, 30, 3, 5), (5, 5, 0, 30, 0, 0), (10, 2, 0, 30, 3, 5)]
    a, b = jmhip.split_coded(d)
    assert [(x.first_mb, x.n_mb, x.lead_nbits) for x in a] == [(0, 5, 3), (5, 5, 0), (10, 2, 3)]
    assert [(x.first_mb, x.n_mb, x.slice_qp) for x in b] == [(0, 5, 30), (5, 5, 30), (10, 2, 30)]
    r = jmhip.coded_from_runs([5, 5, 2], jmhip.JMH_P_SLICE, 30, lead=[(3, 0b101), (0, 0)])
    assert bytes(r) == bytes(d)


def test_psnr_from_ssd_equals_psnr_pl():
    """a stand-alone host program (ASan + UBSan), random 8-, 9- and 10-bit planes, with and without a crop"""
    r = subprocess.run(["make", "-s", "-C", HARNESS, "-f", "psnr_ssd.mk"], capture_output=True, text=True)
    if r.returncode:
        pytest.fail("psnr_ssd_check build failed:\n" + r.stdout + r.stderr)
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and r.stdout.count("plane") == 24
