"""The search kernels' spiral decode on the device (csrc/jmh_spiral.h jms_decode_dev, what subpel_wave
of k_mb_analyse and k_mb_flow calls) against the table.

The decode takes its ring candidate from the device's own square root instruction and repairs it in
integers; tests/test_spiral_core.py proves the repair for any candidate off by one, this test that the
instruction's candidate is never further off: jmh_spiral_positions (include/jmhip_spiral.h) runs the
device function over every index of search ranges 1, 8 and 32 in one small launch each, and the
positions must be those of JM's loops (Init_Motion_Search_Module, restated below) -- which is also
what the context's index -> position table holds (tests/harness/spiral_check.c)."""
import numpy as np
import pytest

from jmpaths import ensure_built, load_jmhip

jmhip = load_jmhip()


def jm_spiral(sr):
    """Init_Motion_Search_Module: the positions in search order, [(2 sr + 1)^2][2] as (x, y)"""
    pos = [(0, 0)]
    for l in range(1, max(1, sr) + 1):
        for i in range(-l + 1, l):
            pos += [(i, -l), (i, l)]
        for i in range(-l, l + 1):
            pos += [(-l, i), (l, i)]
    return np.array(pos, np.int32)


def test_loops_cover_the_window():
    """CPU: the restated loops give every position of the window once, ring by ring"""
    for sr in (1, 8, 32):
        p = jm_spiral(sr)
        assert len(p) == (2 * sr + 1) ** 2 == len({(int(x), int(y)) for x, y in p})
        ring = np.abs(p).max(axis=1)
        assert (np.diff(ring) >= 0).all() and ring[-1] == sr
        for l in range(1, sr + 1):
            assert int(np.flatnonzero(ring == l)[0]) == (2 * l - 1) ** 2


@pytest.mark.gpu
def test_device_decode_is_the_table():
    ensure_built()
    jmhip.load()
    enc = jmhip.Encoder(32, 32, search_range=8)
    try:
        for sr in (1, 8, 32):
            got = enc.spiral_positions(sr)
            want = jm_spiral(sr)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, f"search range {sr}: index {int(bad[0])} decodes to {got[bad[0]].tolist()}, the spiral has {want[bad[0]].tolist()}"
    finally:
        enc.close()
