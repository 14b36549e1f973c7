"""JM's spiral order as csrc/jmh_spiral.h states it (the text ordtab_fill of csrc/jmhip_abi.hip and
subpel_wave of csrc/jmh_analyse.hip compile), on the CPU.

tests/harness/spiral_check.c is a stand-alone C program built from the header with
-fsanitize=address,undefined -fno-sanitize-recover and run directly.  It generates the spiral by the
nested loops of Init_Motion_Search_Module (docs/JM_SEMANTICS.md item 5) and, for every search range
1..32 and every index, requires index -> position to give the loops' position, position -> index to
be its inverse, the ring number to be exact and the integer repair of a ring candidate off by one
either way (what the device's square root may hand it) to be exact too; and the three tables of the
per-context order table to be bit for bit those of the fill the header replaced."""
import fcntl
import os
import re
import subprocess

import pytest

from jmpaths import HARNESS

ASAN = os.path.join(HARNESS, "_build_asan")
CHECK = os.path.join(ASAN, "spiral_check")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")


@pytest.fixture(scope="module")
def checker():
    with open(os.path.join(HARNESS, ".sanitize.lock"), "w") as lk:       # one sanitizer build at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", HARNESS, "-f", "spiral.mk"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("spiral_check build failed:\n" + r.stdout + r.stderr)
    return CHECK


def test_spiral_is_jm_loops_and_tables_are_unchanged(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120, env=ENV)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in log and "Sanitizer" not in log, log[-4000:]
    m = re.search(r"spiral check: (\d+) ranges, (\d+) indices, (\d+) tables equal, (\d+) differ", log)
    assert m, log[-2000:]
    ranges, indices, tables, bad = (int(g) for g in m.groups())
    assert ranges == 32 and tables == 32 and bad == 0
    assert indices == sum((2 * sr + 1) ** 2 for sr in range(1, 33))
