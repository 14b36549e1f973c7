"""k_mb_flow's neighbour fetches where they degenerate: dataflow == ticks == oracle, bit for bit, on
pictures of one macroblock, one row, one column and 3 x 2 macroblocks.

After its dependency wait a macroblock fetches its neighbours' border cells (ref_idx, the MV pair as
one word, the Intra4x4 mode), its intra neighbourhood and its search window, and its final fetches
the left / top neighbours' deblocked samples and results.  Every one of these loads is predicated on
the neighbour's availability, and the window is clamped at the picture's edges:

  16x16   no neighbour at all: every border / intra / deblocking load is off
  48x16   one row: no top, top-left or top-right neighbour
  16x48   one column: no left neighbour, the top-right one never available
  48x32   macroblock (1, 1) has all four neighbours, (2, 1) takes D for C, the row's first has no left

The sequences are I P P chains with deblocking on, of the hand-off test's pan (a picture that moves
by (3, -2) samples per picture), so the border MVs are not zero and the window is clamped at every
edge.  The chains go through test_flow_chain_gpu's helpers (the oracle's encode plus deblock_ref's
loop filter, each P picture on the previous deblocked one); test_border_cells_carry_motion checks on
the CPU, from the oracle's results alone, that the 48x32 chain gives what the GPU test relies on.
"""
import numpy as np
import pytest

import test_flow_chain_gpu as fc
from jmpaths import ensure_built, load_jmhip
from test_flow_handoff_gpu import pan_seq
from test_gpu_parity import assert_same

jmhip = load_jmhip()
INTER = (0, 1, 2, 3, 8)                       # P_Skip, 16x16, 16x8, 8x16, P8x8

# name -> (width, height, pictures, encoder settings): cases of test_flow_chain_gpu's helpers
# (oracle_chain, device_chain), under names of their own
EDGE_CASES = {
    "edge16x16": (16, 16, lambda: pan_seq(16, 16, 3, 3), dict(search_range=32)),
    "edge48x16": (48, 16, lambda: pan_seq(48, 16, 3, 3), dict(search_range=32)),
    "edge16x48": (16, 48, lambda: pan_seq(16, 48, 3, 3), dict(search_range=32)),
    "edge48x32": (48, 32, lambda: pan_seq(48, 32, 3, 3), dict(search_range=32)),
}
fc.CASES.update(EDGE_CASES)


def border_cells(mbx, mby, mbw):
    """(macroblock index, 4x4 block) of the border cells load_border reads for macroblock (mbx, mby):
    the row above from the top-left to the top-right neighbour, the column to the left."""
    cells = []
    if mby > 0:
        if mbx > 0:
            cells.append(((mby - 1) * mbw + mbx - 1, 15))
        cells += [((mby - 1) * mbw + mbx, 12 + k) for k in range(4)]
        if mbx + 1 < mbw:
            cells.append(((mby - 1) * mbw + mbx + 1, 12))
    if mbx > 0:
        cells += [(mby * mbw + mbx - 1, 4 * k + 3) for k in range(4)]
    return cells


def test_border_cells_carry_motion():
    """CPU: in a P picture of the 48x32 chain macroblocks (1, 1) and (2, 1) are inter, and at least
    one border cell each of them reads has a non-zero MV."""
    mbw = 3
    ok = []
    for i, (res, _, _) in enumerate(fc.oracle_chain("edge48x32")[1:], 1):
        inter = all(int(res["mb_type"][mby * mbw + mbx]) in INTER for mbx, mby in ((1, 1), (2, 1)))
        moving = all(any(res["mv"][m][k].any() for m, k in border_cells(mbx, mby, mbw)) for mbx, mby in ((1, 1), (2, 1)))
        print(f"picture {i}: mb_type {res['mb_type'].tolist()}, (1,1) and (2,1) inter: {inter}, border MVs non-zero: {moving}")
        ok.append(inter and moving)
    assert any(ok), "no P picture with inter macroblocks (1, 1) and (2, 1) that read a non-zero border MV"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_edges_flow_ticks_oracle(name):
    """dataflow == ticks == oracle: every result field, every reconstruction and deblocked plane."""
    ensure_built()
    jmhip.load()
    w = EDGE_CASES[name][0]
    want = fc.oracle_chain(name)
    for flow in (1, 0):
        got = fc.device_chain(name, flow)
        assert len(got) == len(want)
        for i, ((gres, grec, gdbk), (ores, orec, odbk)) in enumerate(zip(got, want)):
            assert_same(gres, grec, ores, orec, w // 16)
            for pl, (x, y) in enumerate(zip(gdbk, odbk)):
                assert np.array_equal(x, y), f"JMH_FLOW={flow} picture {i}: deblocked plane {pl} differs from the oracle chain"
