"""The deblocking reference (tests/deblock_ref.py, written from H.264 8.7) before any GPU is
involved: hand-worked lines for every branch of 8.7.2.3 / 8.7.2.4, the table corners, and
reference == the product's host deblocker (host/deblock.c through jmhip.deblock_ref) on the CPU
oracle's pictures for every case of deblock_cases.py and a sweep over the thresholds.

Every expected value below was worked out by hand from the standard's formulae, with
alpha = 20, beta = 7 (indexA = indexB = 28) unless stated: (alpha >> 2) + 2 = 7.
"""
import numpy as np
import pytest

import deblock_cases as dc
import deblock_ref as dr
import oracle_lib
from jmpaths import ensure_built, load_jmhip

jmhip = load_jmhip()
A, B = 20, 7


@pytest.fixture(scope="module", autouse=True)
def built():
    ensure_built()


def line(p, q, bS, tc0, chroma=False, alpha=A, beta=B, maxv=255):
    np_, nq, notes = dr.filter_samples(list(p), list(q), bS, alpha, beta, tc0, chroma, maxv)
    return np_, nq, set(notes)


# ---------------- the gate (8-468) ----------------
@pytest.mark.parametrize("p,q", [
    ([100, 100, 100, 100], [120, 120, 120, 120]),     # |p0 - q0| = 20 = alpha
    ([100, 107, 100, 100], [104, 104, 104, 104]),     # |p1 - p0| = 7 = beta
    ([100, 100, 100, 100], [104, 111, 104, 104]),     # |q1 - q0| = 7 = beta
])
@pytest.mark.parametrize("bS", [1, 4])
def test_gate_rejects(p, q, bS):
    assert line(p, q, bS, 2) == (p, q, {"gated"})


def test_gate_passes_one_below_each_threshold():
    # |p0 - q0| = 19, |p1 - p0| = 6, |q1 - q0| = 6; ap = aq = 19: tc = tc0 = 2
    # raw = (4 * 19 + (94 - 125) + 4) >> 3 = 49 >> 3 = 6 -> 2
    np_, nq, notes = line([100, 94, 119, 0], [119, 125, 100, 0], 2, 2)
    assert (np_, nq) == ([102, 94, 119, 0], [117, 125, 100, 0]) and notes == {"filt", "delta_clipped"}


def test_bs0_is_never_filtered():
    assert line([100] * 4, [104] * 4, 0, 0)[2] == {"gated"}


# ---------------- bS < 4, luma (8.7.2.3), tc0 = 2 ----------------
def test_weak_neither_side_flat():
    # ap = aq = 7 = beta: tc = 2; raw = (32 + (102 - 106) + 4) >> 3 = 4 -> +tc = 2
    np_, nq, notes = line([100, 102, 107, 110], [108, 106, 115, 120], 3, 2)
    assert (np_, nq) == ([102, 102, 107, 110], [106, 106, 115, 120])
    assert notes == {"filt", "delta_clipped"}


def test_weak_p_side_flat():
    # ap = 3: tc = 3, delta = 3 (raw 4); p1' = 102 + Clip3(-2, 2, (103 + 104 - 204) >> 1 = 1) = 103
    np_, nq, notes = line([100, 102, 103, 110], [108, 106, 120, 120], 3, 2)
    assert (np_, nq) == ([103, 103, 103, 110], [105, 106, 120, 120])
    assert notes == {"filt", "delta_clipped", "p1_mod"}


def test_weak_both_sides_flat():
    # tc = 4, delta = raw = 4; q1' = 106 + Clip3(-2, 2, (105 + 104 - 212) >> 1 = -2) = 104
    np_, nq, notes = line([100, 102, 103, 110], [108, 106, 105, 120], 3, 2)
    assert (np_, nq) == ([104, 103, 103, 110], [104, 104, 105, 120])
    assert notes == {"filt", "p1_mod", "q1_mod"}


def test_weak_delta_clipped_at_minus_tc():
    # raw = (-32 + (106 - 102) + 4) >> 3 = -24 >> 3 = -3 -> -tc = -2
    np_, nq, notes = line([108, 106, 120, 120], [100, 102, 110, 110], 1, 2)
    assert (np_, nq) == ([106, 106, 120, 120], [102, 102, 110, 110])
    assert notes == {"filt", "delta_clipped"}


def test_weak_p1_clipped_at_tc0():
    # delta = (0 + 0 + 4) >> 3 = 0; p1' = 100 + Clip3(-2, 2, (106 + 100 - 200) >> 1 = 3) = 102
    np_, nq, notes = line([100, 100, 106, 106], [100, 100, 100, 100], 2, 2)
    assert (np_, nq) == ([100, 102, 106, 106], [100, 100, 100, 100])
    assert notes == {"filt", "p1_mod", "q1_mod"}


def test_clip1_at_255():
    # tc = 4; raw = (0 + (255 - 250) + 4) >> 3 = 1: p0' = Clip1(256) = 255, q0' = 254
    # q1' = 250 + Clip3(-2, 2, (250 + 255 - 500) >> 1 = 2) = 252
    np_, nq, notes = line([255, 255, 255, 255], [255, 250, 250, 250], 1, 2)
    assert (np_, nq) == ([255, 255, 255, 255], [254, 252, 250, 250])
    assert notes == {"filt", "clip1_hi", "p1_mod", "q1_mod"}


def test_clip1_at_0():
    # raw = (0 + (0 - 5) + 4) >> 3 = -1: p0' = Clip1(-1) = 0, q0' = 1
    # q1' = 5 + Clip3(-2, 2, (5 + 0 - 10) >> 1 = -3) = 3
    np_, nq, notes = line([0, 0, 0, 0], [0, 5, 5, 5], 1, 2)
    assert (np_, nq) == ([0, 0, 0, 0], [1, 3, 5, 5])
    assert notes == {"filt", "clip1_lo", "p1_mod", "q1_mod"}


def test_clip1_at_1023():
    # 10 bits: alpha = 80, beta = 28, tc0 = 8; tc = 10; raw = (0 + 20 + 4) >> 3 = 3: p0' = Clip1(1026) = 1023
    # q1' = 1003 + Clip3(-8, 8, (1003 + 1023 - 2006) >> 1 = 10) = 1011
    np_, nq, notes = line([1023] * 4, [1023, 1003, 1003, 1003], 1, 8, alpha=80, beta=28, maxv=1023)
    assert (np_, nq) == ([1023, 1023, 1023, 1023], [1020, 1011, 1003, 1003])
    assert notes == {"filt", "clip1_hi", "p1_mod", "q1_mod"}


# ---------------- bS 4, luma (8.7.2.4) ----------------
def test_strong_both_sides():
    # |p0 - q0| = 4 < 7, ap = aq = 2
    # p0' = (102 + 202 + 200 + 208 + 105 + 4) >> 3 = 821 >> 3 = 102, p1' = 409 >> 2 = 102, p2' = 821 >> 3 = 102
    # q0' = 829 >> 3 = 103, q1' = 417 >> 2 = 104, q2' = 845 >> 3 = 105
    np_, nq, notes = line([100, 101, 102, 103], [104, 105, 106, 107], 4, 0)
    assert (np_, nq) == ([102, 102, 102, 103], [103, 104, 105, 107])
    assert notes == {"filt", "strong_p", "strong_q"}


def test_strong_one_below_the_quarter_alpha_bound():
    # |p0 - q0| = 6 < (20 >> 2) + 2 = 7
    # p0' = 827 >> 3 = 103, p1' = 411 >> 2 = 102, p2' = 823 >> 3 = 102; q0' = 839 >> 3 = 104, q1' = 423 >> 2 = 105, q2' = 859 >> 3 = 107
    np_, nq, notes = line([100, 101, 102, 103], [106, 107, 108, 109], 4, 0)
    assert (np_, nq) == ([103, 102, 102, 103], [104, 105, 107, 109])
    assert notes == {"filt", "strong_p", "strong_q"}


def test_weak4_at_the_quarter_alpha_bound():
    # |p0 - q0| = 7: p0' = (202 + 100 + 108 + 2) >> 2 = 103, q0' = (216 + 107 + 101 + 2) >> 2 = 106
    np_, nq, notes = line([100, 101, 102, 103], [107, 108, 109, 110], 4, 0)
    assert (np_, nq) == ([103, 101, 102, 103], [106, 108, 109, 110])
    assert notes == {"filt", "weak4_p", "weak4_q"}


def test_strong_p_weak_q():
    # aq = 7 = beta: q0' = (210 + 104 + 101 + 2) >> 2 = 104
    np_, nq, notes = line([100, 101, 102, 103], [104, 105, 111, 111], 4, 0)
    assert (np_, nq) == ([102, 102, 102, 103], [104, 105, 111, 111])
    assert notes == {"filt", "strong_p", "weak4_q"}


def test_weak_p_strong_q():
    # the mirror image: q0' = (105 + 208 + 200 + 202 + 102 + 4) >> 3 = 102, q1' = 409 >> 2 = 102, q2' = 821 >> 3 = 102
    np_, nq, notes = line([104, 105, 111, 111], [100, 101, 102, 103], 4, 0)
    assert (np_, nq) == ([104, 105, 111, 111], [102, 102, 102, 103])
    assert notes == {"filt", "weak4_p", "strong_q"}


# ---------------- chroma ----------------
def test_chroma_weak():
    # tc = tc0 + 1 = 2; raw = 4 -> 2
    assert line([100, 102], [108, 106], 1, 1, chroma=True) == ([102, 102], [106, 106], {"filt", "delta_clipped"})
    # raw = (16 + (100 - 104) + 4) >> 3 = 2 = tc
    assert line([100, 100], [104, 104], 2, 1, chroma=True) == ([102, 100], [102, 104], {"filt"})


def test_chroma_bs4():
    # p0' = (204 + 100 + 106 + 2) >> 2 = 103, q0' = (212 + 108 + 102 + 2) >> 2 = 106
    assert line([100, 102], [108, 106], 4, 0, chroma=True) == ([103, 102], [106, 106], {"filt", "weak4_p", "weak4_q"})


# ---------------- the tables' corners ----------------
def test_table_corners():
    assert dr.thresholds(15, 0, 0, 8) == (15, 15, 0, 0)
    assert dr.thresholds(16, 0, 0, 8) == (16, 16, 4, 2)
    assert dr.thresholds(17, 0, 0, 8) == (17, 17, 4, 2)
    assert dr.thresholds(51, 0, 0, 8) == (51, 51, 255, 18)
    assert dr.thresholds(50, 6, -6, 8) == (51, 38, 255, 12)          # Clip3 at 51
    assert dr.thresholds(5, -6, 6, 8) == (0, 17, 0, 2)               # Clip3 at 0
    assert dr.thresholds(16, 0, 0, 10) == (16, 16, 16, 8)            # times 1 << (BitDepth - 8)
    assert dr.thresholds(28, 0, 0, 9) == (28, 28, 40, 14)
    assert [dr.tc0_of(16, b, 8) for b in (1, 2, 3, 4)] == [0, 0, 0, 0]
    assert [dr.tc0_of(17, b, 8) for b in (1, 2, 3)] == [0, 0, 1]
    assert [dr.tc0_of(21, b, 8) for b in (1, 2, 3)] == [0, 1, 1]
    assert [dr.tc0_of(23, b, 8) for b in (1, 2, 3)] == [1, 1, 1]
    assert [dr.tc0_of(28, b, 8) for b in (1, 2, 3)] == [1, 1, 2]
    assert [dr.tc0_of(51, b, 8) for b in (1, 2, 3, 4)] == [13, 17, 25, 0]
    assert [dr.tc0_of(51, b, 10) for b in (1, 2, 3)] == [52, 68, 100]
    assert [dr.chroma_qp(q, 0, 8) for q in (0, 29, 30, 34, 40, 51)] == [0, 29, 29, 32, 36, 39]
    assert dr.chroma_qp(51, 12, 8) == 39 and dr.chroma_qp(20, 12, 8) == 31
    assert dr.chroma_qp(2, -12, 8) == 0 and dr.chroma_qp(2, -12, 9) == -6 and dr.chroma_qp(2, -12, 10) == -10
    assert dr.thresholds(dr.chroma_qp(2, -12, 9), 6, 6, 9)[:2] == (6, 6)
    assert dr.thresholds(dr.chroma_qp(0, -12, 10), 0, 0, 10) == (0, 0, 0, 0)       # a negative QPc clamps to index 0


def intra_results(n, mb_type=10):
    res = np.zeros(n, jmhip.MB_RESULT_DTYPE)
    res["mb_type"] = mb_type
    return res


def test_whole_picture_by_hand():
    """Two Intra16x16 MBs, flat 100 | 104, QP 28: only the MB edge at x = 16 (bS 4, strong) moves samples.
    Luma: p2' = (200 + 300 + 304 + 4) >> 3 = 101, p1' = 406 >> 2 = 101, p0' = 816 >> 3 = 102, q0' = 824 >> 3 = 103,
    q1' = 414 >> 2 = 103, q2' = 832 >> 3 = 104; chroma (x = 8): p0' = 406 >> 2 = 101, q0' = 414 >> 2 = 103.
    Then the right MB's inner edge at x = 20 (bS 3, tc0 = 2) sees p2 p1 p0 = 103 104 104 (x = 17..19): delta = 0 and
    p1' = 104 + Clip3(-2, 2, (103 + 104 - 208) >> 1 = -1) = 103 at x = 18.  (The left MB's edge at x = 12 ran before
    the MB edge moved anything.)"""
    y = np.full((16, 32), 100, np.uint8)
    y[:, 16:] = 104
    u = np.full((8, 16), 100, np.uint8)
    u[:, 8:] = 104
    v = np.full((8, 16), 50, np.uint8)      # flat: stays as it is
    res = intra_results(2)
    (dy, du, dv), cnt = dr.deblock((y, u, v), res, 2, 1, 28)
    ey = y.copy()
    ey[:, 13:19] = [101, 101, 102, 103, 103, 103]
    eu = u.copy()
    eu[:, 7:9] = [101, 103]
    assert np.array_equal(dy, ey) and np.array_equal(du, eu) and np.array_equal(dv, v)
    assert cnt["L_edge_bS4"] == 4 and cnt["L_edge_bS3"] == 2 * (3 * 4 + 3 * 4) and cnt["L_strong_p"] == 16 and cnt["C_filt_bS4"] == 16
    for a, b in zip(jmhip.deblock_ref((y, u, v), res, 2, 1, 28), (ey, eu, v)):
        assert np.array_equal(a, b)
    # the same two macroblocks one above the other: the horizontal MB edge
    (ty, tu, tv), _ = dr.deblock((y.T.copy(), u.T.copy(), v.T.copy()), res, 1, 2, 28)
    assert np.array_equal(ty, ey.T) and np.array_equal(tu, eu.T)
    # inter, no coefficients, equal MVs: bS 0 everywhere, nothing moves; MVs 4 quarter samples apart: bS 1
    res = intra_results(2, mb_type=1)
    assert np.array_equal(dr.deblock((y, u, v), res, 2, 1, 28)[0][0], y)
    res["mv"][1, :, 0] = 4
    _, cnt = dr.deblock((y, u, v), res, 2, 1, 28)
    assert cnt["L_edge_bS1"] == 4 and cnt["L_filt_bS1"] == 16 and cnt["L_edge_bS0"] == 2 * 24
    res["mv"][1, :, 0] = 3
    assert dr.deblock((y, u, v), res, 2, 1, 28)[1]["L_edge_bS1"] == 0
    # MB 0's block 7 (row 1, column 3) coded: bS 2 on its four sides (left and top: odd edges, bottom: edge 2, right: the
    # MB edge), of which chroma has the bottom and the right one, per plane
    res["cbp_blk"][0] = 1 << 7
    cnt = dr.deblock((y, u, v), res, 2, 1, 28)[1]
    assert cnt["L_edge_bS2"] == 4 and cnt["C_edge_bS2"] == 2 * 2


# ---------------- reference == the host's C deblocker on the oracle's pictures ----------------
def same_planes(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            r, c = np.argwhere(g != w)[0]
            pytest.fail(f"{what}: plane {k} differs first at row {r}, column {c}: {g[r, c]} != {w[r, c]}")


def cpu_chain(case):
    """I, P, P through the CPU oracle, each P referencing the reference-deblocked previous picture."""
    o = oracle_lib.OracleEncoder(case.w, case.h, **case.kw)
    mbw, mbh = case.w // 16, case.h // 16
    records = []
    for i, pic in enumerate(case.pics()):
        res, rec = o.encode(*pic, jmhip.JMH_I_SLICE if i == 0 else jmhip.JMH_P_SLICE, case.qp, case.cqo)
        trace = {}
        dbk, cnt = dr.deblock(rec, res, mbw, mbh, case.qp, case.cqo, case.ab[0], case.ab[1], case.bd, trace=trace)
        host = jmhip.deblock_ref(rec, res, mbw, mbh, case.qp, case.cqo, case.ab[0], case.ab[1], case.bd)
        same_planes(host, dbk, f"{case.name} picture {i}: host C vs reference")
        records.append((rec, res, cnt, trace))
        o.set_reference(*dbk)
    o.close()
    return records


@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_reference_equals_host_c(case):
    records = cpu_chain(case)
    print(case.name, dict(sorted(sum((r[2] for r in records), dr.Counter()).items())))
    dc.check_case(case, records)


@pytest.mark.parametrize("qp", dc.SWEEP_QPS)
def test_threshold_sweep(qp):
    pics = dc.sweep_pics()
    mbw, mbh = dc.SWEEP_W // 16, dc.SWEEP_H // 16
    o = oracle_lib.OracleEncoder(dc.SWEEP_W, dc.SWEEP_H, search_range=8)
    for cqo in dc.SWEEP_CQO:
        ires, irec = o.encode(*pics[0], jmhip.JMH_I_SLICE, qp, cqo)
        for ab in dc.SWEEP_AB:
            cnt = dr.Counter()
            rec, res = irec, ires
            for i in range(2):
                if i:
                    o.set_reference(*dbk)
                    res, rec = o.encode(*pics[1], jmhip.JMH_P_SLICE, qp, cqo)
                dbk, c = dr.deblock(rec, res, mbw, mbh, qp, cqo, ab[0], ab[1])
                same_planes(jmhip.deblock_ref(rec, res, mbw, mbh, qp, cqo, ab[0], ab[1]), dbk, f"QP {qp} {ab} {cqo} picture {i}")
                cnt += c
            dc.check_sweep(qp, ab, cqo, cnt)
    o.close()


def test_host_entry_rejects_bad_arguments():
    y, u, v = np.zeros((16, 16), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8)
    res = intra_results(1)
    for bad in (dict(qp=52), dict(alpha_div2=7), dict(beta_div2=-7), dict(chroma_qp_offset=13), dict(bit_depth=11)):
        kw = dict(qp=30)
        kw.update(bad)
        with pytest.raises(jmhip.JmhError):
            jmhip.deblock_ref((y, u, v), res, 1, 1, **kw)
    with pytest.raises(jmhip.JmhError):
        jmhip.deblock_ref((y, u, v), intra_results(2), 1, 1, 30)
