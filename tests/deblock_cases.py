"""The deblocking tests' shared cases: content, filter parameters and what each case must contain
(test_deblock_ref.py on the CPU, test_deblock_gpu.py on the device).  Test infrastructure only.

A case is three pictures (I, P, P) of its size; `need` names the counters of deblock_ref.deblock
that must be non-zero over the chain -- what the case is there for.

What the reference counted on the CPU oracle's chains (filtered lines by bS 1/2/3/4):
    moving_qp28        luma 163/144/1350/391 (gated 161/164/1626/441), chroma 161/66/476/461; bS 4 strong p/q 313/311,
                       weak 78/80; p1/q1 rewritten 1534/1516; delta clipped 82 + 85
    moving_qp36_off6   luma 162/33/2289/797, chroma 162/22/902/919; strong 700/719, weak 97/78; delta clipped 6 + 13
    moving_qp44        luma 112/0/3933/1220, chroma 100/0/1348/1212 (no bS 2 in this content)
    moving_qp20_offm2  luma 122 filtered, 8614 gated; chroma 445 / 3683
    blocks_qp30        chroma Clip1 at the top 4, at 0 once
    blocks_qp51        chroma Clip1 11 / 19; delta clipped 2331 + 621; bS 4 weak p/q 729/564, strong 302/467
    near_white         luma Clip1 at 255 on 6 lines;  near_black: luma Clip1 at 0 on 2 lines
    t8_epzs            luma 32/57/1646/599, chroma 48/50/635/561
    high10_epzs        luma 841/32/1530/467, chroma 730/15/561/565
    high9_negqpc_qp2   nothing filtered (12864 lines gated);  high9_negqpc_qp4: luma 116 filtered, chroma none
    one_mb             24 bS 3 segments, no bS 4;  one_column / one_row: 12 bS 4 segments in the I picture"""
import numpy as np

from test_gpu_parity import moving_seq

BS = (1, 2, 3, 4)
FILT = ["%s_filt_bS%d" % (t, b) for t in "LC" for b in BS]
GATED = ["%s_gated_bS%d" % (t, b) for t in "LC" for b in BS]
BRANCHES = ["L_strong_p", "L_strong_q", "L_weak4_p", "L_weak4_q", "L_p1_mod", "L_q1_mod", "L_delta_clipped"]


def block_seq(w, h, n, seed):
    """4x4 blocks of 0 / 255 with +-3 noise, chroma = luma / its inverse: Clip1 at both ends."""
    rng = np.random.default_rng(seed)
    big = np.kron(rng.integers(0, 2, ((h + 32) // 4, (w + 32) // 4)) * 255, np.ones((4, 4), np.int64))
    pics = []
    for i in range(n):
        y = big[4 * i:4 * i + h, 8 * i:8 * i + w]
        y = np.clip(y + rng.integers(-3, 4, y.shape), 0, 255).astype(np.uint8)
        pics.append((np.ascontiguousarray(y), np.ascontiguousarray(y[::2, ::2]), np.ascontiguousarray(255 - y[1::2, 1::2])))
    return pics


def near_white_seq(w, h, n, seed, invert=False):
    """255 minus sparse 2x2 dips of 0..39, +-2 noise (invert: the near-black mirror image)."""
    rng = np.random.default_rng(seed)
    bh, bw = (h + 32) // 2, (w + 32) // 2
    dips = np.where(rng.random((bh, bw)) < 0.25, rng.integers(0, 40, (bh, bw)), 0)
    big = np.kron(dips, np.ones((2, 2), np.int64))
    pics = []
    for i in range(n):
        y = 255 - big[2 * i:2 * i + h, 4 * i:4 * i + w]
        y = np.clip(y + rng.integers(-2, 3, y.shape), 0, 255)
        if invert:
            y = 255 - y
        y = y.astype(np.uint8)
        pics.append((np.ascontiguousarray(y), np.ascontiguousarray(y[::2, ::2]), np.ascontiguousarray(y[1::2, 1::2])))
    return pics


def widen(pics, bd):
    """8-bit pictures at bit depth bd: v << (bd - 8) with the low bits set."""
    sh = bd - 8
    return [tuple(np.ascontiguousarray((p.astype(np.uint16) << sh) + ((1 << sh) - 1)) for p in pic) for pic in pics]


class Case:
    def __init__(self, name, pics, qp, ab, need, cqo=0, bd=8, w=96, h=64, kw=None, check=None):
        self.name, self.make, self.qp, self.ab, self.need, self.cqo, self.bd, self.w, self.h = name, pics, qp, ab, need, cqo, bd, w, h
        self.kw = dict(search_range=8, **(kw or {}))     # what the case itself needs of the encoder
        self.check = check                               # further assertions on (case, pictures' records)

    def pics(self):
        return self.make(self.w, self.h)

    def __repr__(self):
        return self.name


def _mov(step, seed):
    return lambda w, h: moving_seq(w, h, 3, seed, step)


CASES = [
    Case("moving_qp28", _mov((5, -3), 1), 28, (0, 0), FILT + GATED + BRANCHES),
    Case("moving_qp36_off6", _mov((5, -3), 2), 36, (6, 6), FILT + GATED + BRANCHES),
    Case("moving_qp44", _mov((3, 2), 3), 44, (0, 0), ["L_filt_bS1", "L_filt_bS3", "L_filt_bS4", "C_filt_bS1", "C_filt_bS3", "C_filt_bS4"]),
    Case("moving_qp20_offm2", _mov((3, 2), 4), 20, (-2, -2), ["L_filt", "L_gated"], check="mostly_gated"),
    Case("blocks_qp30", lambda w, h: block_seq(w, h, 3, 5), 30, (3, 3), ["C_clip1_hi", "C_clip1_lo"]),
    Case("blocks_qp51", lambda w, h: block_seq(w, h, 3, 6), 51, (6, 6), ["C_clip1_hi", "C_clip1_lo"], check="qp51"),
    Case("near_white", lambda w, h: near_white_seq(w, h, 3, 7), 40, (6, 6), ["L_clip1_hi"]),
    Case("near_black", lambda w, h: near_white_seq(w, h, 3, 7, invert=True), 40, (6, 6), ["L_clip1_lo"]),
    Case("t8_epzs", _mov((5, -3), 8), 34, (0, 0), FILT, kw=dict(transform_8x8_mode=1, search_mode=3), check="t8"),
    Case("high10_epzs", lambda w, h: widen(moving_seq(w, h, 3, 9, (5, -3)), 10), 32, (0, 0), FILT, bd=10,
         kw=dict(bit_depth=10, search_mode=3), check="above255"),
    # 9 bits, chroma_qp_index_offset -12: qPI = Clip3(-6, 51, QP - 12) = -6 = QPc, chroma indexA = Clip3(0, 51, -6 + 12) = 6:
    # alpha' = 0, no chroma line can pass.  At QP 2 luma indexA = 2 + 12 = 14 has alpha' = 0 as well (Table 8-16 starts at
    # 16), so luma lines pass only from QP 4 on: the second case carries "luma filtered, chroma not"
    Case("high9_negqpc_qp2", lambda w, h: widen(moving_seq(w, h, 3, 10, (5, -3)), 9), 2, (6, 6), ["L_gated", "C_gated"], cqo=-12, bd=9,
         kw=dict(bit_depth=9, search_mode=3), check="none_filtered"),
    Case("high9_negqpc_qp4", lambda w, h: widen(moving_seq(w, h, 3, 10, (5, -3)), 9), 4, (6, 6), ["L_filt", "C_gated"], cqo=-12, bd=9,
         kw=dict(bit_depth=9, search_mode=3), check="no_chroma_filtered"),
    Case("one_mb", _mov((1, 1), 11), 36, (2, 2), ["L_edge_bS3", "L_filt_bS3"], w=16, h=16, check="one_mb"),
    Case("one_column", _mov((1, 1), 12), 36, (2, 2), ["L_edge_bS4", "L_filt"], w=16, h=64, check="one_column"),
    Case("one_row", _mov((1, 1), 13), 36, (2, 2), ["L_edge_bS4", "L_filt"], w=64, h=16, check="one_row"),
]


def total(counters, prefix):
    """Sum of the counters whose name starts with prefix ('L_filt' covers L_filt_bS1..4)."""
    return sum(v for k, v in counters.items() if k.startswith(prefix))


def check_need(case, counters):
    for name in case.need:
        assert total(counters, name) > 0, f"{case.name}: the chain never reaches {name}: {dict(counters)}"


def check_case(case, records):
    """records: per picture (rec, results, counters, trace).  The case's own assertions."""
    allc = sum((r[2] for r in records), type(records[0][2])())
    check_need(case, allc)
    k = case.check
    mbw, mbh = case.w // 16, case.h // 16
    if k == "mostly_gated":
        assert total(allc, "L_gated") > total(allc, "L_filt") and total(allc, "C_gated") > total(allc, "C_filt"), dict(allc)
    elif k == "qp51":
        assert allc["L_delta_clipped"] + allc["C_delta_clipped"] >= 2000, dict(allc)
        assert allc["L_weak4_p"] > allc["L_strong_p"] and allc["L_weak4_q"] > allc["L_strong_q"], dict(allc)
    elif k == "t8":
        n_inter_t8 = 0
        for rec, res, cnt, trace in records:
            for a in np.flatnonzero(res["transform_8x8"] == 1):
                n_inter_t8 += int(res["mb_type"][a]) not in (9, 10, 13)
            t8 = set(np.flatnonzero(res["transform_8x8"] == 1).tolist())
            for pl, vertical, edge, along, bS in trace.get("lines", []):      # no odd (4x4) luma edge of such an MB is filtered
                x, y = (edge, along) if vertical else (along, edge)
                assert not (pl == 0 and edge % 8 == 4 and (y // 16) * mbw + x // 16 in t8), (vertical, edge, along)
        assert n_inter_t8 > 0, "no inter macroblock with the 8x8 transform"
    elif k == "above255":
        for side in "pq":
            assert any(t[2] == side and t[3] == 0 and rec[pl][r, c] > 255
                       for rec, res, cnt, trace in records for key, t in trace.items() if key != "lines" for pl, r, c in [key]), side
    elif k == "none_filtered":
        assert total(allc, "L_filt") == 0 and total(allc, "C_filt") == 0, dict(allc)
    elif k == "no_chroma_filtered":
        assert total(allc, "C_filt") == 0, dict(allc)
    elif k == "one_mb":
        assert allc["L_edge_bS4"] == 0 and allc["C_edge_bS4"] == 0, dict(allc)
    elif k in ("one_column", "one_row"):
        # only the (mb - 1) MB edges across the long direction exist; the I picture is all intra: 4 segments each
        i_cnt = records[0][2]
        assert i_cnt["L_edge_bS4"] == 4 * (max(mbw, mbh) - 1), dict(i_cnt)


SWEEP_QPS = (0, 15, 16, 17, 28, 36, 45, 51)
SWEEP_AB = ((-6, -6), (0, 0), (6, 6), (-6, 6), (6, -6), (3, -2))
SWEEP_CQO = (-12, 0, 12)
SWEEP_W, SWEEP_H = 64, 48


def sweep_pics():
    return moving_seq(SWEEP_W, SWEEP_H, 2, 14, (3, -2))


def check_sweep(qp, ab, cqo, counters):
    """Table 8-16: alpha' = 0 below index 16, so nothing passes at QP <= 15 with offsets <= 0 (chroma:
    QPc <= QP when chroma_qp_index_offset <= 0 as well)."""
    if qp <= 15 and ab[0] <= 0 and ab[1] <= 0:
        assert total(counters, "L_filt") == 0, (qp, ab, cqo, dict(counters))
        if cqo <= 0:
            assert total(counters, "C_filt") == 0, (qp, ab, cqo, dict(counters))
    if qp == 16 and ab == (0, 0):
        assert total(counters, "L_filt") > 0, (qp, ab, cqo, dict(counters))
