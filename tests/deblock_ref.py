"""A plain reference of the H.264 deblocking filter, written from the standard's clause 8.7.

Test infrastructure only.  It shares nothing with the product's two deblockers (the host's C one
and the device's fused one) nor with the oracle: the tables below are typed from Tables 8-15, 8-16
and 8-17, and the walk over the picture is per line of samples in picture coordinates -- every
line asks "which two 4x4 blocks of which macroblocks do my p0 and q0 lie in" -- not per macroblock
tile with precomputed strengths.

Scope (what the encoder under test produces): frame macroblocks, 4:2:0, one reference picture, one
QP for the whole picture, disable_deblocking_filter_idc 0 (slice edges are filtered like any other
macroblock edge), BitDepthY == BitDepthC.

    deblock(rec_yuv, results, mbw, mbh, qp, ...) -> (y, u, v), counters

counters is a collections.Counter of what the filter did, luma ("L_...") and chroma ("C_...",
both planes together) apart:
    edge_bS0 .. edge_bS4      edge segments (4 luma / 2 chroma lines sharing one bS) by strength,
                              picture edges and the skipped inner edges of 8x8-transform MBs left out
    filt_bS1 .. filt_bS4      lines that passed the alpha / beta gate (filterSamplesFlag, 8-468)
    gated_bS1 .. gated_bS4    lines with bS > 0 that did not
    strong_p/q, weak4_p/q     (luma) the two bS 4 branches of 8.7.2.4, per side
    p1_mod, q1_mod            (luma) bS < 4 lines with ap < beta / aq < beta: p1 / q1 rewritten
    delta_clipped             bS < 4 lines whose delta was limited by tC
    clip1_hi, clip1_lo        bS < 4 lines where p0 + delta or q0 - delta left [0, max]
"""
from collections import Counter

import numpy as np

# Table 8-16: alpha' and beta' by indexA / indexB (0..51)
ALPHA_T = ([0] * 16 +
           [4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90,
            101, 113, 127, 144, 162, 182, 203, 226, 255, 255])
BETA_T = ([0] * 16 +
          [2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13,
           14, 14, 15, 15, 16, 16, 17, 17, 18, 18])
# Table 8-17: tC0' by indexA, one row per bS 1, 2, 3
TC0_T = {
    1: [0] * 23 + [1] * 10 + [2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6, 6, 7, 8, 9, 10, 11, 13],
    2: [0] * 21 + [1] * 10 + [2, 2, 2, 2, 3, 3, 3, 4, 4, 5, 5, 6, 7, 8, 8, 10, 11, 12, 13, 15, 17],
    3: [0] * 17 + [1] * 10 + [2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 23, 25],
}
# Table 8-15: QPc by qPI; below 30 QPc = qPI
QPC_FROM_30 = [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]
assert len(ALPHA_T) == len(BETA_T) == 52 and all(len(r) == 52 for r in TC0_T.values()) and len(QPC_FROM_30) == 22

INTRA_TYPES = (9, 10, 13)          # jmh_mb_result.mb_type: Intra4x4, Intra16x16, Intra8x8


def clip3(lo, hi, v):
    return lo if v < lo else hi if v > hi else v


def chroma_qp(qp, chroma_qp_offset, bit_depth):
    """QPc (8.4.2.2.8 / Table 8-15) of qPI = Clip3(-QpBdOffsetC, 51, QPY + chroma_qp_index_offset)."""
    qpi = clip3(-6 * (bit_depth - 8), 51, qp + chroma_qp_offset)
    return qpi if qpi < 30 else QPC_FROM_30[qpi - 30]


def thresholds(qp_av, alpha_div2, beta_div2, bit_depth):
    """8.7.2.2: (indexA, indexB, alpha, beta) for the average QP of the two blocks (8-461 .. 8-467)."""
    index_a = clip3(0, 51, qp_av + 2 * alpha_div2)
    index_b = clip3(0, 51, qp_av + 2 * beta_div2)
    scale = 1 << (bit_depth - 8)
    return index_a, index_b, ALPHA_T[index_a] * scale, BETA_T[index_b] * scale


def tc0_of(index_a, bS, bit_depth):
    """8-469 / 8-470: tC0 = tC0' * (1 << (BitDepth - 8)); bS 4 has none."""
    return TC0_T[bS][index_a] * (1 << (bit_depth - 8)) if bS < 4 else 0


def filter_samples(p, q, bS, alpha, beta, tc0, chroma, maxv):
    """One line across an edge: p = [p0, p1, (p2, p3)], q = [q0, q1, (q2, q3)].
    Returns (p', q', notes): the filtered samples (new lists) and what happened, a list of strings
    from 'gated', 'filt', 'strong_p', 'weak4_p', 'strong_q', 'weak4_q', 'p1_mod', 'q1_mod',
    'delta_clipped', 'clip1_hi', 'clip1_lo'."""
    p0, p1, q0, q1 = p[0], p[1], q[0], q[1]
    np_, nq = list(p), list(q)
    # filterSamplesFlag (8-468)
    if not (bS != 0 and abs(p0 - q0) < alpha and abs(p1 - p0) < beta and abs(q1 - q0) < beta):
        return np_, nq, ["gated"]
    notes = ["filt"]
    if bS < 4:                                       # 8.7.2.3
        if chroma:
            tc = tc0 + 1
        else:
            ap, aq = abs(p[2] - p0), abs(q[2] - q0)
            tc = tc0 + (1 if ap < beta else 0) + (1 if aq < beta else 0)
        raw = (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3
        delta = clip3(-tc, tc, raw)
        if delta != raw:
            notes.append("delta_clipped")
        for val in (p0 + delta, q0 - delta):
            if val > maxv:
                notes.append("clip1_hi")
            elif val < 0:
                notes.append("clip1_lo")
        np_[0] = clip3(0, maxv, p0 + delta)
        nq[0] = clip3(0, maxv, q0 - delta)
        if not chroma:
            mid = (p0 + q0 + 1) >> 1
            if ap < beta:
                np_[1] = p1 + clip3(-tc0, tc0, (p[2] + mid - (p1 << 1)) >> 1)
                notes.append("p1_mod")
            if aq < beta:
                nq[1] = q1 + clip3(-tc0, tc0, (q[2] + mid - (q1 << 1)) >> 1)
                notes.append("q1_mod")
        return np_, nq, notes
    # bS 4: 8.7.2.4
    close = abs(p0 - q0) < ((alpha >> 2) + 2)
    if not chroma and abs(p[2] - p0) < beta and close:
        p2, p3 = p[2], p[3]
        np_[0] = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3
        np_[1] = (p2 + p1 + p0 + q0 + 2) >> 2
        np_[2] = (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3
        notes.append("strong_p")
    else:
        np_[0] = (2 * p1 + p0 + q1 + 2) >> 2
        notes.append("weak4_p")
    if not chroma and abs(q[2] - q0) < beta and close:
        q2, q3 = q[2], q[3]
        nq[0] = (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3
        nq[1] = (p0 + q0 + q1 + q2 + 2) >> 2
        nq[2] = (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3
        notes.append("strong_q")
    else:
        nq[0] = (2 * q1 + q0 + p1 + 2) >> 2
        notes.append("weak4_q")
    return np_, nq, notes


class _Blocks:
    """What 8.7.2.1 asks about the 4x4 luma block that covers luma sample (x, y)."""

    def __init__(self, results, mbw):
        self.mbw = mbw
        self.intra = [int(t) in INTRA_TYPES for t in results["mb_type"]]
        self.cbp_blk = [int(c) for c in results["cbp_blk"]]
        self.mv = results["mv"].astype(np.int64).tolist()
        self.ref = results["ref_idx"].astype(np.int64).tolist()
        self.t8 = [bool(t) for t in results["transform_8x8"]]

    def mb(self, x, y):
        return (y >> 4) * self.mbw + (x >> 4)

    def strength(self, px, py, qx, qy):
        """bS of the line whose p0 is luma sample (px, py) and whose q0 is (qx, qy)."""
        mp, mq = self.mb(px, py), self.mb(qx, qy)
        if self.intra[mp] or self.intra[mq]:
            return 4 if mp != mq else 3          # frame pictures: every MB edge gets 4
        bp = ((py & 15) >> 2) * 4 + ((px & 15) >> 2)
        bq = ((qy & 15) >> 2) * 4 + ((qx & 15) >> 2)
        if (self.cbp_blk[mp] >> bp) & 1 or (self.cbp_blk[mq] >> bq) & 1:
            return 2
        rp = self.ref[mp][((py & 15) >> 3) * 2 + ((px & 15) >> 3)]
        rq = self.ref[mq][((qy & 15) >> 3) * 2 + ((qx & 15) >> 3)]
        if rp != rq:
            return 1
        vp, vq = self.mv[mp][bp], self.mv[mq][bq]
        if abs(vp[0] - vq[0]) >= 4 or abs(vp[1] - vq[1]) >= 4:     # quarter samples, frame MBs
            return 1
        return 0


def deblock(rec_yuv, results, mbw, mbh, qp, chroma_qp_offset=0, alpha_div2=0, beta_div2=0, bit_depth=8, trace=None):
    """Deblock the reconstruction rec_yuv = (y, u, v) of a picture of mbw x mbh macroblocks whose
    results (MB_RESULT_DTYPE[mbw * mbh]; mb_type, cbp_blk, mv, ref_idx and transform_8x8 are read)
    are given.  Returns ((y, u, v), counters); the inputs are left alone.

    trace: an optional dict; every sample within reach of a line that passed the gate (p0..p2 and
    q0..q2 in luma, p0 and q0 in chroma) is entered as trace[(plane, row, column)] =
    (bS, [notes of filter_samples], 'p' or 'q', k of p_k / q_k) (plane 0, 1, 2; last line wins), and
    trace["lines"] lists those lines as (plane, vertical edge?, luma coordinate of the edge, luma
    coordinate along it, bS)."""
    blocks = _Blocks(results, mbw)
    planes = [np.asarray(p).astype(np.int64).tolist() for p in rec_yuv]
    assert len(planes[0]) == 16 * mbh and len(planes[0][0]) == 16 * mbw
    assert len(planes[1]) == 8 * mbh and len(planes[1][0]) == 8 * mbw
    maxv = (1 << bit_depth) - 1
    counters = Counter()
    qpc = chroma_qp(qp, chroma_qp_offset, bit_depth)
    # one QP for the picture: qPav = (qPp + qPq + 1) >> 1 is that QP (luma) / its QPc (chroma)
    thr = [thresholds(qp, alpha_div2, beta_div2, bit_depth)] + [thresholds(qpc, alpha_div2, beta_div2, bit_depth)] * 2

    for mby in range(mbh):
        for mbx in range(mbw):                       # 8.7: macroblocks in raster order
            t8 = blocks.t8[mby * mbw + mbx]
            for pl in range(3):                      # the planes do not read each other
                chroma = pl > 0
                sub = 2 if chroma else 1
                tag = "C_" if chroma else "L_"
                plane = planes[pl]
                index_a, _, alpha, beta = thr[pl]
                for vertical in (True, False):       # vertical edges left to right, then horizontal
                    for k in range(4):
                        if chroma and k & 1:
                            continue                 # 4:2:0 chroma: the edges 8 luma samples apart
                        if not chroma and t8 and k & 1:
                            continue                 # transform_size_8x8_flag: no 4x4 luma edges
                        edge = 16 * (mbx if vertical else mby) + 4 * k      # luma coordinate across
                        if edge == 0:
                            continue                 # picture edge
                        along0 = 16 * (mby if vertical else mbx)
                        for n in range(0, 16, sub):  # luma coordinate along the edge
                            along = along0 + n
                            if vertical:
                                bS = blocks.strength(edge - 1, along, edge, along)
                            else:
                                bS = blocks.strength(along, edge - 1, along, edge)
                            if n % 4 == 0:
                                counters[tag + "edge_bS%d" % bS] += 1
                            if bS == 0:
                                continue
                            e, a, taps = edge // sub, along // sub, 2 if chroma else 4
                            if vertical:
                                p = [plane[a][e - 1 - i] for i in range(taps)]
                                q = [plane[a][e + i] for i in range(taps)]
                            else:
                                p = [plane[e - 1 - i][a] for i in range(taps)]
                                q = [plane[e + i][a] for i in range(taps)]
                            np_, nq, notes = filter_samples(p, q, bS, alpha, beta, tc0_of(index_a, bS, bit_depth), chroma, maxv)
                            if notes[0] == "gated":
                                counters[tag + "gated_bS%d" % bS] += 1
                                continue
                            counters[tag + "filt_bS%d" % bS] += 1
                            for note in notes[1:]:
                                counters[tag + note] += 1
                            if trace is not None:
                                trace.setdefault("lines", []).append((pl, vertical, edge, along, bS))
                            for i in range(taps):
                                for side, off, new in (("p", -1 - i, np_[i]), ("q", i, nq[i])):
                                    r, c = (a, e + off) if vertical else (e + off, a)
                                    plane[r][c] = new
                                    if trace is not None and i < (1 if chroma else 3):   # the filter's reach
                                        trace[(pl, r, c)] = (bS, notes, side, i)
    dt = np.uint16 if bit_depth > 8 else np.uint8
    return tuple(np.array(p, dt) for p in planes), counters
