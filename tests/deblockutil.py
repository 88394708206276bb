"""The deblocking filter of 8.7 written once more, in numpy on int64, straight from 8.7.2.1 - 8.7.2.4: the yardstick of tests/test_deblock_edges.py
(the edge functions of k_deblock and k_deblock_x alone on the device) and tests/test_deblock_ranges.py (whole pictures of the generator).

Independent of streamgen/sg_recon.c, oracle/h264o_recon.c and the kernels: its own copies of Tables 8-16 and 8-17, every line of an edge filtered
at once (no per-line branches: both filters are computed and selected), and a class word per line that says which branches of the rule the line took."""
import numpy as np

# Table 8-16: alpha' and beta' by indexA / indexB
ALPHA = np.array([0] * 16 + [4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182,
                             203, 226, 255, 255], dtype=np.int64)
BETA = np.array([0] * 16 + [2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18],
                dtype=np.int64)
# Table 8-17: tC0' [indexA][bS - 1]
TC0 = np.array([[0, 0, 0]] * 17 + [[0, 0, 1]] * 4 + [[0, 1, 1]] * 2 + [[1, 1, 1]] * 4 + [[1, 1, 2]] * 4 + [[1, 2, 3]] * 2 + [
    [2, 2, 3], [2, 2, 4], [2, 3, 4], [2, 3, 4], [3, 3, 5], [3, 4, 6], [3, 4, 6], [4, 5, 7], [4, 5, 8], [4, 6, 9], [5, 7, 10], [6, 8, 11], [6, 8, 13],
    [7, 10, 14], [8, 11, 16], [9, 12, 18], [10, 13, 20], [11, 15, 23], [13, 17, 25]], dtype=np.int64)
assert ALPHA.shape == (52,) and BETA.shape == (52,) and TC0.shape == (52, 3)

# ---- the class word of a line (filter_lines) ----
C_FILTERED = 1 << 0
C_REJ_SHIFT, C_REJ_MASK = 1, 7       # why a line was left alone: REJ_*
REJ_NONE, REJ_BS0, REJ_ALPHA, REJ_BETA_P, REJ_BETA_Q = 0, 1, 2, 3, 4   # the first test of 8.7.2.2 that failed, in the order |p0 - q0|, |p1 - p0|, |q1 - q0|
C_AP, C_AQ = 1 << 4, 1 << 5          # luma lines that are filtered: |p2 - p0| < beta, |q2 - q0| < beta
# bS < 4, filtered lines.  "Hit" means the clip changed the value: the unclipped value lay outside the range.
C_DELTA_SHIFT = 6                    # delta: 0 inside, 1 clipped at -tc, 2 clipped at +tc
C_P1_SHIFT, C_Q1_SHIFT = 8, 10       # the p1 / q1 correction (luma, ap / aq): 0 inside (or none), 1 clipped at -tC0, 2 clipped at +tC0
C_P0_SHIFT, C_Q0_SHIFT = 12, 14      # p0 + delta / q0 - delta: 0 inside, 1 clipped at 0, 2 clipped at 255
C_TC0_ZERO = 1 << 19                 # tC0 == 0
# bS 4, filtered lines
C_SMALL = 1 << 16                    # |p0 - q0| < (alpha >> 2) + 2
C_STRONG_P, C_STRONG_Q = 1 << 17, 1 << 18  # the side took the strong filter (luma: ap / aq and C_SMALL); else the weak one


def field(cls, shift, mask=3):
    return (cls >> shift) & mask


def describe(c):
    """a class word as text"""
    c = int(c)
    rej = ("", "bS 0", "|p0-q0| >= alpha", "|p1-p0| >= beta", "|q1-q0| >= beta")[field(c, C_REJ_SHIFT, C_REJ_MASK)]
    if not c & C_FILTERED:
        return "not filtered (%s)" % rej
    t = ["filtered", "ap" if c & C_AP else "!ap", "aq" if c & C_AQ else "!aq"]
    t.append("delta " + ("inside", "at -tc", "at +tc")[field(c, C_DELTA_SHIFT)])
    t.append("p1 corr " + ("inside", "at -tC0", "at +tC0")[field(c, C_P1_SHIFT)])
    t.append("q1 corr " + ("inside", "at -tC0", "at +tC0")[field(c, C_Q1_SHIFT)])
    t.append("p0' " + ("inside", "at 0", "at 255")[field(c, C_P0_SHIFT)])
    t.append("q0' " + ("inside", "at 0", "at 255")[field(c, C_Q0_SHIFT)])
    if c & C_TC0_ZERO:
        t.append("tC0 0")
    if c & C_SMALL:
        t.append("small")
    t.append("strong p" if c & C_STRONG_P else "-")
    t.append("strong q" if c & C_STRONG_Q else "-")
    return ", ".join(t)


def _i64(a, n):
    a = np.asarray(a).astype(np.int64)
    return np.broadcast_to(a, (n,)) if a.ndim == 0 else a


def filter_lines(samples, bs, alpha, beta, tc0, chroma):
    """8.7.2.2 - 8.7.2.4 on n lines across one edge.  samples: (n, 8) p3 p2 p1 p0 q0 q1 q2 q3 (luma) or (n, 4) p1 p0 q0 q1 (chroma); bs, alpha, beta,
    tc0: per line (tc0 is tC0' of Table 8-17; ignored where bS is 4).  Returns (filtered lines as uint8, class word per line as int64)."""
    s = np.asarray(samples).astype(np.int64)
    n = s.shape[0]
    assert s.shape == (n, 4 if chroma else 8) and s.min(initial=0) >= 0 and s.max(initial=0) <= 255
    bs, alpha, beta, tc0 = _i64(bs, n), _i64(alpha, n), _i64(beta, n), _i64(tc0, n)
    assert bs.shape == alpha.shape == beta.shape == tc0.shape == (n,) and bs.min(initial=0) >= 0 and bs.max(initial=0) <= 4
    if chroma:
        p1, p0, q0, q1 = s.T
        p2 = q2 = p3 = q3 = None
    else:
        p3, p2, p1, p0, q0, q1, q2, q3 = s.T
    # 8.7.2.2: filterSamplesFlag
    t_a, t_p, t_q = np.abs(p0 - q0) < alpha, np.abs(p1 - p0) < beta, np.abs(q1 - q0) < beta
    filt = (bs > 0) & t_a & t_p & t_q
    rej = np.where(bs == 0, REJ_BS0, np.where(~t_a, REJ_ALPHA, np.where(~t_p, REJ_BETA_P, np.where(~t_q, REJ_BETA_Q, REJ_NONE))))
    cls = filt.astype(np.int64) * C_FILTERED | rej.astype(np.int64) << C_REJ_SHIFT
    if chroma:
        ap = aq = np.zeros(n, dtype=bool)
    else:
        ap, aq = np.abs(p2 - p0) < beta, np.abs(q2 - q0) < beta
    normal, strong = filt & (bs < 4), filt & (bs == 4)
    cls |= np.where(filt & ap, C_AP, 0) | np.where(filt & aq, C_AQ, 0)
    # 8.7.2.3: bS < 4
    tc = tc0 + 1 if chroma else tc0 + ap + aq
    raw = (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3
    delta = np.clip(raw, -tc, tc)
    n_p0, n_q0 = np.clip(p0 + delta, 0, 255), np.clip(q0 - delta, 0, 255)
    cls |= np.where(normal, np.where(raw < -tc, 1, np.where(raw > tc, 2, 0)), 0) << C_DELTA_SHIFT
    cls |= np.where(normal, np.where(p0 + delta < 0, 1, np.where(p0 + delta > 255, 2, 0)), 0) << C_P0_SHIFT
    cls |= np.where(normal, np.where(q0 - delta < 0, 1, np.where(q0 - delta > 255, 2, 0)), 0) << C_Q0_SHIFT
    cls |= np.where(normal & (tc0 == 0), C_TC0_ZERO, 0)
    out = s.copy()
    P0, Q0 = (1, 2) if chroma else (3, 4)
    out[:, P0], out[:, Q0] = np.where(normal, n_p0, p0), np.where(normal, n_q0, q0)
    if not chroma:
        avg = (p0 + q0 + 1) >> 1
        raw_p, raw_q = (p2 + avg - (p1 << 1)) >> 1, (q2 + avg - (q1 << 1)) >> 1
        out[:, 2] = np.where(normal & ap, p1 + np.clip(raw_p, -tc0, tc0), p1)
        out[:, 5] = np.where(normal & aq, q1 + np.clip(raw_q, -tc0, tc0), q1)
        cls |= np.where(normal & ap, np.where(raw_p < -tc0, 1, np.where(raw_p > tc0, 2, 0)), 0) << C_P1_SHIFT
        cls |= np.where(normal & aq, np.where(raw_q < -tc0, 1, np.where(raw_q > tc0, 2, 0)), 0) << C_Q1_SHIFT
    # 8.7.2.4: bS 4
    small = np.abs(p0 - q0) < (alpha >> 2) + 2
    cls |= np.where(strong & small, C_SMALL, 0)
    weak_p, weak_q = (2 * p1 + p0 + q1 + 2) >> 2, (2 * q1 + q0 + p1 + 2) >> 2
    if chroma:
        out[:, P0], out[:, Q0] = np.where(strong, weak_p, out[:, P0]), np.where(strong, weak_q, out[:, Q0])
    else:
        sp, sq = strong & ap & small, strong & aq & small
        cls |= np.where(sp, C_STRONG_P, 0) | np.where(sq, C_STRONG_Q, 0)
        out[:, 3] = np.where(sp, (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, np.where(strong, weak_p, out[:, 3]))
        out[:, 2] = np.where(sp, (p2 + p1 + p0 + q0 + 2) >> 2, out[:, 2])
        out[:, 1] = np.where(sp, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3, p2)
        out[:, 4] = np.where(sq, (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3, np.where(strong, weak_q, out[:, 4]))
        out[:, 5] = np.where(sq, (p0 + q0 + q1 + q2 + 2) >> 2, out[:, 5])
        out[:, 6] = np.where(sq, (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3, q2)
    assert out.min(initial=0) >= 0 and out.max(initial=0) <= 255
    return out.astype(np.uint8), cls


# ---- 8.7.2.1: boundary strengths ----
def _block_grids(mbs):
    """per 4x4 block of the picture [4 * rows, 4 * columns]: intra, coefficients, the pictures of the two lists (-1: list unused) and their vectors"""
    hmb, wmb = mbs.shape
    up = lambda a: np.repeat(np.repeat(a, 4, axis=0), 4, axis=1)
    bit = np.arange(16).reshape(4, 4)                                   # block 4 * row + column of a macroblock
    nz = (mbs["nzmask"].astype(np.int64)[:, :, None, None] >> bit) & 1
    nz = nz.transpose(0, 2, 1, 3).reshape(4 * hmb, 4 * wmb)
    quad = (np.arange(4)[:, None] // 2) * 2 + np.arange(4)[None, :] // 2  # the 8x8 quadrant of a block
    ref = [mbs[k].astype(np.int64)[:, :, quad].transpose(0, 2, 1, 3).reshape(4 * hmb, 4 * wmb) for k in ("refid", "refid1")]
    mv = [mbs[k].astype(np.int64).reshape(hmb, wmb, 4, 4, 2).transpose(0, 2, 1, 3, 4).reshape(4 * hmb, 4 * wmb, 2) for k in ("mv", "mv1")]
    return up(mbs["intra"] != 0), nz != 0, ref, mv


def strengths(mbs, field, how=None):
    """bS of the left edge (first result) and of the top edge (second) of every 4x4 block of a picture, [4 * rows, 4 * columns]; 0 along the picture's
    left / top border.  Frame and field pictures without MBAFF.  how (optional dict) receives, for the same two grids, flags of how two-vector blocks were
    decided: 1 bS 1 although the pictures pair crossed, 2 ... straight, 4 bS 0 through the crossed pairing."""
    intra, nz, ref, mv = _block_grids(mbs)
    out = []
    for axis in (1, 0):  # vertical edges: the neighbour is the block to the left; horizontal: the block above
        def pq(a):
            a = np.moveaxis(a, axis, 0)
            return a[:-1], a[1:]
        ip, iq = pq(intra)
        zp, zq = pq(nz)
        (ap, aq), (bp, bq) = pq(ref[0]), pq(ref[1])
        (vap, vaq), (vbp, vbq) = pq(mv[0]), pq(mv[1])
        vlimit = 2 if field else 4

        def close(u, v):
            return (np.abs(u[..., 0] - v[..., 0]) < 4) & (np.abs(u[..., 1] - v[..., 1]) < vlimit)
        n_p, n_q = (ap >= 0).astype(int) + (bp >= 0), (aq >= 0).astype(int) + (bq >= 0)
        # one vector each: the same picture (whichever list it came through) and vectors close
        pic_p, pic_q = np.where(ap >= 0, ap, bp), np.where(aq >= 0, aq, bq)
        v_p, v_q = np.where((ap >= 0)[..., None], vap, vbp), np.where((aq >= 0)[..., None], vaq, vbq)
        one = ~((pic_p == pic_q) & close(v_p, v_q))
        # two vectors each: the same two pictures, and a pairing of the vectors by picture that is close
        straight, crossed = (ap == aq) & (bp == bq), (ap == bq) & (bp == aq)
        s_ok, c_ok = straight & close(vap, vaq) & close(vbp, vbq), crossed & close(vap, vbq) & close(vbp, vaq)
        two = ~(s_ok | c_ok)
        motion = np.where(n_p != n_q, 1, np.where(n_p == 1, one, np.where(n_p == 2, two, 0))).astype(np.int64)
        pos = np.arange(1, intra.shape[axis])
        mb_edge = (pos % 4 == 0).reshape((-1,) + (1,) * (ip.ndim - 1))
        strong = 3 if (field and axis == 0) else 4       # horizontal macroblock edges of field pictures: 3
        bs = np.where(ip | iq, np.where(mb_edge, strong, 3), np.where(zp | zq, 2, motion))
        flags = np.where(~(ip | iq | zp | zq) & (n_p == 2) & (n_q == 2),
                         (two & crossed) * 1 + (two & straight) * 2 + (~s_ok & c_ok) * 4, 0)
        full, fl = np.zeros(np.moveaxis(intra, axis, 0).shape, dtype=np.int64), np.zeros(np.moveaxis(intra, axis, 0).shape, dtype=np.int64)
        full[1:], fl[1:] = bs, flags
        out.append((np.moveaxis(full, 0, axis), np.moveaxis(fl, 0, axis)))
    if how is not None:
        how["v"], how["h"] = out[0][1], out[1][1]
    return out[0][0], out[1][0]


COUNTERS = ("db_filt_luma_bs1", "db_filt_luma_bs2", "db_filt_luma_bs3", "db_filt_luma_bs4", "db_rej_luma_bs1", "db_rej_luma_bs2", "db_rej_luma_bs3", "db_rej_luma_bs4",
            "db_filt_chroma_bs1", "db_filt_chroma_bs2", "db_filt_chroma_bs3", "db_filt_chroma_bs4", "db_rej_chroma_bs1", "db_rej_chroma_bs2", "db_rej_chroma_bs3",
            "db_rej_chroma_bs4", "db_rej_alpha", "db_rej_beta_p", "db_rej_beta_q", "db_ap0_aq0", "db_ap0_aq1", "db_ap1_aq0", "db_ap1_aq1", "db_delta_lo", "db_delta_hi",
            "db_delta_in", "db_p1_lo", "db_p1_hi", "db_q1_lo", "db_q1_hi", "db_p0_at0", "db_p0_at255", "db_q0_at0", "db_q0_at255", "db_tc0_zero", "db_tc0_zero_ap",
            "db_bs4_small", "db_bs4_not_small", "db_bs4_strong_p0_q0", "db_bs4_strong_p0_q1", "db_bs4_strong_p1_q0", "db_bs4_strong_p1_q1", "db_index_a_min",
            "db_index_a_max", "db_index_b_min", "db_index_b_max", "db_index_a_clip0", "db_index_a_clip51", "db_qp_odd", "db_pcm_edge", "db_cbcr_alpha",
            "db_pair_differs", "db_cbcr_pair_differs", "db_seg_none", "db_field_bs3", "db_b_bs1_crossed", "db_b_bs1_straight", "db_b_bs0_crossed", "db_slice_offsets",
            "db_idc1_modified", "db_idc2_skipped")


def new_counters():
    c = dict.fromkeys(COUNTERS, 0)
    c["db_index_a_min"] = c["db_index_b_min"] = 1 << 20
    c["db_index_a_max"] = c["db_index_b_max"] = -(1 << 20)
    return c


def _count_lines(c, cls, bs, chroma):
    """the class words of the lines of one plane of an edge into the counters (the generator's SG_R_DB_* definitions, from the class words)"""
    pl = "chroma" if chroma else "luma"
    f = (cls & C_FILTERED) != 0
    for b in (1, 2, 3, 4):
        c["db_filt_%s_bs%d" % (pl, b)] += int((f & (bs == b)).sum())
        c["db_rej_%s_bs%d" % (pl, b)] += int((~f & (bs == b)).sum())
    rej = field(cls, C_REJ_SHIFT, C_REJ_MASK)
    for name, r in (("db_rej_alpha", REJ_ALPHA), ("db_rej_beta_p", REJ_BETA_P), ("db_rej_beta_q", REJ_BETA_Q)):
        c[name] += int((rej == r).sum())
    normal, strong = f & (bs < 4), f & (bs == 4)
    d = field(cls, C_DELTA_SHIFT)
    c["db_delta_lo"] += int((normal & (d == 1)).sum())
    c["db_delta_hi"] += int((normal & (d == 2)).sum())
    c["db_delta_in"] += int((normal & (d == 0)).sum())
    for name, sh in (("p0", C_P0_SHIFT), ("q0", C_Q0_SHIFT)):
        c["db_%s_at0" % name] += int((normal & (field(cls, sh) == 1)).sum())
        c["db_%s_at255" % name] += int((normal & (field(cls, sh) == 2)).sum())
    if chroma:
        return
    ap, aq = (cls & C_AP) != 0, (cls & C_AQ) != 0
    for a in (0, 1):
        for q in (0, 1):
            c["db_ap%d_aq%d" % (a, q)] += int((normal & (ap == a) & (aq == q)).sum())
            c["db_bs4_strong_p%d_q%d" % (a, q)] += int((strong & (((cls & C_STRONG_P) != 0) == a) & (((cls & C_STRONG_Q) != 0) == q)).sum())
    for name, sh in (("p1", C_P1_SHIFT), ("q1", C_Q1_SHIFT)):
        c["db_%s_lo" % name] += int((normal & (field(cls, sh) == 1)).sum())
        c["db_%s_hi" % name] += int((normal & (field(cls, sh) == 2)).sum())
    z = (cls & C_TC0_ZERO) != 0
    c["db_tc0_zero"] += int(z.sum())
    c["db_tc0_zero_ap"] += int((z & ap).sum())
    c["db_bs4_small"] += int((strong & ((cls & C_SMALL) != 0)).sum())
    c["db_bs4_not_small"] += int((strong & ((cls & C_SMALL) == 0)).sum())


def deblock_picture(planes, mbs, field_pic, mono, counters=None):
    """8.7 on one picture: planes = (Y, Cb, Cr) before the filter, mbs = the macroblock table [rows, columns] (streamgen.DBMB), field_pic = the picture
    is a field, mono = no chroma.  Macroblocks in raster order; in each the vertical edges left to right, then the horizontal edges top to bottom,
    luma then Cb and Cr per edge.  Returns the filtered planes; counters (new_counters()) receives what the lines did."""
    Y, Cb, Cr = (np.array(p, dtype=np.uint8) for p in planes)
    hmb, wmb = mbs.shape
    how = {}
    bs_v, bs_h = strengths(mbs, field_pic, how)
    c = counters
    qp = np.where(mbs["pcm"] != 0, 0, mbs["qp"]).astype(np.int64)          # I_PCM: QP_Y 0
    qpc = mbs["qpc"].astype(np.int64)
    for my in range(hmb):
        for mx in range(wmb):
            cur = mbs[my, mx]
            idc = int(cur["dbf_idc"])
            if idc == 1:
                continue
            off_a, off_b = int(cur["alpha_off"]), int(cur["beta_off"])
            for vertical in (True, False):
                ny, nx = (my, mx - 1) if vertical else (my - 1, mx)
                have = nx >= 0 and ny >= 0
                if have and idc == 2 and mbs[ny, nx]["slice_id"] != cur["slice_id"]:
                    have = False
                    if c is not None:
                        c["db_idc2_skipped"] += 1
                for e in range(4):
                    if (e == 0 and not have) or (cur["t8x8"] and e in (1, 3)):
                        continue
                    py, px = (ny, nx) if e == 0 else (my, mx)           # the macroblock of the p samples
                    grid, hw = (bs_v, how["v"]) if vertical else (bs_h, how["h"])
                    seg = grid[4 * my:4 * my + 4, 4 * mx + e] if vertical else grid[4 * my + e, 4 * mx:4 * mx + 4]
                    if c is not None:
                        fl = hw[4 * my:4 * my + 4, 4 * mx + e] if vertical else hw[4 * my + e, 4 * mx:4 * mx + 4]
                        c["db_b_bs1_crossed"] += int(((fl & 1) != 0).sum())
                        c["db_b_bs1_straight"] += int(((fl & 2) != 0).sum())
                        c["db_b_bs0_crossed"] += int(((fl & 4) != 0).sum())
                        if field_pic and e == 0 and not vertical:
                            c["db_field_bs3"] += int((seg == 3).sum())
                    if not seg.any():
                        continue
                    did, alphas, any_f, p_changed = {}, {}, False, False
                    for plane in ((0,) if (mono or e & 1) else (0, 1, 2)):
                        P = (Y, Cb, Cr)[plane]
                        size, half = (16, 4) if plane == 0 else (8, 2)
                        pos = e * (4 if plane == 0 else 2)
                        y0, x0 = my * size, mx * size
                        view = P[y0:y0 + size, x0 + pos - half:x0 + pos + half] if vertical else P[y0 + pos - half:y0 + pos + half, x0:x0 + size].T
                        bs = np.repeat(seg, size // 4)
                        qa = (qp[py, px] + qp[my, mx] + 1) >> 1 if plane == 0 else (qpc[py, px, plane - 1] + qpc[my, mx, plane - 1] + 1) >> 1
                        ia, ib = min(max(qa + off_a, 0), 51), min(max(qa + off_b, 0), 51)
                        tc0 = np.where(bs < 4, TC0[ia][np.clip(bs - 1, 0, 2)], 0)
                        before = view.copy()
                        out, cls = filter_lines(before, bs, ALPHA[ia], BETA[ib], tc0, plane != 0)
                        if vertical:
                            P[y0:y0 + size, x0 + pos - half:x0 + pos + half] = out
                        else:
                            P[y0 + pos - half:y0 + pos + half, x0:x0 + size] = out.T
                        if c is not None:
                            f = (cls & C_FILTERED) != 0
                            did[plane], alphas[plane] = f, int(ALPHA[ia])
                            any_f, p_changed = any_f or bool(f.any()), p_changed or bool((out[:, :half] != before[:, :half]).any())
                            _count_lines(c, cls[bs > 0], bs[bs > 0], plane != 0)
                            c["db_index_a_min"], c["db_index_a_max"] = min(c["db_index_a_min"], ia), max(c["db_index_a_max"], ia)
                            c["db_index_b_min"], c["db_index_b_max"] = min(c["db_index_b_min"], ib), max(c["db_index_b_max"], ib)
                            c["db_index_a_clip0"] += qa + off_a < 0
                            c["db_index_a_clip51"] += qa + off_a > 51
                            c["db_seg_none"] += int(((seg > 0) & ~f.reshape(4, -1).any(axis=1)).sum())
                            if plane == 0:
                                c["db_pair_differs"] += int((f[0::2] != f[1::2]).sum())
                    if c is not None:
                        c["db_qp_odd"] += int(qp[py, px] != qp[my, mx] and (qp[py, px] + qp[my, mx]) % 2 == 1)
                        c["db_pcm_edge"] += int(bool(mbs[py, px]["pcm"]) or bool(cur["pcm"]))
                        if 2 in did:
                            c["db_cbcr_alpha"] += alphas[1] != alphas[2]
                            c["db_cbcr_pair_differs"] += int((did[1] != did[2]).sum())
                        if e == 0:
                            other = mbs[py, px]
                            c["db_slice_offsets"] += int(any_f and other["slice_id"] != cur["slice_id"] and
                                                         (other["alpha_off"] != cur["alpha_off"] or other["beta_off"] != cur["beta_off"]))
                            c["db_idc1_modified"] += int(p_changed and other["dbf_idc"] == 1)
    return Y, Cb, Cr


# ---- recipes of tests/test_deblock_ranges.py ----
# name -> (generator parameters, counters of streamgen.last_ranges() that must be above 0).  The conditions are not measurements: the seeds were chosen
# on the CPU until the generator alone met them, and the CPU test asserts them.
_P = dict(idr_period=0, frames=5)
_LUMA_NORMAL = ["db_filt_luma_bs1", "db_filt_luma_bs2", "db_filt_luma_bs3", "db_rej_luma_bs1", "db_rej_luma_bs2", "db_rej_luma_bs3", "db_ap0_aq0", "db_ap0_aq1", "db_ap1_aq0",
                "db_ap1_aq1", "db_delta_lo", "db_delta_hi", "db_delta_in", "db_p1_lo", "db_p1_hi", "db_q1_lo", "db_q1_hi", "db_rej_alpha", "db_rej_beta_p", "db_rej_beta_q",
                "db_pair_differs", "db_seg_none"]
_BS4 = ["db_filt_luma_bs4", "db_rej_luma_bs4", "db_filt_chroma_bs4", "db_bs4_small", "db_bs4_not_small", "db_bs4_strong_p0_q0", "db_bs4_strong_p0_q1", "db_bs4_strong_p1_q0",
        "db_bs4_strong_p1_q1"]
_CHROMA = ["db_filt_chroma_bs1", "db_filt_chroma_bs2", "db_filt_chroma_bs3", "db_rej_chroma_bs1", "db_rej_chroma_bs2", "db_rej_chroma_bs3", "db_rej_chroma_bs4"]
CONTENT = {
    # intra content at a high QP, smooth enough for the strong filter and noisy enough for the weak one: the strong filter on both sides, on one side only, on neither
    "smooth_intra_cavlc": (dict(width=64, height=48, frames=4, idr_period=1, profile_idc=66, cabac=0, qp=34, noise=16, seed=1), _BS4),
    # noisy content at a middle QP: clipped deltas and corrections, every (ap, aq), every test that rejects
    "noisy_cabac": (dict(_P, width=80, height=64, profile_idc=77, cabac=1, qp=30, noise=40, intra_in_p_permille=100, sub8x8_permille=300, seed=1), _LUMA_NORMAL + _CHROMA),
    # the whole QP range in one picture, I_PCM beside coded macroblocks
    "qp_range_pcm_cavlc": (dict(_P, width=96, height=80, profile_idc=66, cabac=0, qp=30, qp_jitter=25, pcm_permille=80, intra_in_p_permille=150, seed=2),
                           ["db_qp_odd", "db_pcm_edge", "db_filt_luma_bs4", "db_filt_luma_bs2"]),
    # offsets of -12 at QPs around 20: indexA clipped at 0 on some edges, 16 .. 20 (tC0 0) on others, which still filter
    "offsets_minus6_cabac": (dict(_P, width=80, height=64, profile_idc=77, cabac=1, qp=22, qp_jitter=12, pcm_permille=40, intra_in_p_permille=200, alpha_off_div2=-6,
                                  beta_off_div2=-6, noise=4, seed=1), ["db_index_a_clip0", "db_tc0_zero", "db_tc0_zero_ap", "db_filt_luma_bs3"]),
    # offsets of +12 at QPs around 45: indexA clipped at 51
    "offsets_plus6_cavlc": (dict(_P, width=80, height=64, profile_idc=66, cabac=0, qp=45, qp_jitter=6, intra_in_p_permille=100, alpha_off_div2=6, beta_off_div2=6, noise=30,
                                 seed=1), ["db_index_a_clip51", "db_filt_luma_bs1", "db_filt_luma_bs4"]),
    # 0 / 255 content under offsets of +12: p0 + delta and q0 - delta leave 0 .. 255
    "contrast_plus6_cabac": (dict(_P, width=64, height=48, frames=4, profile_idc=77, cabac=1, contrast=1, qp=40, motion_x4=5, motion_y4=-3, alpha_off_div2=6, beta_off_div2=6,
                                  seed=1), ["db_p0_at0", "db_p0_at255", "db_q0_at0", "db_q0_at255"]),
    # chroma_qp_index_offset -12 with a second offset of -11 (High): Cb and Cr under different alpha, one filtered and one not
    "cqp_minus12_high_8x8": (dict(_P, width=80, height=64, profile_idc=100, cabac=1, transform8x8=1, chroma_qp_offset=-12, qp=34, noise=25, intra_in_p_permille=150, seed=1),
                             ["db_cbcr_alpha", "db_cbcr_pair_differs", "db_filt_chroma_bs2"]),
    "cqp_plus12_cavlc": (dict(_P, width=64, height=48, profile_idc=77, cabac=0, chroma_qp_offset=12, qp=28, noise=25, intra_in_p_permille=150, seed=26), _CHROMA),
    # three slices, each with its own disable_deblocking_filter_idc and offsets
    "slices3_per_slice_cabac": (dict(_P, width=80, height=80, frames=7, profile_idc=77, cabac=1, slices=3, dbf_per_slice=1, qp=32, noise=20, intra_in_p_permille=150, seed=2),
                                ["db_slice_offsets", "db_idc1_modified", "db_idc2_skipped"]),
    "slices3_per_slice_cavlc_8x8": (dict(_P, width=64, height=80, frames=6, profile_idc=100, cabac=0, transform8x8=1, slices=3, dbf_per_slice=1, qp=30, qp_jitter=5, noise=20,
                                         seed=3), ["db_slice_offsets", "db_idc1_modified", "db_idc2_skipped"]),
    # B pictures: two vectors on both sides of an edge, paired straight and crossed; P pictures with one picture at two indices
    "b_spatial_cabac": (dict(_P, width=96, height=64, frames=7, profile_idc=77, cabac=1, bframes=2, num_ref_frames=3, weighted_pred=1, wp_range=2, bskip_permille=100,
                             sub8x8_permille=300, qp=34, noise=4, seed=3), ["db_b_bs1_crossed", "db_b_bs1_straight", "db_b_bs0_crossed", "ref_twice"]),
    "b_temporal_cavlc": (dict(_P, width=96, height=64, frames=7, profile_idc=77, cabac=0, bframes=2, num_ref_frames=3, direct_temporal=1, weighted_pred=1, wp_range=2,
                              bskip_permille=200, sub8x8_permille=300, qp=34, noise=4, seed=1), ["db_b_bs1_straight", "db_filt_luma_bs1"]),
    # field pictures: bS 3 on horizontal macroblock edges, the vertical vector limit of 2
    "field_p_cavlc": (dict(_P, width=96, height=64, frames=4, profile_idc=77, cabac=0, field_pics=1, num_ref_frames=2, intra_in_p_permille=200, sub8x8_permille=300, seed=1),
                      ["db_field_bs3", "db_filt_luma_bs4", "db_filt_luma_bs1"]),
    "field_b_cavlc": (dict(_P, width=96, height=64, frames=5, profile_idc=77, cabac=0, field_pics=2, bframes=1, num_ref_frames=2, intra_in_p_permille=150, seed=1),
                      ["db_field_bs3", "db_filt_luma_bs1"]),
    "mono_cabac": (dict(_P, width=64, height=48, frames=4, profile_idc=100, cabac=1, mono=1, transform8x8=1, intra_in_p_permille=150, noise=20, seed=1),
                   ["db_filt_luma_bs2", "db_filt_luma_bs4"]),
}
# what k_deblock distinguishes: groups of 8 macroblock rows, a window of four macroblock columns, loads of four macroblocks
_G = dict(idr_period=0, frames=4, intra_in_p_permille=120, sub8x8_permille=300, noise=20)
GEOMETRY = {
    "geo_16x16": (dict(_G, width=16, height=16, profile_idc=77, cabac=1, seed=1), ["db_filt_luma_bs2"]),
    "geo_16x272": (dict(_G, width=16, height=272, profile_idc=66, cabac=0, seed=1), ["db_filt_luma_bs4"]),
    "geo_80x144": (dict(_G, width=80, height=144, profile_idc=77, cabac=1, slices=2, seed=1), ["db_filt_luma_bs4"]),
    "geo_80x272": (dict(_G, width=80, height=272, profile_idc=100, cabac=0, transform8x8=1, bframes=1, num_ref_frames=2, seed=1), ["db_filt_luma_bs4"]),
    "geo_272x16": (dict(_G, width=272, height=16, profile_idc=77, cabac=1, pcm_permille=40, seed=1), ["db_filt_luma_bs4"]),
    "geo_1040x32": (dict(_G, width=1040, height=32, profile_idc=77, cabac=0, qp_jitter=5, seed=1), ["db_filt_luma_bs4"]),
}
RECIPE_TABLE = dict(CONTENT, **GEOMETRY)
RECIPES = {k: v[0] for k, v in RECIPE_TABLE.items()}


def pictures_of(kw):
    return kw["frames"] * (2 if kw.get("field_pics") else 1)


def unmet(name, r):
    """The conditions of recipe `name` that the counters r = streamgen.last_ranges() do not meet (an empty list: all met)."""
    kw, need = RECIPE_TABLE[name]
    bad = [k for k in need if r[k] <= 0]
    if name == "qp_range_pcm_cavlc" and not (r["db_index_a_min"] <= 10 and r["db_index_a_max"] >= 48):
        bad.append("indexA from 10 or below to 48 or above")
    if name == "offsets_minus6_cabac" and not (r["db_index_a_min"] == 0 and r["db_index_b_min"] == 0):
        bad.append("indexA and indexB down to 0")
    if name == "offsets_plus6_cavlc" and not (r["db_index_a_max"] == 51 and r["db_index_b_max"] == 51):
        bad.append("indexA and indexB up to 51")
    return bad


def required_somewhere():
    """every deblocking counter must be asked for by at least one recipe (the four minima / maxima through the conditions of unmet())"""
    asked = {k for _, need in RECIPE_TABLE.values() for k in need} | {"db_index_a_min", "db_index_a_max", "db_index_b_min", "db_index_b_max"}
    return [k for k in COUNTERS if k not in asked]
