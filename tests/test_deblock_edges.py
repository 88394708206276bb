"""The edge functions of the two K5 kernel families alone on the device, against 8.7.2.2 - 8.7.2.4 in numpy (deblockutil.filter_lines).

k_deblock filters two lines per lane in packed 16-bit halves (k_deblock_pk.h: pk_luma_edge / pk_chroma_edge), k_deblock_x one line per lane
(k_deblock_edge.h: filter_edge).  The hook h264mi_internal_deblock_edge_probe runs those very functions on 2^18 lines of samples per kind -- luma or
chroma, macroblock edge or inner edge, either family -- and every byte must equal the yardstick's.  There is no tolerance in this file.

The lines are drawn with a fixed seed around the thresholds of the rule; the CPU test asserts from the yardstick's class words alone that every
branch of the rule, and every way the two halves of a lane or the lanes of a wavefront can disagree, is taken by at least 256 lines (lanes,
wavefronts) -- conditions on the inputs, which hold before any kernel has run."""
import functools

import numpy as np
import pytest

import deblockutil as D

N = 1 << 18               # lines per kind
WAVE_LINES = 128          # the packed layout: 64 lanes of two lines
NEED = 256
INDICES = np.array([0, 15, 16, 17, 20, 28, 36, 44, 51])
INDEX_P = np.array([.04, .04, .10, .10, .14, .14, .14, .15, .15])
KINDS = [(c, m) for c in (0, 1) for m in (1, 0)]
# wavefront modes: what the lanes of a wavefront may draw
M_MIX, M_NO4, M_ONLY4, M_ALPHA0, M_BS0, M_ONE = range(6)


@functools.lru_cache(maxsize=None)
def case(chroma, mb_edge):
    """(samples, bs, alpha, beta, tc0, expected, class words, index_a) of one kind: drawn once, filtered once by the yardstick, read-only"""
    rng = np.random.default_rng(8700 + 2 * chroma + mb_edge)
    n, nl, nw = N, N // 2, N // WAVE_LINES
    mode = np.full(nw, M_MIX)
    k = nw // 16   # sixteenths: 6 mixed, 2 without bS 4, 2 of bS 4 alone (both mixed on inner edges), 3 with alpha 0, 1 with bS 0, 2 with one live lane
    mode[6 * k:8 * k], mode[8 * k:10 * k] = (M_NO4, M_ONLY4) if mb_edge else (M_MIX, M_MIX)
    mode[10 * k:13 * k], mode[13 * k:14 * k], mode[14 * k:] = M_ALPHA0, M_BS0, M_ONE
    lmode = np.repeat(mode, 64)                                            # per lane
    # bS per lane; indexA / indexB per lane (luma) or per line (chroma: the Cb and the Cr half of a lane, equal in half of the lanes)
    bs_l = rng.integers(0, 5 if mb_edge else 4, nl)
    bs_l = np.where(lmode == M_NO4, rng.integers(0, 4, nl), bs_l)
    bs_l = np.where(lmode == M_ONLY4, 4, bs_l)
    bs_l = np.where(np.isin(lmode, (M_ALPHA0, M_ONE)), rng.integers(1, 5 if mb_edge else 4, nl), bs_l)
    bs_l = np.where(lmode == M_BS0, 0, bs_l)
    ia_l, ib_l = rng.choice(INDICES, nl, p=INDEX_P), rng.choice(INDICES, nl, p=INDEX_P)
    # the corners the issue names: alpha 255 / beta 18 / tC0 25 (indices 51, 51, bS 3) and alpha 4 / beta 2 (indices 16, 16)
    corner = rng.random(nl)
    ia_l, ib_l = np.where(corner < .06, np.where(corner < .03, 51, 16), ia_l), np.where(corner < .06, np.where(corner < .03, 51, 16), ib_l)
    bs_l = np.where((corner < .03) & (lmode == M_MIX) & (bs_l > 0), 3, bs_l)
    ia_l = np.where(np.isin(lmode, (M_ALPHA0, M_ONE)), rng.choice([0, 15], nl), ia_l)
    # a wavefront with one live lane: everything else has alpha 0
    live = np.zeros(nl, dtype=bool)
    one = np.flatnonzero(mode == M_ONE)
    live[one * 64 + rng.integers(0, 64, one.size)] = True
    ia_l, ib_l = np.where(live, 36, ia_l), np.where(live, 36, ib_l)
    bs, ia, ib = np.repeat(bs_l, 2), np.repeat(ia_l, 2), np.repeat(ib_l, 2)
    if chroma:
        other = (rng.random(nl) < .5) & (lmode < M_ALPHA0)
        ia[1::2] = np.where(other, rng.choice(INDICES, nl, p=INDEX_P), ia[1::2])
        ib[1::2] = np.where(other, rng.choice(INDICES, nl, p=INDEX_P), ib[1::2])
    alpha, beta = D.ALPHA[ia], D.BETA[ib]
    tc0 = np.where((bs > 0) & (bs < 4), D.TC0[ia, np.clip(bs - 1, 0, 2)], 0)
    # samples around the thresholds
    p0 = np.where(rng.random(n) < .3, rng.choice([0, 1, 254, 255], n), rng.integers(0, 256, n))
    gap = np.stack([alpha - 1, alpha, (alpha >> 2) + 1, (alpha >> 2) + 2, rng.integers(0, 4, n)])[rng.choice(5, n, p=[.2, .15, .15, .15, .35]), np.arange(n)]
    gap = np.maximum(gap, 0)
    sign = np.where(rng.random(n) < .5, 1, -1)
    sign = np.where((p0 + sign * gap < 0) | (p0 + sign * gap > 255), -sign, sign)   # the other way where the range ends
    q0 = np.clip(p0 + sign * gap, 0, 255)

    def near(x):  # within +-(beta + 1) of x, with exact hits on beta - 1 and beta
        how = rng.random(n)
        off = np.where(how < .25, beta - 1, np.where(how < .4, beta, rng.integers(0, 1 << 30, n) % (beta + 2)))
        sg = np.where(rng.random(n) < .5, 1, -1)
        sg = np.where((x + sg * off < 0) | (x + sg * off > 255), -sg, sg)
        return np.clip(x + sg * off, 0, 255)
    # the ends of the sample range: p0 and q0 both at (or one beside) 0 or 255 and one of p1 / q1 there too, so that delta points out of the range
    ends = rng.random(n) < .1
    e = np.where(rng.random(n) < .5, 0, 255)
    p0, q0 = np.where(ends, np.abs(e - rng.integers(0, 2, n)), p0), np.where(ends, np.abs(e - rng.integers(0, 2, n)), q0)
    p1, q1 = near(p0), near(q0)
    pin = rng.random(n) < .5
    p1, q1 = np.where(ends & pin, e, p1), np.where(ends & ~pin, e, q1)
    if chroma:
        s = np.stack([p1, p0, q0, q1], axis=1)
    else:
        from_p1 = rng.random(n) < .3   # p2 / q2 beside p1 / q1 in some lines, around the ap / aq threshold of p0 / q0 in the others
        p2, q2 = np.where(from_p1, near(p1), near(p0)), np.where(from_p1, near(q1), near(q0))
        s = np.stack([near(p2), p2, p1, p0, q0, q1, q2, near(q2)], axis=1)
    flat = np.repeat(live, 2)
    s = np.where(flat[:, None], s[:, :1], s)   # the live lane of an otherwise dead wavefront: flat lines, filtered whatever the strength
    s = s.astype(np.uint8)
    out, cls = D.filter_lines(s, bs, alpha, beta, tc0, bool(chroma))
    arrays = [np.ascontiguousarray(a) for a in (s, bs.astype(np.uint8), alpha.astype(np.uint8), beta.astype(np.uint8), tc0.astype(np.uint8), out, cls, ia)]
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


def coverage(chroma, mb_edge):
    """name -> count of lines / lanes / wavefronts, from the class words and the parameters alone"""
    s, bs, alpha, beta, tc0, out, cls, ia = case(chroma, mb_edge)
    bs, alpha, beta, tc0 = (a.astype(np.int64) for a in (bs, alpha, beta, tc0))
    f = (cls & D.C_FILTERED) != 0
    normal, strong = f & (bs < 4), f & (bs == 4)
    c = {}
    c["filtered"], c["bs0"] = f.sum(), (D.field(cls, D.C_REJ_SHIFT, 7) == D.REJ_BS0).sum()
    for name, r in (("rej_alpha", D.REJ_ALPHA), ("rej_beta_p", D.REJ_BETA_P), ("rej_beta_q", D.REJ_BETA_Q)):
        c[name] = (D.field(cls, D.C_REJ_SHIFT, 7) == r).sum()
    for b in (1, 2, 3) + ((4,) if mb_edge else ()):
        c["filtered_bs%d" % b], c["rejected_bs%d" % b] = (f & (bs == b)).sum(), (~f & (bs == b)).sum()
    for k, name in enumerate(("inside", "lo", "hi")):
        c["delta_" + name] = (normal & (D.field(cls, D.C_DELTA_SHIFT) == k)).sum()
        c["p0_" + ("inside", "at0", "at255")[k]] = (normal & (D.field(cls, D.C_P0_SHIFT) == k)).sum()
        c["q0_" + ("inside", "at0", "at255")[k]] = (normal & (D.field(cls, D.C_Q0_SHIFT) == k)).sum()
    c["tc0_zero_filtered"] = ((cls & D.C_TC0_ZERO) != 0).sum()
    c["alpha0"] = ((alpha == 0) & (bs > 0)).sum()
    c["alpha255_beta18_tc25"] = (f & (alpha == 255) & (beta == 18) & (tc0 == 25)).sum()
    c["alpha4_beta2"] = (f & (alpha == 4) & (beta == 2)).sum()
    ap, aq = (cls & D.C_AP) != 0, (cls & D.C_AQ) != 0
    if not chroma:
        for a in (0, 1):
            for q in (0, 1):
                c["normal_ap%d_aq%d" % (a, q)] = (normal & (ap == a) & (aq == q)).sum()
        c["tc0_zero_ap"] = (((cls & D.C_TC0_ZERO) != 0) & ap).sum()
        for k, name in enumerate(("inside", "lo", "hi")):
            c["p1_" + name], c["q1_" + name] = (normal & ap & (D.field(cls, D.C_P1_SHIFT) == k)).sum(), (normal & aq & (D.field(cls, D.C_Q1_SHIFT) == k)).sum()
    if mb_edge:
        small = (cls & D.C_SMALL) != 0
        c["bs4_small"], c["bs4_not_small"] = (strong & small).sum(), (strong & ~small).sum()
        if not chroma:
            sp, sq = (cls & D.C_STRONG_P) != 0, (cls & D.C_STRONG_Q) != 0
            for a in (0, 1):
                for q in (0, 1):
                    c["bs4_strong_p%d_q%d" % (a, q)] = (strong & (sp == a) & (sq == q)).sum()
                    c["bs4_ap%d_aq%d" % (a, q)] = (strong & (ap == a) & (aq == q)).sum()
            c["bs4_ap_not_small"] = (strong & ap & aq & ~small).sum()
    # the packed layout: lane k of the launch holds lines 2k and 2k + 1
    e, o = slice(0, None, 2), slice(1, None, 2)
    c["lane_filtered_differs"] = (f[e] != f[o]).sum()
    both_n = normal[e] & normal[o]
    de, do_ = D.field(cls, D.C_DELTA_SHIFT)[e], D.field(cls, D.C_DELTA_SHIFT)[o]
    c["lane_delta_sign_differs"] = (both_n & (de != 0) & (do_ != 0) & (de != do_)).sum()
    if chroma:
        c["lane_alpha_differs"], c["lane_tc_differs"] = (f[e] & f[o] & (alpha[e] != alpha[o])).sum(), (both_n & (tc0[e] != tc0[o])).sum()
        c["lane_beta_differs"] = (f[e] & f[o] & (beta[e] != beta[o])).sum()
    else:
        both = f[e] & f[o]
        c["lane_ap_differs"], c["lane_aq_differs"] = (both & (ap[e] != ap[o])).sum(), (both & (aq[e] != aq[o])).sum()
        if mb_edge:
            c["lane_small_differs"] = (strong[e] & strong[o] & (((cls[e] ^ cls[o]) & D.C_SMALL) != 0)).sum()
            c["lane_strong_p_differs"] = (strong[e] & strong[o] & (((cls[e] ^ cls[o]) & D.C_STRONG_P) != 0)).sum()
    lane_f = (f[e] | f[o]).reshape(-1, 64)
    c["wave_none_filtered"], c["wave_one_lane_filtered"] = (lane_f.sum(1) == 0).sum(), (lane_f.sum(1) == 1).sum()
    c["wave_none_filtered_bs_on"] = ((lane_f.sum(1) == 0) & (bs[e].reshape(-1, 64) > 0).all(1)).sum()
    if mb_edge:
        b = bs[e].reshape(-1, 64)
        has0, has13, has4 = (b == 0).any(1), ((b > 0) & (b < 4)).any(1), (b == 4).any(1)
        c["wave_bs_0_13_4"], c["wave_no_bs4"], c["wave_only_bs4"] = (has0 & has13 & has4).sum(), (~has4 & has13).sum(), (b == 4).all(1).sum()
        f4 = (strong[e] | strong[o]).reshape(-1, 64).any(1)
        c["wave_filters_without_strong"] = (lane_f.any(1) & ~f4).sum()
    return {k: int(v) for k, v in c.items()}


@pytest.mark.parametrize("chroma,mb_edge", KINDS)
def test_lines_reach_every_branch(chroma, mb_edge):
    c = coverage(chroma, mb_edge)
    print("%s, %s edge:" % ("chroma" if chroma else "luma", "macroblock" if mb_edge else "inner"), c)
    short = {k: v for k, v in c.items() if v < NEED}
    assert not short, sorted(short.items())
    s, bs = case(chroma, mb_edge)[:2]
    assert s.shape == (N, 4 if chroma else 8) and (mb_edge or bs.max() < 4)


def test_class_words_on_lines_worked_by_hand():
    """a handful of lines filtered by hand from 8.7.2.3 / 8.7.2.4, so that the yardstick itself is pinned"""
    # luma, bS 1, alpha 20, beta 6, tC0 1: ap and aq, tc 3; delta = clip((4 * 8 + (50 - 60) + 4) >> 3 = 3) = 3
    out, cls = D.filter_lines([[50, 50, 50, 52, 60, 60, 60, 60]], [1], [20], [6], [1], False)
    assert out.tolist() == [[50, 50, 51, 55, 57, 59, 60, 60]] and cls[0] & D.C_AP and cls[0] & D.C_AQ and D.field(cls[0], D.C_DELTA_SHIFT) == 0
    assert D.field(cls[0], D.C_P1_SHIFT) == 2 and D.field(cls[0], D.C_Q1_SHIFT) == 1
    # the same line at bS 4: |p0 - q0| = 8 >= (20 >> 2) + 2, both sides weak
    out, cls = D.filter_lines([[50, 50, 50, 52, 60, 60, 60, 60]], [4], [20], [6], [0], False)
    assert out.tolist() == [[50, 50, 50, 53, 58, 60, 60, 60]] and not cls[0] & (D.C_SMALL | D.C_STRONG_P | D.C_STRONG_Q)
    # bS 4, small, ap only: strong on the p side
    out, cls = D.filter_lines([[40, 44, 48, 50, 52, 56, 62, 70]], [4], [20], [7], [0], False)
    assert out.tolist() == [[40, 45, 49, 50, 53, 56, 62, 70]] and cls[0] & D.C_STRONG_P and not cls[0] & D.C_STRONG_Q and cls[0] & D.C_SMALL
    # chroma, bS 2, tC0 0: tc 1; p0 + delta below 0
    out, cls = D.filter_lines([[0, 0, 0, 9]], [2], [10], [10], [0], True)
    assert out.tolist() == [[0, 0, 1, 9]] and D.field(cls[0], D.C_P0_SHIFT) == 1 and cls[0] & D.C_TC0_ZERO
    # rejected by the second test
    out, cls = D.filter_lines([[9, 0, 1, 1]], [3], [10], [9], [5], True)
    assert out.tolist() == [[9, 0, 1, 1]] and D.field(cls[0], D.C_REJ_SHIFT, 7) == D.REJ_BETA_P


def test_probe_refuses_what_a_lane_cannot_hold(H):
    """pairs of lines that a lane of k_deblock cannot hold, sizes that are no whole wavefronts of the packed layout, bS 4 on an inner edge"""
    f = H.load_hooks().h264mi_internal_deblock_edge_probe
    n = 128
    s, out = np.zeros((n, 8), np.uint8), np.zeros((n, 8), np.uint8)
    bs, one = np.ones(n, np.uint8), np.ones(n, np.uint8)
    odd = one.copy()
    odd[1] = 2
    p = lambda a: a.ctypes.data
    assert f(0, 0, 1, p(s), p(odd), p(one), p(one), p(one), p(out), n) == -1
    assert f(0, 0, 1, p(s), p(bs), p(odd), p(one), p(one), p(out), n) == -1
    assert f(0, 1, 1, p(s), p(odd), p(one), p(one), p(one), p(out), n) == -1
    assert f(1, 0, 0, p(s), p(bs * 4), p(one), p(one), p(one), p(out), n) == -1
    assert f(1, 0, 1, p(s), p(bs), p(one), p(one), p(one), p(out), 64) == -1
    assert f(2, 0, 1, p(s), p(bs), p(one), p(one), p(one), p(out), n) == -1
    assert f(1, 0, 1, None, p(bs), p(one), p(one), p(one), p(out), n) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("impl", (0, 1))
@pytest.mark.parametrize("chroma,mb_edge", KINDS)
def test_gpu_edge_functions_equal_the_rule(chroma, mb_edge, impl, H):
    s, bs, alpha, beta, tc0, want, cls, _ = case(chroma, mb_edge)
    got = np.full_like(s, 0x5A)
    p = lambda a: a.ctypes.data
    r = H.load_hooks().h264mi_internal_deblock_edge_probe(impl, chroma, mb_edge, p(s), p(bs), p(alpha), p(beta), p(tc0), p(got), N)
    assert r == 0, H.load().h264mi_last_error_string()
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        i = int(bad[0])
        print("%d of %d lines differ; first: line %d (wavefront %d), bS %d alpha %d beta %d tC0 %d\n  in   %s\n  want %s\n  got  %s\n  class: %s" % (
            bad.size, N, i, i // (WAVE_LINES if impl == 0 else 64), bs[i], alpha[i], beta[i], tc0[i], s[i].tolist(), want[i].tolist(), got[i].tolist(), D.describe(cls[i])))
        print("  classes of the differing lines:", sorted({D.describe(c) for c in cls[bad[:2000]]})[:12])
    assert bad.size == 0
