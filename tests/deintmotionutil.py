"""The yardstick of motion-adaptive deinterlacing (include/h264mi.h, "Motion-adaptive deinterlacing"), in numpy int64.

Written from the header's text: a frame is a function of the source's tight I420 frame S, a predecessor's frame P of the same size or None, a spatial
mode M (FIELD or EDGE) and a parity.  Kept rows are copied; a missing row is the spatial value sp pulled to within m of the woven sample t, m the largest
move of rows up, y and dn since P.  sp comes from deintutil.plane and the rows from deintutil.rows; nothing here calls the product, the oracle or the
generator."""
import numpy as np

import cscutil
import deintutil as du

FIELD, EDGE = du.FIELD, du.EDGE
MODES = {"motion": FIELD, "motion_edge": EDGE}
PREV_NONE, PREV_HISTORY, HISTORY = -1, -2, 1  # H264MI_DEINT_PREV_NONE, _PREV_HISTORY; the flag H264MI_DEINT_HISTORY


def pixel(s, p, sp):
    """One sample: s and p are (up, y, dn) of the source and the predecessor (p None: no predecessor), sp the spatial value."""
    if p is None:
        return int(sp)
    m = max(abs(int(s[i]) - int(p[i])) for i in range(3))
    t = int(s[1])
    return min(max(int(sp), t - m), t + m)


def plane(src, prev, mode, parity, luma):
    """uint8[hp][wp] (and the predecessor's plane or None) -> uint8[hp][wp]."""
    assert mode in (FIELD, EDGE) and parity in (0, 1)
    spatial = du.plane(src, mode, parity, luma)
    if prev is None:
        return spatial
    s, p, sp = np.asarray(src).astype(np.int64), np.asarray(prev).astype(np.int64), spatial.astype(np.int64)
    assert s.shape == p.shape
    hp = s.shape[0]
    out = np.empty_like(s)
    for y in range(hp):
        kept, up, dn = du.rows(mode, parity, hp, y)
        if kept:
            out[y] = s[y]
            continue
        m = np.maximum(np.maximum(np.abs(s[up] - p[up]), np.abs(s[dn] - p[dn])), np.abs(s[y] - p[y]))
        out[y] = np.minimum(np.maximum(sp[y], s[y] - m), s[y] + m)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def frame(i420, prev_i420, w, h, mode, parity):
    """A tight I420 frame of w x h and its predecessor (or None) -> the motion-adaptive deinterlaced tight I420 frame."""
    s = cscutil.planes(i420, w, h)
    p = (None, None, None) if prev_i420 is None else cscutil.planes(prev_i420, w, h)
    return np.concatenate([plane(s[i], p[i], mode, parity, i == 0).reshape(-1) for i in range(3)])


def missing_rows(w, h, parity):
    """Boolean mask over a tight I420 frame: the samples of rows that are not kept (the rule is FIELD's and EDGE's alike)."""
    def mask(hp, wp):
        m = np.zeros((hp, wp), bool)
        for y in range(hp):
            m[y] = not du.rows(FIELD, parity, hp, y)[0]
        return m.reshape(-1)
    hc, wc = (h + 1) // 2, (w + 1) // 2
    return np.concatenate([mask(h, w), mask(hc, wc), mask(hc, wc)])
