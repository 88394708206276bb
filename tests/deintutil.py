"""The yardstick of the deinterlaced output (include/h264mi.h, "Deinterlaced output"): the three modes on a tight I420 frame, in numpy.

Written from the header's text, row by row, in int64: each plane on its own with the same parity, luma
h x w, each chroma plane ceil(h / 2) x ceil(w / 2); every clamp at the edge of the plane.  Nothing here calls the product, the oracle or the generator."""
import numpy as np

import cscutil

FIELD, BLEND, EDGE = 0, 1, 2  # H264MI_DEINT_*
MODES = {"field": FIELD, "blend": BLEND, "edge": EDGE}
PARITY_FIRST = -1             # H264MI_DEINT_PARITY_FIRST
MAX = 16384                   # H264MI_SCALE_MAX


def rows(mode, parity, n_rows, y):
    """(kept, up, dn) of row y of a plane of n_rows rows; None for illegal arguments.  kept = 1: the row is copied, up = dn = y."""
    if mode not in (FIELD, BLEND, EDGE) or parity not in (0, 1) or (mode == BLEND and parity != 0):
        return None
    if not 1 <= n_rows <= MAX or not 0 <= y < n_rows:
        return None
    if mode == BLEND:
        return 0, max(y - 1, 0), min(y + 1, n_rows - 1)
    if (y & 1) == parity:
        return 1, y, y
    up, dn = y - 1, y + 1
    if up < 0:
        up = dn
    if dn >= n_rows:
        dn = up
    if not 0 <= up < n_rows:  # neither row exists: one row, parity 1
        return 1, y, y
    return 0, up, dn


def plane(src, mode, parity, luma):
    """uint8[hp][wp] -> uint8[hp][wp].  luma: the plane takes the EDGE rule under EDGE (chroma planes follow FIELD)."""
    s = np.asarray(src).astype(np.int64)
    hp, wp = s.shape
    out = np.empty_like(s)
    for y in range(hp):
        kept, up, dn = rows(mode, parity, hp, y)
        if kept:
            out[y] = s[y]
        elif mode == BLEND:
            out[y] = (s[up] + 2 * s[y] + s[dn] + 2) >> 2
        elif mode == FIELD or not luma or up == dn:
            out[y] = (s[up] + s[dn] + 1) >> 1  # (up == dn: the sample itself)
        else:
            x = np.arange(wp)
            cost = None
            for d in (0, -1, 1):  # in that order: a later direction wins only with a strictly smaller cost
                a, b = s[up][np.clip(x + d, 0, wp - 1)], s[dn][np.clip(x - d, 0, wp - 1)]
                take = np.ones(wp, bool) if cost is None else np.abs(a - b) < cost
                cost = np.where(take, np.abs(a - b), 0 if cost is None else cost)
                out[y] = np.where(take, (a + b + 1) >> 1, out[y])
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def frame(i420, w, h, mode, parity):
    """A tight I420 frame of w x h -> the deinterlaced tight I420 frame."""
    y, cb, cr = cscutil.planes(i420, w, h)
    return np.concatenate([plane(y, mode, parity, True).reshape(-1), plane(cb, mode, parity, False).reshape(-1), plane(cr, mode, parity, False).reshape(-1)])
