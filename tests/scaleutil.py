"""The yardstick of the scaled output (include/h264mi.h, "Scaled output"): resize a tight I420 frame and convert it, in numpy.

Exactly the integer rule, per plane and per axis: luma w x h -> ow x oh, each chroma plane ceil(w / 2) x ceil(h / 2) -> ceil(ow / 2) x ceil(oh / 2), scaled as
planes, centre-aligned.  Every output index of an axis has a short list of taps (source index, integer weight), built by explicit loops from the text of
the rule; a plane is scaled by the two tap matrices, W_y S W_x^T in int64 (so nothing can wrap unseen), with the one rounding of the filter at the end,
and `limits` asserts that every intermediate fits the 32 bits the rule promises.  The conversion of the scaled frame is cscutil's.  Nothing here calls
the product, the oracle or the generator."""
import numpy as np

import cscutil

BILINEAR, AREA = 0, 1  # H264MI_SCALE_BILINEAR / _AREA
FILTERS = {"bilinear": BILINEAR, "area": AREA}
MAX = 16384            # H264MI_SCALE_MAX


def taps(filter, n_in, n_out, i):
    """([source indices], [weights]) of output index i on an axis of n_in samples scaled to n_out."""
    assert 1 <= n_in <= MAX and 1 <= n_out <= MAX and 0 <= i < n_out
    if filter == BILINEAR:
        step = (n_in << 16) // n_out
        p = i * step + (step >> 1) - 32768
        assert i * step < 2 ** 31 and -2 ** 31 <= p < 2 ** 31
        p = min(max(p, 0), (n_in - 1) << 16)
        a, f = p >> 16, (p >> 8) & 255
        return [a, min(a + 1, n_in - 1)], [256 - f, f]
    assert filter == AREA and n_out <= n_in
    idx, wts = [], []
    k = (i * n_in) // n_out  # the first source sample [k n_out, (k + 1) n_out) that reaches into [i n_in, (i + 1) n_in)
    while k * n_out < (i + 1) * n_in:
        idx.append(k)
        wts.append(min((i + 1) * n_in, (k + 1) * n_out) - max(i * n_in, k * n_out))
        k += 1
    assert all(v > 0 for v in wts) and idx[-1] < n_in
    return idx, wts


def area_weight(n_in, n_out, i, k):
    """The overlap formula of the rule, literally: what `taps` walks through."""
    return max(0, min((i + 1) * n_in, (k + 1) * n_out) - max(i * n_in, k * n_out))


def matrix(filter, n_in, n_out):
    """int64[n_out][n_in]: row i holds the weights of output index i (taps that meet at a clamp add up)."""
    m = np.zeros((n_out, n_in), dtype=np.int64)
    for i in range(n_out):
        for k, wt in zip(*taps(filter, n_in, n_out, i)):
            m[i, k] += wt
    return m


def scale_plane(src, ow, oh, filter):
    """uint8[h][w] -> uint8[oh][ow]."""
    src = np.asarray(src)
    h, w = src.shape
    v = matrix(filter, h, oh) @ src.astype(np.int64) @ matrix(filter, w, ow).T
    if filter == BILINEAR:
        assert v.max() + 32768 < 2 ** 24  # the rule: the sum is below 2^24
        out = (v + 32768) >> 16
    else:
        assert 255 * w * h + ((w * h) >> 1) < 2 ** 32 and v.max() + ((w * h) >> 1) < 2 ** 32  # unsigned 32-bit arithmetic
        out = (v + ((w * h) >> 1)) // (w * h)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def scale_plane_real(src, ow, oh):
    """Centre-aligned bilinear interpolation in float64, unrounded: what the integer bilinear rule approximates."""
    src = np.asarray(src).astype(np.float64)
    h, w = src.shape

    def axis(n_in, n_out):
        c = np.clip((np.arange(n_out) + 0.5) * n_in / n_out - 0.5, 0, n_in - 1)
        a = np.floor(c).astype(np.int64)
        return a, np.minimum(a + 1, n_in - 1), c - a
    ax, bx, fx = axis(w, ow)
    ay, by, fy = axis(h, oh)
    top = (1 - fx) * src[ay][:, ax] + fx * src[ay][:, bx]
    bot = (1 - fx) * src[by][:, ax] + fx * src[by][:, bx]
    return (1 - fy)[:, None] * top + fy[:, None] * bot


def scale_i420(frame, w, h, ow, oh, filter):
    """A tight I420 frame of w x h -> the tight I420 frame of ow x oh."""
    y, cb, cr = cscutil.planes(frame, w, h)
    owc, ohc = (ow + 1) // 2, (oh + 1) // 2
    return np.concatenate([scale_plane(y, ow, oh, filter).reshape(-1), scale_plane(cb, owc, ohc, filter).reshape(-1), scale_plane(cr, owc, ohc, filter).reshape(-1)])


def scale_convert(frame, w, h, ow, oh, filter, fmt, csc=0):
    """The frame scaled to ow x oh in layout `fmt` ("i420", "nv12", "rgb24", "rgbp") as a flat uint8 array: cscutil's rule on the scaled frame."""
    s = scale_i420(frame, w, h, ow, oh, filter)
    if fmt == "i420":
        assert csc == 0
        return s
    return cscutil.convert(s, ow, oh, fmt, csc)


def scale_convert_all(frames, w, h, ow, oh, filter, fmt, csc=0):
    return np.concatenate([scale_convert(f, w, h, ow, oh, filter, fmt, csc) for f in frames])


def limits(filter, n_in, n_out):
    """The extreme intermediates of one axis, as Python integers: (largest i * step, smallest and largest unclamped position) for bilinear,
    (largest tap count, largest (k + 1) * n_out the tap walk forms) for area."""
    if filter == BILINEAR:
        step = (n_in << 16) // n_out
        return (n_out - 1) * step, (step >> 1) - 32768, (n_out - 1) * step + (step >> 1) - 32768
    counts = [len(taps(AREA, n_in, n_out, i)[0]) for i in sorted({0, 1 % n_out, n_out // 2, n_out - 1})]
    return max(counts), (taps(AREA, n_in, n_out, n_out - 1)[0][-1] + 1) * n_out
