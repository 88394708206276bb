"""The yardstick of the output formats (include/h264mi.h, "Output formats"): NV12 and RGB from a tight I420 frame, in numpy.

Exactly the integer rule: coefficients rounded from Kr, Kb at 13 fractional bits, int32 arithmetic, one `+ 4096 >> 13` (floor) per component, clip to
0..255; chroma either repeated (nearest) or interpolated for the 4:2:0 siting of chroma_sample_loc_type 0 with weights 3:1 vertically and 1:1 between
columns, one rounding, clamped at the edges of the frame's own chroma planes.  Nothing here calls the product, the oracle or the generator."""
import numpy as np

BT601, BT709 = 1, 2            # H264MI_CSC_BT601 / _BT709
FULL_RANGE, BILINEAR = 16, 32  # H264MI_CSC_FULL_RANGE / _CHROMA_BILINEAR
KR_KB = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722)}


def coefficients(matrix, full):
    """(cy, crv, cgu, cgv, cbu) in 1/8192, rounded half up from float64."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
    real = (sy, 2 * (1 - kr) * sc, 2 * kb * (1 - kb) / kg * sc, 2 * kr * (1 - kr) / kg * sc, 2 * (1 - kb) * sc)
    return tuple(int(np.floor(8192.0 * v + 0.5)) for v in real)


def ycc_to_rgb(y, cb, cr, matrix, full):
    """int32 arrays of one shape (8-bit values) -> uint8[..., 3]."""
    cy, crv, cgu, cgv, cbu = (np.int32(c) for c in coefficients(matrix, full))
    y = y.astype(np.int32) - np.int32(0 if full else 16)
    u, v = cb.astype(np.int32) - np.int32(128), cr.astype(np.int32) - np.int32(128)
    r = (cy * y + crv * v + np.int32(4096)) >> 13
    g = (cy * y - cgu * u - cgv * v + np.int32(4096)) >> 13
    b = (cy * y + cbu * u + np.int32(4096)) >> 13
    assert r.dtype == np.int32 and g.dtype == np.int32 and b.dtype == np.int32
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def ycc_to_rgb_real(y, cb, cr, matrix, full):
    """The real-valued formula in float64, rounded half up and clipped: what the integer rule approximates."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
    yy = (y.astype(np.float64) - (0 if full else 16)) * sy
    u, v = (cb.astype(np.float64) - 128) * sc, (cr.astype(np.float64) - 128) * sc
    r = yy + 2 * (1 - kr) * v
    g = yy - 2 * kb * (1 - kb) / kg * u - 2 * kr * (1 - kr) / kg * v
    b = yy + 2 * (1 - kb) * u
    return np.clip(np.floor(np.stack([r, g, b], axis=-1) + 0.5), 0, 255).astype(np.uint8)


def planes(frame, w, h):
    """Y[h][w], Cb[hc][wc], Cr[hc][wc] of a tight I420 frame."""
    wc, hc = (w + 1) // 2, (h + 1) // 2
    frame = np.asarray(frame)
    assert frame.shape == (w * h + 2 * wc * hc,)
    return frame[:w * h].reshape(h, w), frame[w * h:w * h + wc * hc].reshape(hc, wc), frame[w * h + wc * hc:].reshape(hc, wc)


def upsample_nearest(c, w, h):
    return c[np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1].astype(np.int32)


def upsample_bilinear(c, w, h):
    hc, wc = c.shape
    c = c.astype(np.int32)
    x, y = np.arange(w), np.arange(h)
    k, j = x >> 1, y >> 1
    k1 = np.where(x & 1, np.minimum(k + 1, wc - 1), k)  # even x: 2 C[k]; odd x: C[k] + C[min(k + 1, wc - 1)]
    hrow = c[:, k] + c[:, k1]                            # [hc][w]
    j1 = np.where(y & 1, np.minimum(j + 1, hc - 1), np.maximum(j - 1, 0))
    return (3 * hrow[j] + hrow[j1] + 4) >> 3


def to_rgb(frame, w, h, csc):
    """uint8[h][w][3] of a tight I420 frame; csc = BT601 / BT709 | FULL_RANGE | BILINEAR (a resolved value: never AUTO)."""
    y, cb, cr = planes(frame, w, h)
    up = upsample_bilinear if csc & BILINEAR else upsample_nearest
    return ycc_to_rgb(y, up(cb, w, h), up(cr, w, h), csc & 15, bool(csc & FULL_RANGE))


def to_nv12(frame, w, h):
    y, cb, cr = planes(frame, w, h)
    return np.concatenate([y.reshape(-1), np.stack([cb, cr], axis=-1).reshape(-1)])


def convert(frame, w, h, fmt, csc=0):
    """The frame in layout `fmt` ("nv12", "rgb24", "rgbp") as a flat uint8 array."""
    if fmt == "nv12":
        assert csc == 0
        return to_nv12(frame, w, h)
    rgb = to_rgb(frame, w, h, csc)
    return (rgb if fmt == "rgb24" else rgb.transpose(2, 0, 1)).reshape(-1).copy()


def convert_all(frames, w, h, fmt, csc=0):
    return np.concatenate([convert(f, w, h, fmt, csc) for f in frames])


def output_size(fmt, w, h):
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2) if fmt in ("i420", "nv12") else 3 * w * h


def resolve_auto(matrix_coefficients, video_full_range, w, h):
    """What H264MI_CSC_AUTO stands for: BT601 / BT709 | FULL_RANGE, or None where the matrix is neither."""
    if matrix_coefficients == 1:
        m = BT709
    elif matrix_coefficients in (5, 6):
        m = BT601
    elif matrix_coefficients == 2:
        m = BT709 if (w >= 1280 or h > 576) else BT601
    else:
        return None
    return m | (FULL_RANGE if video_full_range else 0)
