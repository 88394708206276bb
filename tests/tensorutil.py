"""The yardstick of the model-input tensors (include/h264mi.h, "Model input"): region, placement, canvas, element mapping and layout, in numpy.

A tensor item is a function of the tight I420 frame, the region, the spec, scaleutil's rule and cscutil's rule: the region frame is cut out of the
display planes, scaled to the picture size `fit_rect` gives (scaleutil.scale_i420), converted to RGB (cscutil.convert on the scaled frame), placed in
the canvas among pad pixels, and every 8-bit value is mapped by two float32 operations -- a multiply and an add, each rounded, numpy never fuses them --
and rounded to the element type.  Nothing here calls the product, the oracle or the generator."""
from fractions import Fraction

import numpy as np

import cscutil
import scaleutil

STRETCH, LETTERBOX = 0, 1                 # H264MI_FIT_*
U8, F16, BF16, F32 = 0, 1, 2, 3           # H264MI_DT_*
ELEM = {U8: 1, F16: 2, BF16: 2, F32: 4}
MAX = scaleutil.MAX
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def fit_rect(fit, w, h, ow, oh):
    """(px, py, sw, sh): where a w x h source goes in an ow x oh canvas.  Python integers, // is floor; None for illegal arguments."""
    if fit not in (STRETCH, LETTERBOX) or not all(1 <= v <= MAX for v in (w, h, ow, oh)):
        return None
    if fit == STRETCH:
        return 0, 0, ow, oh
    if w * oh >= h * ow:
        sw, sh = ow, min(max((2 * h * ow + w) // (2 * w), 1), oh)
    else:
        sh, sw = oh, min(max((2 * w * oh + h) // (2 * h), 1), ow)
    assert 2 * max(w, h) * max(ow, oh) + max(w, h) < 2 ** 31  # the rule promises 32 bits
    return (ow - sw) >> 1, (oh - sh) >> 1, sw, sh


def region_frame(i420, w, h, x, y, rw, rh):
    """The tight I420 frame of region (x, y, rw, rh) of a tight w x h frame: Y[y : y + rh, x : x + rw], C[y / 2 : y / 2 + ceil(rh / 2), x / 2 : ...]."""
    assert x % 2 == 0 and y % 2 == 0 and rw >= 1 and rh >= 1 and x + rw <= w and y + rh <= h
    yy, cb, cr = cscutil.planes(i420, w, h)
    cw, ch = (rw + 1) // 2, (rh + 1) // 2
    assert x // 2 + cw <= cb.shape[1] and y // 2 + ch <= cb.shape[0]  # always inside the display chroma plane
    return np.concatenate([yy[y:y + rh, x:x + rw].reshape(-1), cb[y // 2:y // 2 + ch, x // 2:x // 2 + cw].reshape(-1), cr[y // 2:y // 2 + ch, x // 2:x // 2 + cw].reshape(-1)])


def place(picture, px, py, ow, oh, pad):
    """uint8[sh][sw][3] at (px, py) of a uint8[oh][ow][3] canvas of pad = (R, G, B)."""
    sh, sw = picture.shape[:2]
    assert 0 <= px and px + sw <= ow and 0 <= py and py + sh <= oh
    canvas = np.empty((oh, ow, 3), np.uint8)
    canvas[:] = np.asarray(pad[:3], np.uint8)
    canvas[py:py + sh, px:px + sw] = picture
    return canvas


def item(i420, w, h, region, size, fit, filter, csc, pad):
    """The 8-bit canvas uint8[oh][ow][3] (colours R, G, B) of one item: region = (x, y, rw, rh) or None for the whole frame, size = (ow, oh), csc a
    resolved value (never AUTO)."""
    x, y, rw, rh = (0, 0, w, h) if region is None or tuple(region[2:]) == (0, 0) else region
    px, py, sw, sh = fit_rect(fit, rw, rh, size[0], size[1])
    assert filter == scaleutil.BILINEAR or (sw <= rw and sh <= rh)
    scaled = scaleutil.scale_i420(region_frame(i420, w, h, x, y, rw, rh), rw, rh, sw, sh, filter)
    picture = cscutil.convert(scaled, sw, sh, "rgb24", csc).reshape(sh, sw, 3)
    return place(picture, px, py, size[0], size[1], pad)


def bf16_bits(r):
    """float32 array -> uint16 bfloat16 bit patterns, round to nearest even, by the bit rule (finite values)."""
    u = np.asarray(r, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def mapped(v, dtype, scale, bias):
    """The elements of 8-bit values v of ONE colour: uint8, float16, uint16 (bfloat16 bit patterns) or float32."""
    v = np.asarray(v, np.uint8)
    if dtype == U8:
        assert scale == 1 and bias == 0
        return v
    prod = v.astype(np.float32) * np.float32(scale)  # rounded to float32 ...
    r = prod + np.float32(bias)                      # ... and rounded again: two operations
    assert prod.dtype == np.float32 and r.dtype == np.float32
    if dtype == F32:
        return r
    if dtype == F16:
        with np.errstate(over="ignore"):
            return r.astype(np.float16)
    assert dtype == BF16
    return bf16_bits(r)


def elements(canvas, dtype, scale=(1, 1, 1), bias=(0, 0, 0), fmt="rgbp", bgr=False):
    """The item of an 8-bit canvas uint8[oh][ow][3] as a flat array of bytes: element mapping per colour, BGR, layout."""
    planes = [mapped(canvas[..., c], dtype, scale[c], bias[c]) for c in range(3)]
    if bgr:
        planes = planes[::-1]
    out = np.stack(planes, axis=0 if fmt == "rgbp" else -1)
    assert fmt in ("rgbp", "rgb24")
    return np.ascontiguousarray(out).reshape(-1).view(np.uint8)


def mean_std(mean, std):
    """scale, bias of frames_tensor(mean=, std=): Python doubles, rounded to float32 once."""
    return tuple(np.float32(1.0 / (255.0 * s)) for s in std), tuple(np.float32(-m / s) for m, s in zip(mean, std))


def round_f32(q):
    """A Fraction rounded to the nearest float32, ties to even: exact, for checking what a single (fused) rounding would give."""
    f = np.float32(float(q))  # within one float32 step of the answer
    cands = sorted({float(np.nextafter(f, np.float32(-np.inf))), float(f), float(np.nextafter(f, np.float32(np.inf)))})
    best = min(cands, key=lambda c: (abs(Fraction(c) - q), int(np.float32(c).view(np.uint32)) & 1))
    return np.float32(best)


def fused(v, scale, bias):
    """What one fused multiply-add would give for value v: float32(v * scale + bias) with ONE rounding (exact arithmetic in between)."""
    return round_f32(Fraction(int(v)) * Fraction(float(np.float32(scale))) + Fraction(float(np.float32(bias))))
