"""Model input (K9): regions of frames as letterboxed, normalised u8 / f16 / bf16 / f32 tensors, written by one launch.

The yardstick is tests/tensorutil.py -- region, placement, canvas, element mapping and layout of include/h264mi.h ("Model input") in numpy, over
scaleutil's scaler and cscutil's conversion -- applied to the generator's reconstruction.  A tensor item is a function of the tight I420 frame, the
region and the spec, so every GPU comparison is an equality of bit patterns.  The CPU tests pin the yardstick itself (placements worked out by hand,
their properties, the two roundings of the element mapping against an exactly computed fused one, float16 / bfloat16 ties and subnormals) and the
library's pure entry points against it.  The streams are those of test_output_scale.ROWS under other seeds."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cscutil
import scaleutil
import spsutil
import tensorutil as tu
import test_output_convert as toc
import test_output_scale as tos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ECAPACITY = -1, -3, -7
FMT = {"rgb24": 2, "rgbp": 3}
BIL, AREA = scaleutil.BILINEAR, scaleutil.AREA
BT601, BT709, FULL, BILIN = cscutil.BT601, cscutil.BT709, cscutil.FULL_RANGE, cscutil.BILINEAR
S, L = tu.STRETCH, tu.LETTERBOX
U8, F16, BF16, F32 = tu.U8, tu.F16, tu.BF16, tu.F32
DTYPES = {U8: "u8", F16: "f16", BF16: "bf16", F32: "f32"}
PAD = (114, 3, 250)  # unlike per colour: a swapped channel shows
SCALE, BIAS = tu.mean_std(tu.IMAGENET_MEAN, tu.IMAGENET_STD)
CSCS = (BT601, BT709 | FULL | BILIN)  # BT.601 limited nearest, BT.709 full bilinear chroma

# source -> canvas: (px, py, sw, sh), letterbox; worked by hand from the rule
FIT_TABLE = [((16, 16), (33, 19), (7, 0, 19, 19)), ((16, 16), (8, 24), (0, 8, 8, 8)), ((2, 2), (5, 3), (1, 0, 3, 3)), ((2, 2), (1, 1), (0, 0, 1, 1)),
             ((176, 144), (16, 16), (0, 1, 16, 13)), ((37, 21), (16, 16), (0, 3, 16, 9)), ((73, 37), (64, 64), (0, 16, 64, 32)),
             ((174, 144), (50, 37), (2, 0, 45, 37)), ((1920, 1080), (640, 640), (0, 140, 640, 360)), ((16384, 1), (1, 16384), (0, 8191, 1, 1))]
SWEEP = [1, 2, 3, 7, 16, 37, 224, 1080, 1920, 16383, 16384]

# name: (new seed, [(region or None, canvas, fit)]) -- rows of test_output_scale.ROWS
GEOM = {
    "16x16": (3106, [(None, (16, 16), S), (None, (33, 19), L), (None, (8, 24), L), (None, (8, 8), S)]),  # identity; odd px 7; pad rows; exact 2:1
    "two_by_two": (3103, [(None, (5, 3), L), (None, (1, 1), L)]),                                        # chroma 1x1; a canvas of one pixel
    "aligned_origin": (3101, [((32, 16, 64, 48), (64, 48), S), ((2, 6, 37, 21), (16, 16), L)]),           # aligned identity of a region; odd region, 37x21 -> 16x9
    "left_1": (3102, [(None, (50, 37), L), ((4, 2, 50, 37), (50, 37), S)]),                               # 174x144 -> 45x37 at px 2; a region at equal size
    "mono_odd": (3104, [((100, 100, 73, 37), (64, 64), L)]),                                              # reaches the odd right and bottom edges: 73x37 -> 64x32
    "field_pics": (3105, [(None, (86, 58), S)]),
    "qcif": (3107, [(None, (16, 16), L)]),                                                                # 176x144 -> 16x13
}
BGR_ROWS = ("16x16", "qcif")


class Case:
    """A stream of test_output_scale.ROWS under a seed of this file, with its tight I420 frames."""

    def __init__(self, sg, name, seed=None):
        row = tos.ROWS[name][0]
        if isinstance(row, str):
            kw, self.crop = toc.TABLE[row]
            self.rect = toc.RECTS[row]
        else:
            kw, self.crop, self.rect = row, (0, 0, 0, 0), (0, 0, row["width"], row["height"])
        self.kw = dict(kw, seed=GEOM[name][0] if seed is None else seed)
        raw, rec, _ = sg.encode(**self.kw)
        self.stream, self.info = spsutil.recrop(raw, *self.crop) if any(self.crop) else (raw, dict(coded_w=self.kw["width"], coded_h=self.kw["height"]))
        self.i420 = spsutil.expected_frames(rec, self.info, *self.crop) if any(self.crop) else rec
        self.w, self.h = self.rect[2:]
        self.pictures = self.kw["frames"] * (2 if self.kw.get("field_pics") else 1)
        self.i420.setflags(write=False)
        self._canvas = {}

    def canvas(self, frame, region, size, fit, filt, csc, pad=PAD):
        """The yardstick's 8-bit canvas of one item (computed once, never written to)."""
        key = (frame, region, size, fit, filt, csc, pad)
        if key not in self._canvas:
            v = tu.item(self.i420[frame], self.w, self.h, region, size, fit, filt, csc, pad)
            v.setflags(write=False)
            self._canvas[key] = v
        return self._canvas[key]


@pytest.fixture(scope="module")
def cases(sg):
    class Lazy(dict):
        def __missing__(self, name):
            self[name] = Case(sg, name)
            return self[name]
    return Lazy()


def _picture(c, region, size, fit):
    rw, rh = (c.w, c.h) if region is None else region[2:]
    return (rw, rh) + tu.fit_rect(fit, rw, rh, *size)[2:]


# ------------------------------------------------------------------------------------------------ CPU


def test_fit_rect_known_answers_and_properties():
    for (w, h), (ow, oh), want in FIT_TABLE:
        assert tu.fit_rect(L, w, h, ow, oh) == want, (w, h, ow, oh)
        assert tu.fit_rect(S, w, h, ow, oh) == (0, 0, ow, oh)
    for w in SWEEP:
        for h in SWEEP:
            for ow in SWEEP:
                for oh in SWEEP:
                    px, py, sw, sh = tu.fit_rect(L, w, h, ow, oh)
                    assert px >= 0 and py >= 0 and sw >= 1 and sh >= 1 and px + sw <= ow and py + sh <= oh, "the picture lies inside the canvas"
                    assert 0 <= (ow - sw - px) - px <= 1 and 0 <= (oh - sh - py) - py <= 1, "centred: the margins of an axis differ by at most 1"
                    assert sw == ow or sh == oh, "one axis is full"
                    # the other axis: within half a pixel of the exact ratio (in exact integers: |2 w sh - 2 h ow| <= w), unless clamped
                    if sw == ow and w * oh >= h * ow:
                        assert sh == 1 or abs(2 * w * sh - 2 * h * ow) <= w, (w, h, ow, oh)
                    else:
                        assert sh == oh and (sw == 1 or abs(2 * h * sw - 2 * w * oh) <= h), (w, h, ow, oh)


def test_library_fit_rect_equals_the_yardstick(H):
    L_ = H.lib()
    v = [ctypes.c_int32(-7) for _ in range(4)]
    refs = [ctypes.byref(x) for x in v]
    sweep = SWEEP + [0, -1, 16385]
    for fit in (S, L, 2, -1):
        for w in sweep:
            for h in (1, 9, 1080, 16384, 0, 16385):
                for ow in sweep:
                    for oh in (1, 16, 640, 16384, 0, 16385):
                        want = tu.fit_rect(fit, w, h, ow, oh)
                        code = L_.h264mi_fit_rect(fit, w, h, ow, oh, *refs)
                        if want is None:
                            assert code == EINVAL, (fit, w, h, ow, oh)
                        else:
                            assert code == 0 and tuple(x.value for x in v) == want, (fit, w, h, ow, oh)
    for (w, h), (ow, oh), want in FIT_TABLE:
        assert H.fit_rect(H.FIT_LETTERBOX, w, h, ow, oh) == want
    assert L_.h264mi_fit_rect(L, 4, 4, 4, 4, None, refs[1], refs[2], refs[3]) == EINVAL
    with pytest.raises(H.H264MIError):
        H.fit_rect(7, 4, 4, 4, 4)


def test_element_mapping_is_two_roundings_not_a_fused_one():
    """ImageNet constants: the yardstick (a float32 multiply, then a float32 add) against the exactly computed single rounding of v * scale + bias.
    They differ for about half of the 256 values of every colour, so a kernel built with the multiply and add contracted fails the GPU tests at once."""
    v = np.arange(256, dtype=np.uint8)
    for c in range(3):
        two = tu.mapped(v, F32, SCALE[c], BIAS[c])
        assert two.dtype == np.float32
        one = np.array([tu.fused(x, SCALE[c], BIAS[c]) for x in v], np.float32)
        differ = int((two.view(np.uint32) != one.view(np.uint32)).sum())
        print("colour", c, "values where fused differs:", differ)
        assert differ >= 1, "the case discriminates"
        assert np.abs(two.astype(np.float64) - one.astype(np.float64)).max() < 1e-6  # ... by an ulp: the same numbers otherwise
        # and the formula of frames_tensor(mean=, std=): Python doubles rounded once
        assert SCALE[c] == np.float32(1.0 / (255.0 * tu.IMAGENET_STD[c])) and BIAS[c] == np.float32(-tu.IMAGENET_MEAN[c] / tu.IMAGENET_STD[c])
    assert tu.round_f32(tu.Fraction(1, 3)) == np.float32(1.0 / 3.0) and tu.round_f32(tu.Fraction(16777217)) == np.float32(16777216.0)  # a tie goes to even
    assert np.array_equal(tu.mapped(v, U8, 1, 0), v)


def test_float16_and_bfloat16_ties_and_subnormals():
    import torch
    v = np.arange(256, dtype=np.uint8)
    # binary16 has 11 significant bits: 2049 and 2051 lie midway between neighbours and go to the even one
    assert tu.mapped([1, 3, 2], F16, 1.0, 2048.0).tolist() == [2048.0, 2052.0, 2050.0]
    # subnormals are kept: v / (255 * 4096) is below 2^-14 for v <= 63
    sub = tu.mapped(v, F16, np.float32(1.0 / (255.0 * 4096.0)), 0.0).view(np.uint16)
    assert int((((sub & 0x7c00) == 0) & ((sub & 0x3ff) != 0)).sum()) == 63 and sub[0] == 0
    assert np.isinf(tu.mapped([255], F16, 1000.0, 0.0)).all(), "overflow goes to infinity"
    # bfloat16 has 8 significant bits: 257 and 259 are ties
    assert tu.bf16_bits(np.float32([257, 259, 258, 256])).tolist() == [0x4380, 0x4382, 0x4381, 0x4380]
    for c in range(3):
        r = tu.mapped(v, F32, SCALE[c], BIAS[c])
        assert np.array_equal(torch.from_numpy(r.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16), tu.bf16_bits(r)), "the bit rule is torch's"
        assert np.array_equal(torch.from_numpy(r.copy()).to(torch.float16).numpy().view(np.uint16), tu.mapped(v, F16, SCALE[c], BIAS[c]).view(np.uint16))


def test_yardstick_item_by_hand():
    """A 2x2 frame letterboxed into 5x3: the picture is 3x3 at (1, 0), columns 0 and 4 are pad; at equal size the item is cscutil's conversion."""
    rng = np.random.default_rng(9)
    f = rng.integers(0, 256, 4 + 2, dtype=np.uint8)
    c = tu.item(f, 2, 2, None, (5, 3), L, BIL, BT601, PAD)
    assert c.shape == (3, 5, 3) and (c[:, 0] == PAD).all() and (c[:, 4] == PAD).all()
    assert np.array_equal(c[:, 1:4].reshape(-1), scaleutil.scale_convert(f, 2, 2, 3, 3, BIL, "rgb24", BT601))
    g = rng.integers(0, 256, 16 * 8 * 3 // 2, dtype=np.uint8)
    assert np.array_equal(tu.item(g, 16, 8, (0, 0, 0, 0), (16, 8), S, AREA, BT709, PAD).reshape(-1), cscutil.convert(g, 16, 8, "rgb24", BT709))
    # a region: its frame is cut out of the display planes (chroma from (x / 2, y / 2), ceil sizes)
    r = tu.region_frame(g, 16, 8, 2, 4, 5, 3)
    y, cb, cr = cscutil.planes(g, 16, 8)
    assert r.size == 15 + 2 * 6 and np.array_equal(r[:15].reshape(3, 5), y[4:7, 2:7]) and np.array_equal(r[15:21].reshape(2, 3), cb[2:4, 1:4])
    # layout and BGR: scale, bias and pad stay indexed by colour
    e = tu.elements(c, F32, (1, 2, 4), (0, 0, 0), "rgb24", bgr=True).view(np.float32).reshape(3, 5, 3)
    assert e[0, 0].tolist() == [4.0 * PAD[2], 2.0 * PAD[1], 1.0 * PAD[0]]
    assert tu.elements(c, BF16, SCALE, BIAS, "rgbp").size == 3 * 15 * 2


def _spec(H, size, fmt="rgbp", dtype=F32, **kw):
    if dtype != U8:
        kw.setdefault("scale", SCALE)
        kw.setdefault("bias", BIAS)
    return H.tensor_spec(size, fmt, dtype, pad=kw.pop("pad", PAD), **kw)


def test_tensor_size_and_spec_validation(H):
    L_ = H.lib()
    n = ctypes.c_size_t(0)
    for dtype in DTYPES:
        for fmt in FMT:
            sp = _spec(H, (33, 19), fmt, dtype)
            assert L_.h264mi_tensor_size(ctypes.byref(sp), ctypes.byref(n)) == 0 and n.value == 3 * 33 * 19 * tu.ELEM[dtype] == H.Decoder.tensor_size(sp)
    sp = _spec(H, (16384, 16384), "rgbp", F32)
    assert H.Decoder.tensor_size(sp) == 3 * 16384 * 16384 * 4

    def bad(**changes):
        sp = _spec(H, (16, 16), "rgbp", changes.pop("dtype", F32))
        for k, val in changes.items():
            if isinstance(val, tuple):
                for i, x in enumerate(val):
                    getattr(sp, k)[i] = x
            else:
                setattr(sp, k, val)
        n.value = 77
        code = L_.h264mi_tensor_size(ctypes.byref(sp), ctypes.byref(n))
        assert n.value == 77 or code == 0
        return code
    assert bad() == 0
    for changes in (dict(format=0), dict(format=1), dict(format=4), dict(dtype=4), dict(dtype=-1), dict(fit=2), dict(fit=-1), dict(filter=2), dict(filter=-1),
                    dict(flags=2), dict(flags=3), dict(flags=-1), dict(csc=3), dict(csc=FULL), dict(scale=(1.0, float("inf"), 1.0)), dict(scale=(float("nan"), 1.0, 1.0)),
                    dict(bias=(0.0, 0.0, float("-inf"))), dict(dtype=U8, scale=(1.0, 1.0, 0.5)), dict(dtype=U8, bias=(0.25, 0.0, 0.0)),
                    dict(out_w=0), dict(out_h=0), dict(out_w=16385), dict(out_h=16385), dict(out_w=-3)):
        assert bad(**changes) == EINVAL, changes
    assert bad(dtype=U8) == 0 and bad(flags=1) == 0 and bad(csc=BT709 | FULL | BILIN) == 0 and bad(out_w=16384, out_h=1) == 0
    assert L_.h264mi_tensor_size(None, ctypes.byref(n)) == EINVAL
    with pytest.raises(H.H264MIError):
        H.tensor_spec((4, 4), dtype="int8")


def test_new_entry_points_are_declared_and_exported(H):
    hdr = open(os.path.join(ROOT, "include", "h264mi.h")).read()
    from h264decode_amd import _lib
    names = ("h264mi_fit_rect", "h264mi_tensor_size", "h264mi_batch_tensor_device", "h264mi_items_tensor_device")
    for name in names:
        assert ("int32_t %s(" % name) in hdr and name in _lib.EXPORTS and hasattr(H.lib(), name), name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "h264decode_amd", "libh264mi.so")], capture_output=True, text=True, check=True).stdout
    assert all((" T " + name) in out for name in names)
    for line in ("#define H264MI_DT_U8 0", "#define H264MI_DT_F16 1", "#define H264MI_DT_BF16 2", "#define H264MI_DT_F32 3", "#define H264MI_FIT_STRETCH 0",
                 "#define H264MI_FIT_LETTERBOX 1", "#define H264MI_TENSOR_BGR 1"):
        assert line in hdr, line
    assert "Model input (K9)" in hdr
    assert (H.DT_U8, H.DT_F16, H.DT_BF16, H.DT_F32, H.FIT_STRETCH, H.FIT_LETTERBOX, H.TENSOR_BGR) == (0, 1, 2, 3, 0, 1, 1)
    assert ctypes.sizeof(_lib.TensorSpec) == 8 * 4 + 4 + 6 * 4 and ctypes.sizeof(_lib.TensorItem) == 24


# ------------------------------------------------------------------------------------------------ GPU


def _decoder(H, w, h, pictures, streams=1):
    return H.Decoder(max_streams=streams, max_width=w, max_height=h, max_frames_per_batch=pictures, max_slices_per_frame=1)


def _run(dec, spec, want_bytes, items=None, stream=-1, shift=0):
    """tensor_items (or tensor_batch) into a device buffer of exactly the expected size, `shift` bytes into an aligned allocation, with guard bytes
    on both sides, all 0xA5 before."""
    import torch
    buf = torch.full((64 + want_bytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr() + 48 + shift
    n = dec.tensor_batch(base, want_bytes, spec, stream) if items is None else dec.tensor_items(base, want_bytes, spec, items)
    dec.sync()
    got = buf.cpu().numpy()
    assert n == want_bytes
    assert (got[:48 + shift] == 0xA5).all() and (got[48 + shift + want_bytes:] == 0xA5).all(), "K9 wrote outside the destination"
    return got[48 + shift:48 + shift + want_bytes]


def _first_diff(got, want):
    d = np.flatnonzero(got != want)
    return int(d[0]) if d.size else None


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GEOM))
def test_gpu_tensor_geometry_dtype_layout(name, cases, H):
    c = cases[name]
    dec = _decoder(H, c.info["coded_w"], c.info["coded_h"], c.pictures)
    try:
        dec.decode([c.stream])
        assert dec.frame_count(0) == 3
        assert np.array_equal(np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(3)]), c.i420), "the I420 frames themselves"
        for region, size, fit in GEOM[name][1]:
            rw, rh, sw, sh = _picture(c, region, size, fit)
            items = [(0, f) + (region or (0, 0, 0, 0)) for f in range(3)]
            for filt in [BIL] + ([AREA] if sw <= rw and sh <= rh else []):
                for csc in CSCS:
                    canv = [c.canvas(f, region, size, fit, filt, csc) for f in range(3)]
                    combos = [(dt, fmt, False) for dt in DTYPES for fmt in FMT] + ([(F16, "rgb24", True), (U8, "rgbp", True)] if name in BGR_ROWS else [])
                    for dt, fmt, bgr in combos:
                        sc, bi = ((1, 1, 1), (0, 0, 0)) if dt == U8 else (SCALE, BIAS)
                        want = np.concatenate([tu.elements(v, dt, sc, bi, fmt, bgr) for v in canv])
                        spec = _spec(H, size, fmt, dt, csc=csc, filter=filt, letterbox=fit == L, bgr=bgr)
                        assert want.size == 3 * dec.tensor_size(spec)
                        got = _run(dec, spec, want.size, items if region else None, stream=0)
                        assert np.array_equal(got, want), (name, region, size, fit, filt, csc, DTYPES[dt], fmt, bgr, _first_diff(got, want))
                        if filt == BIL and csc == CSCS[1]:  # shifted by one element: the element-store path whatever the geometry
                            got = _run(dec, spec, want.size, items, shift=tu.ELEM[dt])
                            assert np.array_equal(got, want), (name, region, size, DTYPES[dt], fmt, "shifted", _first_diff(got, want))
                    if region is None and size == (c.w, c.h) and fit == S:  # the identity: K9's u8 planes are K7's bytes
                        spec = _spec(H, size, "rgbp", U8, csc=csc, filter=filt)
                        assert np.array_equal(_run(dec, spec, 3 * 3 * c.w * c.h, stream=0), toc._converted(dec, 3 * 3 * c.w * c.h, "rgbp", csc, 0)), (name, filt, csc)
    finally:
        dec.close()


def test_the_table_holds_the_downscaling_pairs_area_needs():
    """(source -> picture) pairs that area runs on, from the table alone: no stream is encoded."""
    sizes = {"16x16": (16, 16), "two_by_two": (2, 2), "aligned_origin": (160, 128), "left_1": (174, 144), "mono_odd": (173, 137), "field_pics": (172, 116), "qcif": (176, 144)}
    pairs = set()
    for name, (_, rows) in GEOM.items():
        assert toc.RECTS.get(name, (0, 0, 176, 144))[2:] == sizes[name]
        for region, size, fit in rows:
            rw, rh = sizes[name] if region is None else region[2:]
            _, _, sw, sh = tu.fit_rect(fit, rw, rh, *size)
            if sw <= rw and sh <= rh:
                pairs.add((rw, rh, sw, sh))
    for need in ((16, 16, 8, 8), (176, 144, 16, 13), (73, 37, 64, 32), (37, 21, 16, 9), (64, 48, 64, 48)):
        assert need in pairs, need


@pytest.fixture(scope="module")
def pair(cases, H):
    """qcif (176x144) and two_by_two (2x2) decoded in one decoder of two streams -- GPU tests only."""
    a, b = cases["qcif"], cases["two_by_two"]
    dec = _decoder(H, 176, 144, 3, streams=2)
    dec.decode([a.stream, b.stream])
    yield dec, a, b
    dec.close()


@pytest.mark.gpu
def test_gpu_one_launch_of_items_over_unlike_streams(pair, H):
    import torch
    dec, a, b = pair
    size, fit = (24, 16), L
    # whole frames of both streams, regions of several frames (one reaching the right and bottom edges), one frame three times
    items = [(0, 1, 0, 0, 0, 0), (1, 2, 0, 0, 0, 0), (0, 1, 16, 8, 64, 48), (0, 0, 100, 60, 76, 84), (1, 0, 0, 0, 2, 2), (0, 2, 2, 2, 1, 1), (0, 1, 0, 0, 176, 144)]
    for dt, fmt, csc in ((F16, "rgbp", BT601), (F32, "rgb24", BT709 | FULL | BILIN), (U8, "rgbp", BT601 | BILIN)):
        spec = _spec(H, size, fmt, dt, csc=csc, letterbox=True)
        one = dec.tensor_size(spec)
        sc, bi = ((1, 1, 1), (0, 0, 0)) if dt == U8 else (SCALE, BIAS)
        want = []
        for s, f, x, y, w, h in items:
            c = (a, b)[s]
            want.append(tu.elements(c.canvas(f, (x, y, w, h) if w else None, size, fit, BIL, csc), dt, sc, bi, fmt))
        assert np.array_equal(want[0], want[6]) and not np.array_equal(want[0], want[2])
        got = _run(dec, spec, len(items) * one, items)
        for i in range(len(items)):
            assert np.array_equal(got[i * one:(i + 1) * one], want[i]), (DTYPES[dt], fmt, "item", i, items[i])
        # one byte short: H264MI_ECAPACITY, *bytes set, nothing written; n = 0 succeeds with *bytes = 0
        buf = torch.full((len(items) * one,), 0xA5, dtype=torch.uint8, device="cuda")
        arr = (H._lib.TensorItem * len(items))(*[H._lib.TensorItem(*it) for it in items])
        n = ctypes.c_size_t(0)
        assert dec._L.h264mi_items_tensor_device(dec._h, ctypes.byref(spec), arr, len(items), buf.data_ptr(), len(items) * one - 1, ctypes.byref(n)) == ECAPACITY
        assert n.value == len(items) * one
        n.value = 5
        assert dec._L.h264mi_items_tensor_device(dec._h, ctypes.byref(spec), arr, 0, buf.data_ptr(), 0, ctypes.byref(n)) == 0 and n.value == 0
        assert dec._L.h264mi_items_tensor_device(dec._h, ctypes.byref(spec), None, 0, buf.data_ptr(), 0, ctypes.byref(n)) == 0 and n.value == 0
        dec.sync()
        assert (buf.cpu().numpy() == 0xA5).all()
    # tensor_batch is the whole of every frame, stream-major, decoding order
    spec = _spec(H, size, "rgbp", BF16, csc=BT601, letterbox=True)
    want = np.concatenate([tu.elements(c.canvas(f, None, size, fit, BIL, BT601), BF16, SCALE, BIAS, "rgbp") for c in (a, b) for f in range(3)])
    assert np.array_equal(_run(dec, spec, want.size), want)
    assert np.array_equal(_run(dec, spec, want.size // 2, stream=1), want[want.size // 2:])


@pytest.mark.gpu
def test_gpu_tensor_illegal_arguments(pair, sg, H):
    import torch
    dec, a, b = pair
    buf = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda")
    n = ctypes.c_size_t(0)

    def call(spec, items, ptr=None, cap=1 << 15):
        arr = (H._lib.TensorItem * len(items))(*[H._lib.TensorItem(*it) for it in items])
        return dec._L.h264mi_items_tensor_device(dec._h, ctypes.byref(spec), arr, len(items), buf.data_ptr() + 16 if ptr is None else ptr, cap, ctypes.byref(n))
    good = (0, 1, 16, 8, 64, 48)
    spec = _spec(H, (16, 16), "rgbp", F32, csc=BT601)
    assert call(spec, [good]) == 0
    dec.sync()
    buf.fill_(0xA5)
    torch.cuda.synchronize()
    for it in ((0, 1, 1, 0, 8, 8), (0, 1, 0, 3, 8, 8),                                  # an odd origin
               (0, 1, 0, 0, 177, 144), (0, 1, 0, 0, 176, 145), (0, 1, 2, 0, 176, 144), (0, 1, 170, 0, 8, 8), (0, 1, 0, 140, 8, 6),  # one past the display size
               (0, 1, 0, 0, 0, 8), (0, 1, 0, 0, 8, 0), (0, 1, 0, 0, -2, 8), (0, 1, -2, 0, 8, 8), (0, 1, 2, 2, 0, 0),  # w = 0 with h != 0; negatives; "whole" from (2, 2)
               (2, 0, 0, 0, 0, 0), (-1, 0, 0, 0, 0, 0), (0, 3, 0, 0, 0, 0), (1, -1, 0, 0, 0, 0)):  # a stream or frame out of range
        assert call(spec, [good, it, good]) == EINVAL, it
        assert "item 1" in dec._L.h264mi_last_error_string().decode(), it
    # area that would upscale in one item of many: the 2x2 frame to 16x16
    area = _spec(H, (16, 16), "rgbp", F32, csc=BT601, filter=AREA)
    assert call(area, [good, (0, 0, 0, 0, 0, 0)]) == 0
    dec.sync()
    buf.fill_(0xA5)
    torch.cuda.synchronize()
    assert call(area, [good, (1, 0, 0, 0, 0, 0), good]) == EINVAL and "scales down" in dec._L.h264mi_last_error_string().decode()
    assert call(area, [(0, 0, 0, 0, 15, 16)]) == EINVAL
    # dst misaligned for the dtype
    for dt, off in ((F32, 1), (F32, 2), (F16, 1), (BF16, 3)):
        assert call(_spec(H, (16, 16), "rgbp", dt, csc=BT601), [good], ptr=buf.data_ptr() + 16 + off) == EINVAL, (dt, off)
    assert call(_spec(H, (16, 16), "rgbp", U8, csc=BT601), [good], ptr=buf.data_ptr() + 16 + 1, cap=0) == ECAPACITY  # u8 has no alignment
    # an illegal spec, a null pointer
    bad = _spec(H, (16, 16), "rgbp", F32, csc=BT601)
    bad.format = 0
    assert call(bad, [good]) == EINVAL
    assert dec._L.h264mi_items_tensor_device(dec._h, None, None, 0, buf.data_ptr(), 16, ctypes.byref(n)) == EINVAL
    assert dec._L.h264mi_batch_tensor_device(dec._h, 2, ctypes.byref(spec), buf.data_ptr(), 1 << 15, ctypes.byref(n)) == EINVAL  # no such stream
    dec.sync()
    assert (buf.cpu().numpy() == 0xA5).all(), "a refused call writes nothing"
    # AUTO over matrix_coefficients 9: H264MI_EUNSUPPORTED, nothing written; an explicit matrix works
    m9 = toc.VuiCase(sg, "m9", 3150)
    d2 = _decoder(H, 176, 144, 3)
    try:
        d2.decode([m9.stream])
        auto = _spec(H, (16, 16), "rgbp", F32)
        arr = (H._lib.TensorItem * 1)(H._lib.TensorItem(*good))
        assert d2._L.h264mi_items_tensor_device(d2._h, ctypes.byref(auto), arr, 1, buf.data_ptr(), 1 << 15, ctypes.byref(n)) == EUNSUPPORTED
        msg = d2._L.h264mi_last_error_string().decode()
        assert "9" in msg and "explicit matrix" in msg
        d2.sync()
        assert (buf.cpu().numpy() == 0xA5).all()
        want = tu.elements(tu.item(m9.i420[1], 176, 144, good[2:], (16, 16), S, BIL, BT709, PAD), F32, SCALE, BIAS, "rgbp")
        assert np.array_equal(_run(d2, _spec(H, (16, 16), "rgbp", F32, csc=BT709), want.size, [good]), want)
    finally:
        d2.close()


@pytest.mark.gpu
def test_gpu_tensor_auto_resolves_from_the_display_size(sg, H):
    """AUTO resolves from each frame's SPS (m1: BT.709; m6_full: BT.601 full range) and, where the SPS says nothing, from the DISPLAY size: a 176x144
    frame is BT.601 even when the canvas is 1280 wide (which, as a display size, would make it BT.709), and for a 64x64 region of it."""
    names = ["m1", "m6_full", "plain"]
    auto = {"m1": BT709, "m6_full": BT601 | FULL, "plain": BT601}
    cs = [toc.VuiCase(sg, n, 3160 + i) for i, n in enumerate(names)]
    dec = _decoder(H, 176, 144, 3, streams=3)
    try:
        dec.decode([c.stream for c in cs])
        for i, (n, c) in enumerate(zip(names, cs)):
            assert cscutil.resolve_auto(c.colour[0], c.colour[1], 176, 144) == auto[n]
            for region, size in (((16, 16, 64, 64), (32, 32)), (None, (1280, 2))):
                assert n != "plain" or cscutil.resolve_auto(2, 0, *size) == (BT709 if size[0] >= 1280 else BT601)
                for fmt, chroma in (("rgbp", 0), ("rgb24", BILIN)):
                    want = tu.elements(tu.item(c.i420[2], 176, 144, region, size, S, BIL, auto[n] | chroma, PAD), U8, fmt=fmt)
                    got = _run(dec, _spec(H, size, fmt, U8, csc=chroma), want.size, [(i, 2) + (region or (0, 0, 0, 0))])
                    assert np.array_equal(got, want), (n, region, size, fmt)
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_next_batch_waits_for_the_tensor_launch(cases, sg, H):
    """tensor_batch of batch n, then batch n + 1 -- other streams -- executed at once, no synchronisation in between: the items of batch n are exact.
    What orders the two is the event of the K9 launch (last_pack): the hooks build shows it recorded by the call and consumed by the execute."""
    import torch
    c = cases["aligned_origin"]
    size = (64, 64)
    spec = _spec(H, size, "rgbp", F16, csc=BT601 | BILIN, letterbox=True)
    want = np.concatenate([tu.elements(c.canvas(f, None, size, L, BIL, BT601 | BILIN), F16, SCALE, BIAS, "rgbp") for f in range(3)])
    others = [spsutil.recrop(sg.encode(**dict(c.kw, seed=3190 + i))[0], *c.crop)[0] for i in range(3)]
    assert all(o != c.stream for o in others)
    pending = H.load_hooks().h264mi_internal_pack_pending
    pending.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]

    def is_pending(dec):
        v = ctypes.c_int32(-1)
        assert pending(dec._h, ctypes.byref(v)) == 0
        return v.value
    dec = _decoder(H, c.info["coded_w"], c.info["coded_h"], c.pictures)
    try:
        bufs = [torch.full((want.size + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(3)]
        assert is_pending(dec) == 0
        for i in range(3):
            dec.prepare([c.stream])
            dec.execute()
            assert is_pending(dec) == 0, "the execute consumes the event"
            assert dec.tensor_batch(bufs[i].data_ptr(), want.size, spec) == want.size
            assert is_pending(dec) == 1, "the K9 launch is recorded for the next pass to wait for"
            dec.prepare([others[i]])  # batch n + 1 decodes other samples into the pool while K9 may still read batch n
            dec.execute()
            assert is_pending(dec) == 0
        dec.sync()
        for b in bufs:
            got = b.cpu().numpy()
            assert np.array_equal(got[:want.size], want) and (got[want.size:] == 0xA5).all()
        dec.prepare([c.stream])
        dec.execute()
        dec.sync()
        assert np.array_equal(np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(3)]), c.i420)
        n = ctypes.c_size_t(0)  # a call that launches nothing records nothing
        assert dec._L.h264mi_batch_tensor_device(dec._h, 0, ctypes.byref(spec), bufs[0].data_ptr(), 2, ctypes.byref(n)) == ECAPACITY
        assert is_pending(dec) == 0
    finally:
        dec.close()


def _pending_hook(H):
    pending = H.load_hooks().h264mi_internal_pack_pending
    pending.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]

    def is_pending(dec):
        v = ctypes.c_int32(-1)
        assert pending(dec._h, ctypes.byref(v)) == 0
        return v.value
    return is_pending


@pytest.mark.gpu
def test_gpu_descriptor_tables_grow_and_alternate(sg, H):
    """Three tensor_items calls with no synchronisation between them: 65 items (past the 64 descriptors a table starts with), 1 item (the other table
    of the pair), 130 items (the first table again, grown a second time while the launch of the first call may still be running).  Every item of every
    call is exact and nothing is written behind a buffer.  One 16x16 picture, regions of it on an 8x8 canvas, u8."""
    import torch
    kw, _ = toc.TABLE["16x16"]
    raw, rec, _ = sg.encode(**dict(kw, frames=1, seed=3170))
    size, csc = (8, 8), BT601 | BILIN
    spec = _spec(H, size, "rgbp", U8, csc=csc)
    one = 3 * 8 * 8
    # unlike regions with even origins, all inside the frame
    regions = []
    for k in range(65 + 1 + 130):
        x, y = 2 * (k % 8), 2 * ((k // 8) % 8)
        regions.append((x, y, 1 + (5 * k) % (16 - x), 1 + (3 * k) % (16 - y)))
    wants = {}
    for r in set(regions):
        wants[r] = tu.elements(tu.item(rec[0], 16, 16, r, size, S, BIL, csc, PAD), U8)
    assert len(wants) > 100 and all(v.size == one for v in wants.values())
    calls = [regions[:65], regions[65:66], regions[66:]]
    dec = _decoder(H, 16, 16, 1)
    try:
        dec.decode([raw])
        assert dec.frame_count(0) == 1
        bufs = [torch.full((len(c) * one + 64,), 0xA5, dtype=torch.uint8, device="cuda") for c in calls]
        for c, b in zip(calls, bufs):
            assert dec.tensor_items(b.data_ptr(), len(c) * one, spec, [(0, 0) + r for r in c]) == len(c) * one
        dec.sync()
        for n, (c, b) in enumerate(zip(calls, bufs)):
            got = b.cpu().numpy()
            assert (got[len(c) * one:] == 0xA5).all(), ("call", n, "wrote behind its buffer")
            for i, r in enumerate(c):
                assert np.array_equal(got[i * one:(i + 1) * one], wants[r]), ("call", n, "item", i, r)
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_the_four_output_kernels_on_one_batch(cases, H):
    """pack_batch, convert_batch, scale_batch and tensor_batch of the same batch, one behind the other with no synchronisation, for three rounds (every
    descriptor table of every family is used again): each call records its launch for the next pass to wait for, the next execute consumes it, all
    twelve buffers are exact, and a call of any family that fails launches and records nothing."""
    import torch
    c = cases["aligned_origin"]
    size, csc = (48, 32), BT601 | BILIN
    spec = _spec(H, size, "rgbp", U8, csc=csc)
    want = {"pack": np.concatenate(list(c.i420)),
            "convert": cscutil.convert_all(c.i420, c.w, c.h, "rgbp", csc),
            "scale": np.concatenate([scaleutil.scale_convert(f, c.w, c.h, size[0], size[1], BIL, "rgbp", csc) for f in c.i420]),
            "tensor": np.concatenate([tu.elements(c.canvas(f, None, size, S, BIL, csc), U8) for f in range(3)])}
    call = {"pack": lambda dec, p, cap: dec.pack_batch(p, cap),
            "convert": lambda dec, p, cap: dec.convert_batch(p, cap, "rgbp", csc),
            "scale": lambda dec, p, cap: dec.scale_batch(p, cap, "rgbp", size, csc, "bilinear"),
            "tensor": lambda dec, p, cap: dec.tensor_batch(p, cap, spec)}
    is_pending = _pending_hook(H)
    dec = _decoder(H, c.info["coded_w"], c.info["coded_h"], c.pictures)
    try:
        bufs = [{k: torch.full((v.size + 64,), 0xA5, dtype=torch.uint8, device="cuda") for k, v in want.items()} for _ in range(3)]
        for rnd in range(3):
            dec.prepare([c.stream])
            dec.execute()
            assert is_pending(dec) == 0, "the execute consumes the event"
            for k in want:
                assert call[k](dec, bufs[rnd][k].data_ptr(), want[k].size) == want[k].size
                assert is_pending(dec) == 1, (k, "the launch is recorded for the next pass to wait for")
        dec.prepare([c.stream])
        dec.execute()
        assert is_pending(dec) == 0
        for k in want:  # one byte of capacity: nothing is launched, nothing recorded
            with pytest.raises(H.H264MIError) as e:
                call[k](dec, bufs[0][k].data_ptr(), 1)
            assert e.value.code == ECAPACITY and is_pending(dec) == 0, k
        dec.sync()
        for rnd in range(3):
            for k, v in want.items():
                got = bufs[rnd][k].cpu().numpy()
                assert np.array_equal(got[:v.size], v) and (got[v.size:] == 0xA5).all(), (rnd, k, _first_diff(got[:v.size], v))
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_frames_tensor_with_the_model_keywords(pair, H):
    import torch
    dec, a, b = pair
    size = (32, 32)
    pad = (114, 114, 114)

    def bits(t):
        return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)

    def want(c, frames, region, fit, csc, dt, fmt, sc=(1, 1, 1), bi=(0, 0, 0), bgr=False, p=pad):
        return np.concatenate([tu.elements(c.canvas(f, region, size, fit, BIL, csc, p), dt, sc, bi, fmt, bgr) for f in frames])
    # the defaults still are K8's uint8 tensor
    t = dec.frames_tensor(0, size=size)
    assert t.dtype == torch.uint8 and tuple(t.shape) == (3, 3, 32, 32)
    assert np.array_equal(bits(t), np.concatenate([scaleutil.scale_convert(f, 176, 144, 32, 32, BIL, "rgbp", BT601) for f in a.i420]))
    # AUTO: no VUI, 176x144 -> BT.601 limited
    t = dec.frames_tensor(0, size=size, dtype=torch.float16, mean=tu.IMAGENET_MEAN, std=tu.IMAGENET_STD, letterbox=True)
    assert t.dtype == torch.float16 and t.is_cuda and tuple(t.shape) == (3, 3, 32, 32)
    assert np.array_equal(bits(t), want(a, range(3), None, L, BT601, F16, "rgbp", SCALE, BIAS))
    t2 = dec.frames_tensor(0, size=size, dtype="f16", scale=[float(s) for s in SCALE], bias=[float(x) for x in BIAS], letterbox=True)
    assert torch.equal(t.view(torch.int16), t2.view(torch.int16)), "mean / std are scale / bias by the documented formula"
    t = dec.frames_tensor(-1, "rgb24", BT709 | FULL | BILIN, size=size, dtype=torch.float32, scale=(2.0, 0.5, 1.0), bias=(-1.0, 0.0, 3.0), bgr=True, pad=PAD)
    assert t.dtype == torch.float32 and tuple(t.shape) == (6, 32, 32, 3)
    w6 = np.concatenate([want(c, range(3), None, S, BT709 | FULL | BILIN, F32, "rgb24", (2.0, 0.5, 1.0), (-1.0, 0.0, 3.0), True, PAD) for c in (a, b)])
    assert np.array_equal(bits(t), w6)
    t = dec.frames_tensor(0, size=size, csc=BT601, dtype=torch.bfloat16, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25))
    sc, bi = tu.mean_std((0.5, 0.5, 0.5), (0.25, 0.25, 0.25))
    assert t.dtype == torch.bfloat16 and tuple(t.shape) == (3, 3, 32, 32) and np.array_equal(bits(t), want(a, range(3), None, S, BT601, BF16, "rgbp", sc, bi))
    rois = [(0, 2, 16, 8, 64, 48), (1, 1, 0, 0, 0, 0), (0, 2, 16, 8, 64, 48)]
    t = dec.frames_tensor(0, size=size, csc=BT601, rois=rois, letterbox=True)  # uint8: K9 without a mapping
    assert t.dtype == torch.uint8 and tuple(t.shape) == (3, 3, 32, 32)
    wr = [want(a, [2], (16, 8, 64, 48), L, BT601, U8, "rgbp"), want(b, [1], None, L, BT601, U8, "rgbp")]
    assert np.array_equal(bits(t), np.concatenate([wr[0], wr[1], wr[0]]))
    assert tuple(dec.frames_tensor(0, size=size, rois=[], dtype="f32").shape) == (0, 3, 32, 32)
    with pytest.raises(ValueError):
        dec.frames_tensor(0, dtype=torch.float16)  # no size
    with pytest.raises(ValueError):
        dec.frames_tensor(0, size=size, dtype=torch.float16, mean=(0, 0, 0), std=(1, 1, 1), scale=(1, 1, 1))  # both forms
    with pytest.raises(ValueError):
        dec.frames_tensor(0, size=size, dtype=torch.float16, std=(1, 1, 1), bias=(0, 0, 0))
    with pytest.raises(ValueError):
        dec.frames_tensor(0, size=size, mean=(0, 0, 0), std=(1, 1, 1))  # uint8
    with pytest.raises(ValueError):
        dec.frames_tensor(0, size=size, dtype=torch.uint8, std=(1, 1, 1))
    with pytest.raises(H.H264MIError):
        dec.frames_tensor(0, "nv12", size=size, dtype=torch.float16)
    with pytest.raises(H.H264MIError):
        dec.frames_tensor(0, size=size, dtype=torch.uint8, scale=(2, 2, 2))


@pytest.mark.gpu
def test_gpu_c_example_writes_tensors(cases, tmp_path):
    c = cases["16x16"]
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    src = tmp_path / "in.h264"
    src.write_bytes(c.stream)
    dst = tmp_path / "out.f32"
    subprocess.run([os.path.join(ROOT, "examples", "h264mi_decode"), str(src), str(dst), "2", "--tensor", "33x19"], stderr=subprocess.PIPE, check=True, timeout=120)
    s = np.float32(1.0) / np.float32(255.0)  # the example's 1.0f / 255.0f
    want = np.concatenate([tu.elements(c.canvas(f, None, (33, 19), L, BIL, BT601, (114, 114, 114)), F32, (s, s, s), (0, 0, 0), "rgbp") for f in range(3)])
    assert np.array_equal(np.frombuffer(dst.read_bytes(), dtype=np.uint8), want)
