"""Scaled output (K8): frames resized on the device while they are converted to I420, NV12, RGB24 or planar RGB.

The yardstick is tests/scaleutil.py -- the integer rule of include/h264mi.h ("Scaled output") in numpy, followed by cscutil's conversion of the scaled
frame -- applied to the generator's reconstruction, cropped by spsutil.expected_frames (the standard's formulas).  A scaled frame is a function of the
tight I420 frame, the output size and the filter, so every GPU comparison is an equality.  The CPU tests pin the yardstick itself: known answers worked
out by hand, identities and invariants, the 32-bit bounds of the rule, its distance from real-valued interpolation; and the library's own statement
of the rule (h264mi_scale_taps) against it.  The geometry recipes are those of test_output_convert.py's TABLE under other seeds."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cscutil
import scaleutil
import spsutil
import test_output_convert as toc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ECAPACITY = -1, -3, -7
FMT = {"i420": 0, "nv12": 1, "rgb24": 2, "rgbp": 3}
BIL, AREA = scaleutil.BILINEAR, scaleutil.AREA
BT601, BT709, FULL, BILIN = cscutil.BT601, cscutil.BT709, cscutil.FULL_RANGE, cscutil.BILINEAR
COMBOS = [("i420", 0)] + toc.COMBOS  # I420 and NV12 convert nothing; RGB24 / RGBP under BT.601 limited and BT.709 full, nearest and bilinear chroma

QCIF = dict(toc.IPP, width=176, height=144, profile_idc=77, cabac=1)
# name: (row of toc.TABLE or a recipe of its own, new seed, output sizes) -- the smallest shapes at which K8 can go wrong
ROWS = {
    "16x16": ("16x16", 2906, [(16, 16), (8, 8), (7, 5), (33, 19)]),   # identity; exact 2:1; odd output, chroma 4x3, one-row last pair; upscaling, source
                                                                      # clamps right / bottom, a tail of 1 column after two 16-column items
    "two_by_two": ("two_by_two", 2903, [(5, 3), (1, 1)]),             # chroma 1x1: every clamp meets, the scaler's and K7's bilinear
    "aligned_origin": ("aligned_origin", 2901, [(64, 48)]),           # 160x128 at (32, 16): 16-byte stores, ratios 2.5 and 2.67
    "left_1": ("left_1", 2902, [(50, 37)]),                           # 174x144 at (2, 0): byte path, odd chroma origin
    "mono_odd": ("mono_odd", 2904, [(64, 64)]),                       # 173x137 monochrome: odd source, chroma stays 128
    "field_pics": ("field_pics", 2905, [(86, 58)]),                   # 172x116: frames of two fields
    "qcif": (QCIF, 2907, [(16, 12)]),                                 # 176x144: area with 11- and 12-tap loops
}
SHAPES = [(16, 16, 16, 16), (16, 16, 8, 8), (16, 16, 7, 5), (16, 16, 33, 19), (2, 2, 5, 3), (2, 2, 1, 1), (160, 128, 64, 48), (174, 144, 50, 37),
          (173, 137, 64, 64), (172, 116, 86, 58), (176, 144, 16, 12)]  # (w, h, ow, oh) of the table above


def _downscales(w, h, ow, oh):
    return ow <= w and oh <= h


class Case:
    def __init__(self, sg, name):
        row, seed, self.sizes = ROWS[name]
        if isinstance(row, str):
            kw, self.crop = toc.TABLE[row]
            self.rect = toc.RECTS[row]
        else:
            kw, self.crop, self.rect = row, (0, 0, 0, 0), (0, 0, row["width"], row["height"])
        self.kw = dict(kw, seed=seed)
        raw, rec, _ = sg.encode(**self.kw)
        self.rec = rec  # at coded size
        self.stream, self.info = spsutil.recrop(raw, *self.crop) if any(self.crop) else (raw, dict(coded_w=self.kw["width"], coded_h=self.kw["height"]))
        if any(self.crop):
            assert spsutil.crop_rect(self.info, *self.crop) == self.rect
            self.i420 = spsutil.expected_frames(rec, self.info, *self.crop)
        else:
            self.i420 = rec
        self.w, self.h = self.rect[2:]
        self.pictures = self.kw["frames"] * (2 if self.kw.get("field_pics") else 1)
        self.i420.setflags(write=False)
        self._scaled, self._want = {}, {}

    def want(self, size, filter, fmt, csc=0):
        """The yardstick's frames at `size`, flat, back to back (each scaled frame and each conversion computed once, never written to)."""
        key = (size, filter, fmt, csc)
        if key not in self._want:
            if (size, filter) not in self._scaled:
                self._scaled[(size, filter)] = [scaleutil.scale_i420(f, self.w, self.h, size[0], size[1], filter) for f in self.i420]
            s = self._scaled[(size, filter)]
            v = np.concatenate(s) if fmt == "i420" else np.concatenate([cscutil.convert(f, size[0], size[1], fmt, csc) for f in s])
            v.setflags(write=False)
            self._want[key] = v
        return self._want[key]


@pytest.fixture(scope="module")
def cases(sg):
    made = {}

    class Lazy(dict):
        def __missing__(self, name):
            made[name] = self[name] = Case(sg, name)
            return made[name]
    return Lazy()


# ------------------------------------------------------------------------------------------------ CPU


def test_known_answers_worked_out_by_hand():
    row = np.array([[10, 50, 200, 90]], dtype=np.uint8)
    # 4 -> 2 bilinear: step 2 << 16, positions 0.5 and 2.5: taps {0, 1} and {2, 3} with f = 128: (10 + 50) / 2, (200 + 90) / 2
    assert [scaleutil.taps(BIL, 4, 2, i) for i in range(2)] == [([0, 1], [128, 128]), ([2, 3], [128, 128])]
    assert scaleutil.scale_plane(row, 2, 1, BIL).tolist() == [[30, 145]]
    assert scaleutil.scale_plane(row, 2, 1, AREA).tolist() == [[30, 145]]
    # 3 -> 2 area: weights {2, 1} and {1, 2}, divisor 3: (20 + 50 + 1) / 3 = 23, (50 + 400 + 1) / 3 = 150
    assert [scaleutil.taps(AREA, 3, 2, i) for i in range(2)] == [([0, 1], [2, 1]), ([1, 2], [1, 2])]
    assert scaleutil.scale_plane(row[:, :3], 2, 1, AREA).tolist() == [[23, 150]]
    # 2 -> 5 bilinear: step 26214; positions -19661 (clamped), 6553, 32767, 58981, 85195 (clamped to 1 << 16)
    got = [scaleutil.taps(BIL, 2, 5, i) for i in range(5)]
    assert [t[0][0] for t in got] == [0, 0, 0, 0, 1] and [t[1][1] for t in got] == [0, 25, 127, 230, 0]
    assert got[4] == ([1, 1], [256, 0])  # the far clamp: a twice, weights as they come out
    # the same column scaled vertically: the rule is per axis
    assert scaleutil.scale_plane(row.T, 1, 2, BIL).tolist() == [[30], [145]]


@pytest.mark.parametrize("w,h,ow,oh", SHAPES)
def test_properties_identity_constant_weight_sum(w, h, ow, oh):
    rng = np.random.default_rng(w * 1000 + ow)
    src = rng.integers(0, 256, (h, w), dtype=np.uint8)
    filters = [BIL] + ([AREA] if _downscales(w, h, ow, oh) else [])
    for f in filters:
        assert np.array_equal(scaleutil.scale_plane(src, w, h, f), src), "identity at equal size"
        for v in (0, 77, 255):
            assert (scaleutil.scale_plane(np.full((h, w), v, np.uint8), ow, oh, f) == v).all(), "a constant plane stays constant"
        got = scaleutil.scale_plane(src, ow, oh, f)
        assert got.shape == (oh, ow) and got.dtype == np.uint8
    for n_in, n_out in ((w, ow), (h, oh), ((w + 1) // 2, (ow + 1) // 2), ((h + 1) // 2, (oh + 1) // 2)):
        for i in range(n_out):
            idx, wts = scaleutil.taps(BIL, n_in, n_out, i)
            assert sum(wts) == 256 and len(idx) == 2 and 0 <= idx[0] <= idx[1] < n_in
            if n_out <= n_in:
                idx, wts = scaleutil.taps(AREA, n_in, n_out, i)
                assert sum(wts) == n_in and len(idx) <= -(-n_in // n_out) + 1, "area weights sum to n_in; the tap loop is bounded"
                assert wts == [scaleutil.area_weight(n_in, n_out, i, k) for k in idx]
                assert all(scaleutil.area_weight(n_in, n_out, i, k) == 0 for k in (idx[0] - 1, idx[-1] + 1) if 0 <= k < n_in)


def test_every_intermediate_fits_32_bits_at_the_largest_sizes():
    """Positions at 16384-sample axes, and the area sum at the largest legal product: Python integers, so nothing wraps here."""
    M = scaleutil.MAX
    for n_in, n_out in ((M, M), (M, 1), (1, M), (M - 1, M), (M, M - 1), (1920, 224), (8192, M), (3, M)):
        i_step, lo, hi = scaleutil.limits(BIL, n_in, n_out)
        assert 0 <= i_step < n_in << 16 <= 2 ** 30 and -2 ** 31 <= lo <= hi < 2 ** 31, (n_in, n_out)
        for i in (0, n_out - 1):
            idx, wts = scaleutil.taps(BIL, n_in, n_out, i)
            assert 0 <= idx[0] <= idx[1] <= n_in - 1 and min(wts) >= 0
    assert 65536 * 255 + 32768 < 2 ** 24  # the bilinear sum before its shift: weights 256 x 256
    for n_in, n_out in ((M, M), (M, 1), (M, M - 1), (M - 1, 1), (1920, 224), (M, 5)):
        count, reach = scaleutil.limits(AREA, n_in, n_out)
        assert count <= -(-n_in // n_out) + 1 and reach <= 2 * n_in * n_out <= 2 ** 29 and n_out * n_in + n_in < 2 ** 32, (n_in, n_out)
    # the largest legal area product: the weighted sum of an all-255 plane is 255 w h, and the rounding term (w h) >> 1 is added before the division --
    # so the legal sizes are those with 255 w h + ((w h) >> 1) < 2^32 (255 w h < 2^32 alone would let the rounding term wrap: 16384 x 1028)
    w, h = 16384, 1026
    assert 255 * w * h + ((w * h) >> 1) < 2 ** 32 <= 255 * w * (h + 1) + ((w * (h + 1)) >> 1)
    assert 255 * 16384 * 1028 < 2 ** 32 <= 255 * 16384 * 1028 + ((16384 * 1028) >> 1)
    v = scaleutil.matrix(AREA, h, 1) @ np.full((h, 4), 255, np.int64)  # one column of it: the vertical weights sum to h, the horizontal ones to w
    assert v.max() == 255 * h and v.max() * w + ((w * h) >> 1) < 2 ** 32


@pytest.mark.parametrize("w,h,ow,oh", SHAPES)
def test_bilinear_is_within_two_of_float64(w, h, ow, oh):
    """The integer bilinear result against float64 centre-aligned bilinear interpolation (unrounded).  Two sources of difference besides the final
    rounding (0.5): the position is i * floor(65536 n_in / n_out) + ..., short of the real one by less than n_out / 65536 source samples (< 2^-2 at
    16384, < 0.001 here), and the fraction keeps 8 bits, floored: each axis' weight is off by less than 1/256, which moves a sample by less than
    255 / 256 per axis.  Together below 0.5 + 2 * (255 / 256 + 255 * 0.001) < 3; measured on these shapes with these seeds: 1.48 (174 x 144 -> 50 x 37); with other samples 1.52 has been seen.  The bound: <= 2."""
    rng = np.random.default_rng(h * 1000 + oh)
    src = rng.integers(0, 256, (h, w), dtype=np.uint8)
    d = np.abs(scaleutil.scale_plane(src, ow, oh, BIL).astype(np.float64) - scaleutil.scale_plane_real(src, ow, oh)).max()
    print("bilinear |integer - float64| max", (w, h, ow, oh), d)
    assert d <= 2


TAP_AXES = [(16, 7), (2, 5), (173, 64), (1920, 224), (16384, 1), (1, 16384)]


@pytest.mark.parametrize("n_in,n_out", TAP_AXES)
def test_scale_taps_equal_the_yardstick(n_in, n_out, H):
    """h264mi_scale_taps -- the rule as the library states it, no GPU -- for every index of the axis, both filters where legal."""
    L = H.lib()
    cap = 16384
    first, count, w = ctypes.c_int32(0), ctypes.c_int32(0), (ctypes.c_int32 * cap)()
    for f in [BIL] + ([AREA] if n_out <= n_in else []):
        for i in range(n_out):
            assert L.h264mi_scale_taps(f, n_in, n_out, i, ctypes.byref(first), ctypes.byref(count), w, cap) == 0, (f, i)
            idx, wts = scaleutil.taps(f, n_in, n_out, i)
            assert [min(first.value + t, n_in - 1) for t in range(count.value)] == idx and list(w[:count.value]) == wts, (f, n_in, n_out, i)
        for i in {0, n_out - 1, n_out // 2}:
            assert H.scale_taps("bilinear" if f == BIL else "area", n_in, n_out, i) == scaleutil.taps(f, n_in, n_out, i)


def test_scale_taps_illegal_arguments_and_capacity(H):
    L = H.lib()
    first, count, w = ctypes.c_int32(-5), ctypes.c_int32(-5), (ctypes.c_int32 * 8)(*([77] * 8))
    args = (ctypes.byref(first), ctypes.byref(count), w, 8)
    for f, n_in, n_out, i in ((2, 4, 2, 0), (-1, 4, 2, 0), (BIL, 0, 2, 0), (BIL, 4, 0, 0), (BIL, 16385, 2, 0), (BIL, 4, 16385, 0), (BIL, 4, 2, 2), (BIL, 4, 2, -1),
                              (AREA, 2, 5, 0), (AREA, 16, 7, 7)):
        assert L.h264mi_scale_taps(f, n_in, n_out, i, *args) == EINVAL, (f, n_in, n_out, i)
    assert L.h264mi_scale_taps(BIL, 4, 2, 0, None, ctypes.byref(count), w, 8) == EINVAL
    assert L.h264mi_scale_taps(BIL, 4, 2, 0, ctypes.byref(first), ctypes.byref(count), w, -1) == EINVAL
    assert list(w) == [77] * 8
    assert L.h264mi_scale_taps(AREA, 2, 5, 0, *args) == EINVAL and "scales down" in L.h264mi_last_error_string().decode()
    # a cap that is too small: H264MI_ECAPACITY, first and count set, no weight written
    idx, wts = scaleutil.taps(AREA, 16, 7, 3)
    assert (idx, wts) == ([6, 7, 8, 9], [1, 7, 7, 1])  # [48, 64) over source samples of 7: ceil(16 / 7) + 1 taps
    assert L.h264mi_scale_taps(AREA, 16, 7, 3, ctypes.byref(first), ctypes.byref(count), w, 3) == ECAPACITY
    assert (first.value, count.value) == (6, 4) and list(w) == [77] * 8
    assert L.h264mi_scale_taps(BIL, 16, 7, 3, ctypes.byref(first), ctypes.byref(count), w, 1) == ECAPACITY and count.value == 2 and list(w) == [77] * 8
    assert L.h264mi_scale_taps(AREA, 16, 7, 3, ctypes.byref(first), ctypes.byref(count), w, 4) == 0 and list(w) == wts + [77] * 4
    with pytest.raises(H.H264MIError):
        H.scale_taps("lanczos", 4, 2, 0)


def test_new_entry_points_are_declared_and_exported(H):
    hdr = open(os.path.join(ROOT, "include", "h264mi.h")).read()
    from h264decode_amd import _lib
    for name in ("h264mi_scale_taps", "h264mi_frame_scale_device", "h264mi_batch_scale_device"):
        assert ("int32_t %s(" % name) in hdr and name in _lib.EXPORTS and hasattr(H.lib(), name), name
    assert "h264mi_*" in open(os.path.join(ROOT, "h264decode_amd", "csrc", "exports.map")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "h264decode_amd", "libh264mi.so")], capture_output=True, text=True, check=True).stdout
    assert all((" T " + name) in out for name in ("h264mi_scale_taps", "h264mi_frame_scale_device", "h264mi_batch_scale_device"))
    assert "#define H264MI_SCALE_BILINEAR 0" in hdr and "#define H264MI_SCALE_AREA 1" in hdr


# ------------------------------------------------------------------------------------------------ GPU


def _decoder(H, w, h, pictures, streams=1):
    return H.Decoder(max_streams=streams, max_width=w, max_height=h, max_frames_per_batch=pictures, max_slices_per_frame=1)


def _scaled(dec, want_bytes, fmt, csc, size, filter, stream, shift=0):
    """scale_batch into a device buffer of exactly the expected size (starting `shift` bytes into an aligned allocation) with guard bytes on both
    sides, all 0xA5 before."""
    import torch
    buf = torch.full((64 + want_bytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr() + 48 + shift
    n = dec.scale_batch(base, want_bytes, fmt, size, csc, filter, stream=stream)
    dec.sync()
    got = buf.cpu().numpy()
    assert n == want_bytes
    assert (got[:48 + shift] == 0xA5).all() and (got[48 + shift + want_bytes:] == 0xA5).all(), "K8 wrote outside the destination"
    return got[48 + shift:48 + shift + want_bytes]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROWS))
def test_gpu_scale_geometry_format_filter(name, cases, H):
    import torch
    c = cases[name]
    dec = _decoder(H, c.info["coded_w"], c.info["coded_h"], c.pictures)
    try:
        dec.decode([c.stream])
        assert dec.frame_count(0) == 3
        assert np.array_equal(np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(3)]), c.i420), "the I420 frames themselves"
        for size in c.sizes:
            for filt in [BIL] + ([AREA] if _downscales(c.w, c.h, *size) else []):
                for fmt, csc in COMBOS:
                    want = c.want(size, filt, fmt, csc)
                    assert want.size == 3 * cscutil.output_size(fmt, *size) == 3 * dec.output_size(fmt, *size)
                    got = _scaled(dec, want.size, fmt, csc, size, filt, 0)
                    assert np.array_equal(got, want), (name, size, filt, fmt, csc, int(np.flatnonzero(got != want)[0]))
                    if size == (c.w, c.h):  # the identity: K8 and K7 write the same bytes (I420: the frames themselves)
                        same = c.i420.reshape(-1) if fmt == "i420" else toc._converted(dec, want.size, fmt, csc, 0)
                        assert np.array_equal(got, same), (name, filt, fmt, csc, "identity")
            # an unaligned destination takes the byte path whatever the size; and one frame on its own with its capacity check
            want = c.want(size, BIL, "rgb24", BT709 | FULL | BILIN)
            assert np.array_equal(_scaled(dec, want.size, "rgb24", BT709 | FULL | BILIN, size, BIL, 0, shift=1), want), (name, size, "unaligned")
            one = want.size // 3
            buf = torch.full((one + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            dec.scale_frame(0, 2, buf.data_ptr(), one, "rgb24", size, BT709 | FULL | BILIN, "bilinear")
            dec.sync()
            got = buf.cpu().numpy()
            assert np.array_equal(got[:one], want[2 * one:]) and (got[one:] == 0xA5).all()
            assert dec._L.h264mi_frame_scale_device(dec._h, 0, 2, FMT["rgb24"], BT709, size[0], size[1], BIL, buf.data_ptr(), one - 1) == ECAPACITY
        if name == "mono_odd":
            size = c.sizes[0]
            chroma = c.want(size, BIL, "i420").reshape(3, -1)[:, size[0] * size[1]:]  # (equal to what K8 wrote: compared above)
            assert (chroma == 128).all(), "monochrome: the chroma is 128 and stays 128"
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_one_scale_launch_makes_unlike_streams_uniform(cases, H):
    """Two streams of different display size (176x144 and 2x2) through stream = -1 to 32x24 in one launch: stream-major, decoding order, every frame
    at offset index * output_size; one byte short gives H264MI_ECAPACITY with *bytes set and nothing written."""
    import torch
    a, b = cases["qcif"], cases["two_by_two"]
    size = (32, 24)
    dec = _decoder(H, 176, 144, 3, streams=2)
    try:
        dec.decode([a.stream, b.stream])
        for fmt, csc in (("i420", 0), ("nv12", 0), ("rgb24", BT601 | BILIN), ("rgbp", BT709 | FULL)):
            one = cscutil.output_size(fmt, *size)
            want = np.concatenate([a.want(size, BIL, fmt, csc), b.want(size, BIL, fmt, csc)])
            assert want.size == 6 * one == 6 * dec.output_size(fmt, *size)
            got = _scaled(dec, want.size, fmt, csc, size, BIL, -1)
            for i in range(6):
                assert np.array_equal(got[i * one:(i + 1) * one], want[i * one:(i + 1) * one]), (fmt, "frame", i)
            assert np.array_equal(_scaled(dec, 3 * one, fmt, csc, size, BIL, 1), b.want(size, BIL, fmt, csc)), (fmt, "stream 1")
            assert np.array_equal(_scaled(dec, want.size, fmt, csc, size, BIL, -1, shift=1), want), (fmt, "unaligned destination")
            buf = torch.full((want.size,), 0xA5, dtype=torch.uint8, device="cuda")
            n = ctypes.c_size_t(0)
            assert dec._L.h264mi_batch_scale_device(dec._h, -1, FMT[fmt], csc, size[0], size[1], BIL, buf.data_ptr(), want.size - 1, ctypes.byref(n)) == ECAPACITY
            assert n.value == want.size
            dec.sync()
            assert (buf.cpu().numpy() == 0xA5).all()
        # area: legal for the 176x144 stream alone, illegal for the call over both (the 2x2 frames would be upscaled); nothing written
        buf = torch.full((6 * 32 * 24 * 3,), 0xA5, dtype=torch.uint8, device="cuda")
        n = ctypes.c_size_t(0)
        assert dec._L.h264mi_batch_scale_device(dec._h, -1, FMT["rgbp"], BT601, 32, 24, AREA, buf.data_ptr(), buf.numel(), ctypes.byref(n)) == EINVAL
        dec.sync()
        assert (buf.cpu().numpy() == 0xA5).all()
        want = a.want(size, AREA, "rgbp", BT601)
        assert np.array_equal(_scaled(dec, want.size, "rgbp", BT601, size, AREA, 0), want)
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_scale_auto_resolves_from_the_source_frame(sg, H):
    """AUTO at 88x72 resolves as at full size: from each frame's SPS (m1: BT.709; m6_full: BT.601 full range), never from the output size; m9 is
    H264MI_EUNSUPPORTED with nothing written, and an explicit matrix works on it."""
    import torch
    names = ["m1", "m6_full", "m9"]
    auto = {"m1": BT709, "m6_full": BT601 | FULL, "m9": None}
    cs = [toc.VuiCase(sg, n, 2950 + i) for i, n in enumerate(names)]
    size = (88, 72)
    one = 3 * 88 * 72
    dec = _decoder(H, 176, 144, 3, streams=3)
    try:
        dec.decode([c.stream for c in cs])
        for i, (n, c) in enumerate(zip(names, cs)):
            assert cscutil.resolve_auto(c.colour[0], c.colour[1], 176, 144) == auto[n] == cscutil.resolve_auto(c.colour[0], c.colour[1], 88, 72)
            for fmt, chroma in (("rgbp", 0), ("rgb24", BILIN)):
                if auto[n] is None:
                    buf = torch.full((3 * one,), 0xA5, dtype=torch.uint8, device="cuda")
                    with pytest.raises(H.H264MIError) as ei:
                        dec.scale_batch(buf.data_ptr(), 3 * one, fmt, size, chroma, "bilinear", stream=i)
                    assert ei.value.code == EUNSUPPORTED and "9" in str(ei.value) and "explicit matrix" in str(ei.value)
                    dec.sync()
                    assert (buf.cpu().numpy() == 0xA5).all()
                    want = scaleutil.scale_convert_all(c.i420, 176, 144, 88, 72, BIL, fmt, BT709 | chroma)
                    assert np.array_equal(_scaled(dec, want.size, fmt, BT709 | chroma, size, BIL, i), want), n
                else:
                    want = scaleutil.scale_convert_all(c.i420, 176, 144, 88, 72, BIL, fmt, auto[n] | chroma)
                    assert np.array_equal(_scaled(dec, want.size, fmt, chroma, size, BIL, i), want), (n, fmt)
        buf = torch.full((9 * one,), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(H.H264MIError) as ei:  # all streams at once: the one frame AUTO cannot resolve fails the call
            dec.scale_batch(buf.data_ptr(), 9 * one, "rgbp", size, 0, "area", stream=-1)
        assert ei.value.code == EUNSUPPORTED
        dec.sync()
        assert (buf.cpu().numpy() == 0xA5).all()
        assert dec.scale_batch(buf.data_ptr(), 9 * one, "i420", size, 0, "area", stream=-1) == 9 * 88 * 72 * 3 // 2  # I420 resolves nothing
        dec.sync()
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_scale_illegal_arguments(cases, H):
    import torch
    from h264decode_amd._lib import check
    c = cases["16x16"]
    dec = _decoder(H, 16, 16, 3)
    try:
        dec.decode([c.stream])
        buf = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
        n = ctypes.c_size_t(0)

        def call(fmt, csc, ow, oh, filt):
            return dec._L.h264mi_batch_scale_device(dec._h, 0, fmt, csc, ow, oh, filt, buf.data_ptr(), 4096, ctypes.byref(n))
        bad = [(FMT["rgbp"], BT601, 17, 16, AREA), (FMT["rgbp"], BT601, 16, 17, AREA), (FMT["i420"], 0, 33, 19, AREA),  # area upscaling, either axis
               (FMT["rgbp"], BT601, 0, 8, BIL), (FMT["rgbp"], BT601, 8, 0, BIL), (FMT["rgbp"], BT601, -1, 8, BIL), (FMT["rgbp"], BT601, 16385, 8, BIL),
               (FMT["rgbp"], BT601, 8, 16385, BIL),                                                                          # sizes
               (FMT["rgbp"], BT601, 8, 8, 2), (FMT["rgbp"], BT601, 8, 8, -1),                                                 # filters
               (FMT["i420"], BT601, 8, 8, BIL), (FMT["nv12"], BILIN, 8, 8, BIL), (FMT["rgbp"], FULL, 8, 8, BIL), (FMT["rgb24"], 3, 8, 8, BIL),
               (4, 0, 8, 8, BIL), (-1, 0, 8, 8, BIL)]                                                                         # format / csc pairs
        for args in bad:
            assert call(*args) == EINVAL, args
        assert dec._L.h264mi_frame_scale_device(dec._h, 0, 3, FMT["rgbp"], BT601, 8, 8, BIL, buf.data_ptr(), 4096) == EINVAL  # no such frame
        assert dec._L.h264mi_batch_scale_device(dec._h, 1, FMT["rgbp"], BT601, 8, 8, BIL, buf.data_ptr(), 4096, ctypes.byref(n)) == EINVAL  # no such stream
        with pytest.raises(H.H264MIError):
            dec.scale_batch(buf.data_ptr(), 4096, "rgbp", (8, 8), BT601, "lanczos")
        check(dec._L.h264mi_batch_sync(dec._h))
        assert (buf.cpu().numpy() == 0xA5).all()
        assert call(FMT["rgbp"], BT601, 16, 16, AREA) == 0 and n.value == 3 * 3 * 256  # equal size is not upscaling
        dec.sync()
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_next_batch_waits_for_the_scale_launch(cases, sg, H):
    """scale_batch of batch n, then batch n + 1 -- other streams -- executed at once, no synchronisation in between: the scaled bytes of batch n are
    exact.  What orders the two is the event of the scale launch (last_pack): the hooks build shows it recorded by the call and consumed by the execute."""
    import torch
    c = cases["aligned_origin"]
    size = (64, 48)
    want = c.want(size, BIL, "rgbp", BT601 | BILIN)
    others = [spsutil.recrop(sg.encode(**dict(c.kw, seed=2990 + i))[0], *c.crop)[0] for i in range(3)]
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
            assert dec.scale_batch(bufs[i].data_ptr(), want.size, "rgbp", size, BT601 | BILIN, "bilinear") == want.size
            assert is_pending(dec) == 1, "the scale launch is recorded for the next pass to wait for"
            dec.prepare([others[i]])  # batch n + 1 decodes other samples into the pool while K8 may still read batch n
            dec.execute()
            assert is_pending(dec) == 0
        dec.sync()
        for b in bufs:
            got = b.cpu().numpy()
            assert np.array_equal(got[:want.size], want) and (got[want.size:] == 0xA5).all()
        # the batch executed after the scale launch is bit-exact itself
        dec.prepare([c.stream])
        dec.execute()
        dec.sync()
        assert np.array_equal(np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(3)]), c.i420)
        # a call that launches nothing records nothing
        n = ctypes.c_size_t(0)
        assert dec._L.h264mi_batch_scale_device(dec._h, 0, FMT["rgbp"], BT601, 64, 48, BIL, bufs[0].data_ptr(), 1, ctypes.byref(n)) == ECAPACITY
        assert is_pending(dec) == 0
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_frames_tensor_with_a_size(cases, H):
    import torch
    a, b = cases["qcif"], cases["two_by_two"]
    size = (32, 24)
    dec = _decoder(H, 176, 144, 6, streams=2)
    try:
        dec.decode([a.stream, b.stream])
        both = {key: np.concatenate([a.want(size, BIL, *key), b.want(size, BIL, *key)]) for key in (("rgbp", BT601), ("rgb24", BT709 | FULL | BILIN), ("nv12", 0), ("i420", 0))}
        t = dec.frames_tensor(0, size=size)  # planar RGB, AUTO: no VUI, 176x144 -> BT.601 limited, nearest
        assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (3, 3, 24, 32)
        assert np.array_equal(t.cpu().numpy().reshape(-1), a.want(size, BIL, "rgbp", BT601))
        t = dec.frames_tensor(-1, size=size)  # all streams: unlike display sizes, one tensor
        assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (6, 3, 24, 32) and np.array_equal(t.cpu().numpy().reshape(-1), both[("rgbp", BT601)])
        t = dec.frames_tensor(-1, "rgb24", BT709 | FULL | BILIN, size=size)
        assert tuple(t.shape) == (6, 24, 32, 3) and np.array_equal(t.cpu().numpy().reshape(-1), both[("rgb24", BT709 | FULL | BILIN)])
        for fmt in ("nv12", "i420"):
            t = dec.frames_tensor(-1, fmt, size=size)
            assert tuple(t.shape) == (6, cscutil.output_size(fmt, *size)) and np.array_equal(t.cpu().numpy().reshape(-1), both[(fmt, 0)])
        t = dec.frames_tensor(0, "rgbp", BT601, size=size, filter="area")
        assert tuple(t.shape) == (3, 3, 24, 32) and np.array_equal(t.cpu().numpy().reshape(-1), a.want(size, AREA, "rgbp", BT601))
        # a crop change inside the stream: with a size the frames make one tensor; without one they still do not
        l1 = cases["left_1"]
        second, info = spsutil.recrop(l1.stream, 3, 5, 7, 2)
        dec.decode([l1.stream + second])
        assert dec.frame_count(0) == 6
        t = dec.frames_tensor(0, "i420", size=(50, 37))
        rect = spsutil.crop_rect(info, 3, 5, 7, 2)
        assert tuple(t.shape) == (6, cscutil.output_size("i420", 50, 37))
        got = t.cpu().numpy()
        assert np.array_equal(got[:3].reshape(-1), l1.want((50, 37), BIL, "i420"))
        tight = spsutil.expected_frames(l1.rec, info, 3, 5, 7, 2)
        assert np.array_equal(got[3:].reshape(-1), scaleutil.scale_convert_all(tight, rect[2], rect[3], 50, 37, BIL, "i420"))
        with pytest.raises(ValueError):
            dec.frames_tensor(0)
        with pytest.raises(ValueError):
            dec.frames_tensor(0, size=None)
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_c_example_scales(cases, tmp_path):
    c = cases["16x16"]
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    src = tmp_path / "in.h264"
    src.write_bytes(c.stream)
    exe = os.path.join(ROOT, "examples", "h264mi_decode")
    for flags, filt, fmt, csc in ((["--scale", "8x8"], BIL, "i420", 0), (["--scale", "8x8:area"], AREA, "i420", 0), (["--rgb", "--scale", "8x8"], BIL, "rgb24", BT601),
                                  (["--nv12", "--scale", "8x8:area"], AREA, "nv12", 0)):
        dst = tmp_path / ("out" + "".join(flags).replace(":", "_"))
        subprocess.run([exe, str(src), str(dst), "2"] + flags, stderr=subprocess.PIPE, check=True, timeout=120)
        assert np.array_equal(np.frombuffer(dst.read_bytes(), dtype=np.uint8), c.want((8, 8), filt, fmt, csc)), flags
