"""Output formats (K7): NV12, RGB24 and planar RGB of decoded frames, converted on the device.

The yardstick is tests/cscutil.py -- the integer rule of include/h264mi.h in numpy -- applied to the generator's reconstruction, cropped by
spsutil.expected_frames (the standard's formulas).  A converted frame is a function of the tight I420 frame alone, so every GPU comparison is an
equality.  The CPU tests pin the yardstick itself: its coefficients against the header's and the kernel's tables, its integer results against the
real-valued formula, its bilinear upsampling against values worked out by hand; and the two pure entry points of the library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cscutil
import spsutil
import vuiutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ECAPACITY = -1, -3, -7
FMT = {"i420": 0, "nv12": 1, "rgb24": 2, "rgbp": 3}
BT601, BT709, FULL, BILIN = cscutil.BT601, cscutil.BT709, cscutil.FULL_RANGE, cscutil.BILINEAR
# (format, csc) of every geometry row: BT.601 limited and BT.709 full, nearest and bilinear, in both RGB layouts; NV12 converts nothing
COMBOS = [("nv12", 0)] + [(f, m | c) for f in ("rgb24", "rgbp") for m in (BT601, BT709 | FULL) for c in (0, BILIN)]

IPP = dict(frames=3, idr_period=0)
# name: (generator recipe at coded size, (left, right, top, bottom) for the SPS) -- the smallest shapes at which K7 can go wrong
TABLE = {
    "aligned_origin": (dict(IPP, width=192, height=144, profile_idc=77, cabac=1, seed=1901), (16, 0, 8, 0)),  # origin (32, 16), 160 wide: the 16-byte path
    "left_1": (dict(IPP, width=176, height=144, profile_idc=66, cabac=0, seed=1902), (1, 0, 0, 0)),           # 174 wide: byte path, chroma origin 1
    "two_by_two": (dict(IPP, width=16, height=16, profile_idc=77, cabac=1, seed=1903), (7, 0, 7, 0)),         # 2x2, chroma 1x1: both bilinear clamps meet
    "mono_odd": (dict(IPP, width=176, height=144, profile_idc=100, mono=1, cabac=1, transform8x8=1, seed=1904), (1, 2, 3, 4)),  # 173x137
    "field_pics": (dict(IPP, width=176, height=128, profile_idc=77, cabac=0, field_pics=1, num_ref_frames=2, seed=1905), (0, 2, 2, 1)),  # 172x116
    "16x16": (dict(IPP, width=16, height=16, profile_idc=77, cabac=1, seed=1906), (0, 0, 0, 0)),
}
RECTS = {"aligned_origin": (32, 16, 160, 128), "left_1": (2, 0, 174, 144), "two_by_two": (14, 14, 2, 2), "mono_odd": (1, 3, 173, 137),
         "field_pics": (0, 8, 172, 116), "16x16": (0, 0, 16, 16)}
# AUTO from the stream: name -> (video_full_range_flag, matrix_coefficients or None; "plain": no VUI at all), all 176x144
VUI = {"m1": (0, 1), "m6_full": (1, 6), "plain": None, "m9": (0, 9), "full_nodesc": (1, None)}


class Case:
    def __init__(self, sg, name):
        self.kw, self.crop = TABLE[name]
        raw, rec, _ = sg.encode(**self.kw)
        self.stream, self.info = spsutil.recrop(raw, *self.crop) if any(self.crop) else (raw, dict(coded_w=self.kw["width"], coded_h=self.kw["height"]))
        self.rect = RECTS[name]
        if any(self.crop):
            assert spsutil.crop_rect(self.info, *self.crop) == self.rect
            self.i420 = spsutil.expected_frames(rec, self.info, *self.crop)
        else:
            self.i420 = rec
        self.w, self.h = self.rect[2:]
        self.pictures = self.kw["frames"] * (2 if self.kw.get("field_pics") else 1)
        self.i420.setflags(write=False)
        self._want = {}

    def want(self, fmt, csc=0):
        """The yardstick's frames, flat, back to back (computed once per (fmt, csc) and never written to)."""
        if (fmt, csc) not in self._want:
            v = cscutil.convert_all(self.i420, self.w, self.h, fmt, csc)
            v.setflags(write=False)
            self._want[(fmt, csc)] = v
        return self._want[(fmt, csc)]


@pytest.fixture(scope="module")
def cases(sg):
    return {name: Case(sg, name) for name in TABLE}


class VuiCase:
    def __init__(self, sg, name, seed):
        raw, rec, _ = sg.encode(**dict(IPP, width=176, height=144, profile_idc=77, cabac=1, seed=seed))
        self.stream = raw if VUI[name] is None else vuiutil.with_video_signal_type(raw, *VUI[name])
        self.i420, self.w, self.h = rec, 176, 144
        self.i420.setflags(write=False)
        self.colour = (2, 0) if VUI[name] is None else (2 if VUI[name][1] is None else VUI[name][1], VUI[name][0])  # what frame_colour must report


@pytest.fixture(scope="module")
def vui_cases(sg):
    return {name: VuiCase(sg, name, 1950 + i) for i, name in enumerate(sorted(VUI))}


# ------------------------------------------------------------------------------------------------ CPU


def _table_rows(path, anchor):
    text = open(path).read()
    text = text[text.index(anchor):]
    rows = re.findall(r"\{\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\s*\}", text)[:4]
    return [tuple(int(v) for v in r) for r in rows]


def test_coefficient_tables_are_the_roundings_of_kr_kb():
    """The header's and the kernel's tables (read as text) against 8192 x the real coefficients, recomputed from Kr, Kb in float64."""
    want = [cscutil.coefficients(m, f) for m in (BT601, BT709) for f in (False, True)]
    assert want[0] == (9539, 13075, 3209, 6660, 16525)  # BT.601 limited: 1.1644, 1.5960, 0.3918, 0.8130, 2.0172 in 1/8192
    assert _table_rows(os.path.join(ROOT, "include", "h264mi.h"), "#define H264MI_CSC_COEFFS") == want
    assert _table_rows(os.path.join(ROOT, "h264decode_amd", "csrc", "k_output_rule.h"), "k_csc_coeffs[4][5]") == want


@pytest.mark.parametrize("matrix", [BT601, BT709])
@pytest.mark.parametrize("full", [False, True])
def test_integer_rule_is_within_one_of_the_real_formula(matrix, full):
    """Every (Y, Cb, Cr) of 0..255^3: the integer result differs from the float64 formula, rounded half up and clipped, by at most 1.  (Coefficient
    rounding moves a component by at most (255 + 128 + 128) * 0.5 / 8192 = 0.03, so the two roundings can fall on different sides of a half, no more.)"""
    cb, cr = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32), indexing="ij")
    worst = 0
    for y0 in range(0, 256, 16):  # chunks of 16 luma values: 1 M triples at a time
        y = np.arange(y0, y0 + 16, dtype=np.int32)[:, None, None] + np.zeros_like(cb)[None]
        a = cscutil.ycc_to_rgb(y, cb[None] + 0 * y, cr[None] + 0 * y, matrix, full).astype(np.int32)
        b = cscutil.ycc_to_rgb_real(y, cb[None] + 0 * y, cr[None] + 0 * y, matrix, full).astype(np.int32)
        worst = max(worst, int(np.abs(a - b).max()))
    assert worst <= 1


def test_bilinear_known_answers():
    """A 4x4 frame over the 2x2 chroma plane [[10, 50], [200, 90]], worked out by hand from the rule: Hrow = 2 C[k] (even x) or C[k] + C[min(k + 1, 1)]
    (odd x); (3 Hrow(j) + Hrow(j') + 4) >> 3 with j' = max(j - 1, 0) (even y) or min(j + 1, 1) (odd y)."""
    c = np.array([[10, 50], [200, 90]], dtype=np.uint8)
    up = cscutil.upsample_bilinear(c, 4, 4)
    assert up.shape == (4, 4)
    # corners: both clamps give the sample itself ((8 c + 4) >> 3)
    assert (up[0, 0], up[0, 3], up[3, 0], up[3, 3]) == (10, 50, 200, 90)
    assert up[0, 1] == (4 * (10 + 50) + 4) >> 3 == 30               # odd x, even y with the row clamp
    assert up[1, 2] == (3 * 2 * 50 + 2 * 90 + 4) >> 3 == 60         # even x (k = 1), odd y: rows 0 and 1, 60.5 floors
    assert up[2, 1] == (3 * (200 + 90) + (10 + 50) + 4) >> 3 == 116  # odd x, even y: rows 1 and 0
    assert up[1, 1] == (3 * (10 + 50) + (200 + 90) + 4) >> 3 == 59   # odd x, odd y
    assert up[2, 2] == (3 * 2 * 90 + 2 * 50 + 4) >> 3 == 80          # even x, even y
    assert np.array_equal(cscutil.upsample_nearest(c, 4, 4), np.array([[10, 10, 50, 50]] * 2 + [[200, 200, 90, 90]] * 2))
    for w, h in ((4, 4), (5, 3), (2, 2), (1, 1), (7, 6)):  # a flat plane stays flat, odd sizes included
        flat = np.full(((h + 1) // 2, (w + 1) // 2), 77, dtype=np.uint8)
        assert (cscutil.upsample_bilinear(flat, w, h) == 77).all() and cscutil.upsample_bilinear(flat, w, h).shape == (h, w)
    # ... and a grey frame is grey in RGB: Y = 126 -> round(110 * 255 / 219) = 128 limited, 126 full
    grey = np.concatenate([np.full(16, 126, np.uint8), np.full(8, 128, np.uint8)])
    assert (cscutil.to_rgb(grey, 4, 4, BT601 | BILIN) == 128).all() and (cscutil.to_rgb(grey, 4, 4, BT709 | FULL) == 126).all()


def test_output_size_and_csc_resolve(H):
    """The two pure entry points, through the product library, without a GPU."""
    L = H.lib()
    n = ctypes.c_size_t(0)
    for w, h in ((2, 2), (173, 137), (1920, 1080)):
        i420 = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
        for fmt, want in (("i420", i420), ("nv12", i420), ("rgb24", 3 * w * h), ("rgbp", 3 * w * h)):
            assert L.h264mi_output_size(FMT[fmt], w, h, ctypes.byref(n)) == 0 and n.value == want == cscutil.output_size(fmt, w, h), (fmt, w, h)
            assert H.Decoder.output_size(fmt, w, h) == want
    assert (cscutil.output_size("nv12", 2, 2), cscutil.output_size("rgbp", 173, 137), cscutil.output_size("i420", 1920, 1080)) == (6, 71103, 3110400)
    for bad in (-1, 4, 99):
        assert L.h264mi_output_size(bad, 16, 16, ctypes.byref(n)) == EINVAL
    assert L.h264mi_output_size(1, 0, 16, ctypes.byref(n)) == EINVAL

    r = ctypes.c_int32(-99)

    def resolve(csc, mc, full, w, h):
        r.value = -99
        return L.h264mi_csc_resolve(csc, mc, full, w, h, ctypes.byref(r)), r.value
    # AUTO: (matrix_coefficients, video_full_range, width, height) -> resolved
    auto = [((1, 0, 176, 144), BT709), ((1, 1, 176, 144), BT709 | FULL), ((5, 0, 1920, 1080), BT601), ((6, 1, 1920, 1080), BT601 | FULL),
            ((2, 0, 1280, 720), BT709), ((2, 0, 720, 576), BT601), ((2, 0, 1279, 576), BT601), ((2, 0, 704, 577), BT709), ((2, 1, 1920, 1080), BT709 | FULL)]
    for args, want in auto:
        assert resolve(0, *args) == (0, want), args
        assert resolve(BILIN, *args) == (0, want | BILIN), args
        assert cscutil.resolve_auto(*args) == want
    for mc in (0, 9, 4, 7, 8, 3, 255):
        code, _ = resolve(0, mc, 0, 1920, 1080)
        assert code == EUNSUPPORTED, mc
        msg = L.h264mi_last_error_string().decode()
        assert str(mc) in msg and "explicit matrix" in msg, msg
        assert cscutil.resolve_auto(mc, 0, 1920, 1080) is None
        assert resolve(BT709, mc, 1, 16, 16) == (0, BT709)  # an explicit matrix never looks at the stream
    assert resolve(BT601 | FULL | BILIN, 9, 0, 16, 16) == (0, BT601 | FULL | BILIN)
    for bad in (FULL, FULL | BILIN, 3, 15, 64, 8 | BT601, -1, 1 << 20):  # FULL_RANGE with AUTO; unknown matrices and bits
        assert resolve(bad, 1, 0, 16, 16)[0] == EINVAL, bad


@pytest.mark.parametrize("name", sorted(n for n in VUI if VUI[n] is not None))
def test_vui_rewrite_is_seen_by_the_parser_and_changes_no_pixel(name, vui_cases, H, oracle_mod):
    c = vui_cases[name]
    full, matrix = VUI[name]
    (rbsp,) = spsutil.sps_rbsps(c.stream)
    sps = H.NewSPS(rbsp)
    assert (sps.VuiParametersPresent, sps.VideoSignalTypePresent, sps.VideoFormat, sps.VideoFullRange) == (1, 1, 5, full)
    assert sps.ColorDescriptionPresent == (0 if matrix is None else 1)
    if matrix is not None:
        assert (sps.ColorPrimaries, sps.TransferCharacteristics, sps.MatrixCoefficients) == (2, 2, matrix)
    assert (sps.AspectRatioInfoPresent, sps.OverscanInfoPresent, sps.ChromaLocInfoPresent, sps.TimingInfoPresent, sps.NalHrdParametersPresent,
            sps.VclHrdParametersPresent, sps.PicStructPresent, sps.BitstreamRestriction) == (0,) * 8
    assert (sps.width, sps.height) == (176, 144)
    out, info = oracle_mod.decode(c.stream, crop=True)
    assert (info.width, info.height) == (176, 144) and np.array_equal(out, c.i420)


# ------------------------------------------------------------------------------------------------ GPU


def _decoder(H, w, h, pictures, streams=1):
    return H.Decoder(max_streams=streams, max_width=w, max_height=h, max_frames_per_batch=pictures, max_slices_per_frame=1)


def _converted(dec, want_bytes, fmt, csc, stream, shift=0):
    """convert_batch into a device buffer of exactly the expected size (starting `shift` bytes into an aligned allocation) with guard bytes on both
    sides, all 0xA5 before."""
    import torch
    buf = torch.full((64 + want_bytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr() + 48 + shift
    n = dec.convert_batch(base, want_bytes, fmt, csc, stream=stream)
    dec.sync()
    got = buf.cpu().numpy()
    assert n == want_bytes
    assert (got[:48 + shift] == 0xA5).all() and (got[48 + shift + want_bytes:] == 0xA5).all(), "K7 wrote outside the destination"
    return got[48 + shift:48 + shift + want_bytes]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLE))
def test_gpu_geometry_format_colour(name, cases, H):
    import torch
    from h264decode_amd._lib import check
    c = cases[name]
    dec = _decoder(H, c.info["coded_w"], c.info["coded_h"], c.pictures)
    try:
        dec.decode([c.stream])
        assert dec.frame_count(0) == 3
        assert np.array_equal(np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(3)]), c.i420), "the I420 frames themselves"
        for fmt, csc in COMBOS:
            want = c.want(fmt, csc)
            assert want.size == 3 * cscutil.output_size(fmt, c.w, c.h) == 3 * dec.output_size(fmt, c.w, c.h)
            got = _converted(dec, want.size, fmt, csc, 0)
            assert np.array_equal(got, want), (name, fmt, csc, int(np.flatnonzero(got != want)[0]))
        # one frame on its own, and its capacity check (before anything is launched)
        one = cscutil.output_size("rgb24", c.w, c.h)
        buf = torch.full((one + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        dec.convert_frame(0, 2, buf.data_ptr(), one, "rgb24", BT709 | FULL | BILIN)
        dec.sync()
        got = buf.cpu().numpy()
        assert np.array_equal(got[:one], c.want("rgb24", BT709 | FULL | BILIN)[2 * one:]) and (got[one:] == 0xA5).all()
        assert dec._L.h264mi_frame_convert_device(dec._h, 0, 2, FMT["rgb24"], BT709, buf.data_ptr(), one - 1) == ECAPACITY
        # what the rule refuses: NV12 with a csc, FULL_RANGE with AUTO, unknown formats (I420 is the pack calls' format)
        n = ctypes.c_size_t(0)
        for fmt, csc in ((FMT["nv12"], BT601), (FMT["nv12"], BILIN), (FMT["rgbp"], FULL), (FMT["i420"], 0), (4, 0), (-1, 0), (FMT["rgb24"], 3)):
            assert dec._L.h264mi_batch_convert_device(dec._h, 0, fmt, csc, buf.data_ptr(), one + 64, ctypes.byref(n)) == EINVAL, (fmt, csc)
        assert dec.frame_colour(0, 0) == (2, 0)  # the generator writes no VUI
        check(dec._L.h264mi_batch_sync(dec._h))
        assert (buf.cpu().numpy()[one:] == 0xA5).all()
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_one_convert_launch_over_mixed_geometry(cases, H):
    """Three streams of different geometry in one decoder, converted by ONE K7 launch: the grid is sized for the tallest frame, so the blocks beyond the
    2x2 frame's one row pair must write nothing; the odd-sized frames shift the alignment of every later frame, which decides between the 16-byte and
    the byte path frame by frame."""
    import torch
    rows = ["aligned_origin", "mono_odd", "two_by_two"]
    cs = [cases[r] for r in rows]
    dec = _decoder(H, 192, 144, 3, streams=3)
    try:
        dec.decode([c.stream for c in cs])
        for fmt, csc in (("nv12", 0), ("rgb24", BT601 | BILIN), ("rgbp", BT709 | FULL), ("rgbp", BT601 | BILIN)):
            want = np.concatenate([c.want(fmt, csc) for c in cs])
            assert want.size == sum(3 * dec.output_size(fmt, c.w, c.h) for c in cs)
            assert np.array_equal(_converted(dec, want.size, fmt, csc, -1), want), (fmt, csc, "all streams")
            assert np.array_equal(_converted(dec, cs[1].want(fmt, csc).size, fmt, csc, 1), cs[1].want(fmt, csc)), (fmt, csc, "stream 1")
            assert np.array_equal(_converted(dec, want.size, fmt, csc, -1, shift=1), want), (fmt, csc, "unaligned destination")
            # one byte short: H264MI_ECAPACITY, *bytes still set, nothing written
            buf = torch.full((want.size,), 0xA5, dtype=torch.uint8, device="cuda")
            n = ctypes.c_size_t(0)
            assert dec._L.h264mi_batch_convert_device(dec._h, -1, FMT[fmt], csc, buf.data_ptr(), want.size - 1, ctypes.byref(n)) == ECAPACITY
            assert n.value == want.size
            dec.sync()
            assert (buf.cpu().numpy() == 0xA5).all()
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_auto_resolves_from_each_frames_own_sps(vui_cases, H):
    import torch
    names = ["m1", "m6_full", "plain", "m9", "full_nodesc"]
    auto = {"m1": BT709, "m6_full": BT601 | FULL, "plain": BT601, "m9": None, "full_nodesc": BT601 | FULL}  # 176x144: "unspecified" is BT.601
    cs = [vui_cases[n] for n in names]
    for n, c in zip(names, cs):
        assert cscutil.resolve_auto(c.colour[0], c.colour[1], 176, 144) == auto[n]
    one = 3 * 176 * 144
    dec = _decoder(H, 176, 144, 6, streams=5)
    try:
        dec.decode([c.stream for c in cs])
        for i, (n, c) in enumerate(zip(names, cs)):
            assert [dec.frame_colour(i, f) for f in range(3)] == [c.colour] * 3, n
            for fmt, chroma in (("rgbp", 0), ("rgb24", BILIN)):
                if auto[n] is None:
                    buf = torch.full((3 * one,), 0xA5, dtype=torch.uint8, device="cuda")
                    with pytest.raises(H.H264MIError) as ei:
                        dec.convert_batch(buf.data_ptr(), 3 * one, fmt, chroma, stream=i)
                    assert ei.value.code == EUNSUPPORTED and "9" in str(ei.value) and "explicit matrix" in str(ei.value)
                    dec.sync()
                    assert (buf.cpu().numpy() == 0xA5).all()
                    want = cscutil.convert_all(c.i420, 176, 144, fmt, BT709 | chroma)  # ... while an explicit matrix works
                    assert np.array_equal(_converted(dec, want.size, fmt, BT709 | chroma, i), want), n
                else:
                    want = cscutil.convert_all(c.i420, 176, 144, fmt, auto[n] | chroma)
                    assert np.array_equal(_converted(dec, want.size, fmt, chroma, i), want), (n, fmt)
        # all streams at once: the one frame AUTO cannot resolve fails the call, nothing is written
        buf = torch.full((15 * one,), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(H.H264MIError) as ei:
            dec.convert_batch(buf.data_ptr(), 15 * one, "rgbp", 0, stream=-1)
        assert ei.value.code == EUNSUPPORTED
        dec.sync()
        assert (buf.cpu().numpy() == 0xA5).all()
        assert dec.convert_batch(buf.data_ptr(), 15 * one, "nv12", 0, stream=-1) == 15 * 176 * 144 * 3 // 2  # NV12 resolves nothing
        dec.sync()
        # two streams with different VUI in one chunk of one stream (second IDR picture, new SPS): every frame by its own SPS
        a, b = vui_cases["m1"], vui_cases["m6_full"]
        dec.decode([a.stream + b.stream])
        assert dec.frame_count(0) == 6
        assert [dec.frame_colour(0, f) for f in range(6)] == [a.colour] * 3 + [b.colour] * 3
        want = np.concatenate([cscutil.convert_all(a.i420, 176, 144, "rgbp", BT709 | BILIN), cscutil.convert_all(b.i420, 176, 144, "rgbp", BT601 | FULL | BILIN)])
        assert np.array_equal(_converted(dec, want.size, "rgbp", BILIN, 0), want)
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_next_batch_waits_for_the_conversion(cases, sg, H):
    """convert_batch of batch n, then batch n + 1 -- other streams, so the frame pool ends up with other samples -- executed at once, no
    synchronisation in between, and only then a sync: the converted bytes of batch n are exact.  What orders the two is the event of the convert launch
    (last_pack) the next pass waits for before it rewrites frames: the hooks build shows it recorded by the convert call and consumed by the execute."""
    import torch
    c = cases["aligned_origin"]
    want = c.want("rgbp", BT601 | BILIN)
    others = [spsutil.recrop(sg.encode(**dict(c.kw, seed=1990 + i))[0], *c.crop)[0] for i in range(3)]
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
            assert dec.convert_batch(bufs[i].data_ptr(), want.size, "rgbp", BT601 | BILIN) == want.size
            assert is_pending(dec) == 1, "the convert launch is recorded for the next pass to wait for"
            dec.prepare([others[i]])  # batch n + 1 decodes other samples into the pool while the conversion of batch n may still read it
            dec.execute()
            assert is_pending(dec) == 0
        dec.sync()
        for b in bufs:
            got = b.cpu().numpy()
            assert np.array_equal(got[:want.size], want) and (got[want.size:] == 0xA5).all()
        # a call that launches nothing records nothing
        n = ctypes.c_size_t(0)
        assert dec._L.h264mi_batch_convert_device(dec._h, 0, FMT["rgbp"], BT601, bufs[0].data_ptr(), 1, ctypes.byref(n)) == ECAPACITY
        assert is_pending(dec) == 0
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_frames_tensor(cases, H):
    import torch
    c = cases["aligned_origin"]
    b, m = cases["left_1"], cases["mono_odd"]
    dec = _decoder(H, 192, 144, 6, streams=2)
    try:
        dec.decode([c.stream, m.stream])
        for cc, s in ((c, 0), (m, 1)):
            t = dec.frames_tensor(s)  # planar RGB, AUTO: no VUI, below 1280x720 -> BT.601 limited, nearest
            assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (3, 3, cc.h, cc.w)
            assert np.array_equal(t.cpu().numpy().reshape(-1), cc.want("rgbp", BT601))
            t = dec.frames_tensor(s, "rgb24", BT709 | FULL | BILIN)
            assert tuple(t.shape) == (3, cc.h, cc.w, 3) and np.array_equal(t.cpu().numpy().reshape(-1), cc.want("rgb24", BT709 | FULL | BILIN))
            t = dec.frames_tensor(s, "nv12")
            assert tuple(t.shape) == (3, cscutil.output_size("nv12", cc.w, cc.h)) and np.array_equal(t.cpu().numpy().reshape(-1), cc.want("nv12"))
        # a crop change inside the stream: frames of two display sizes do not make one tensor
        dec.decode([b.stream + spsutil.recrop(b.stream, 3, 5, 7, 2)[0]])
        assert dec.frame_count(0) == 6
        with pytest.raises(ValueError):
            dec.frames_tensor(0)
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_c_example_writes_rgb_and_nv12(cases, tmp_path):
    c = cases["left_1"]
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    src = tmp_path / "in.h264"
    src.write_bytes(c.stream)
    for flag, fmt, csc in (("--rgb", "rgb24", BT601), ("--nv12", "nv12", 0)):
        dst = tmp_path / ("out" + flag)
        subprocess.run([os.path.join(ROOT, "examples", "h264mi_decode"), str(src), str(dst), "2", flag], stderr=subprocess.PIPE, check=True, timeout=120)
        assert np.array_equal(np.frombuffer(dst.read_bytes(), dtype=np.uint8), c.want(fmt, csc)), flag
