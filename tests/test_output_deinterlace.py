"""Deinterlaced output (K10): derived frames for the output calls K6 .. K9, made on the device.

The yardstick is tests/deintutil.py -- the rule of include/h264mi.h ("Deinterlaced output") in numpy -- applied to the generator's reconstruction,
cropped by spsutil.expected_frames.  A deinterlaced frame is a function of the tight I420 frame, the mode and the parity alone, so every GPU
comparison is an equality; a deinterlaced and converted / scaled / tensor item is cscutil / scaleutil / tensorutil applied to the yardstick's
deinterlaced frame.  The CPU tests pin the yardstick itself against answers worked out by hand, and the pure entry point h264mi_deint_rows against it.
The geometry recipes are those of test_output_convert.py's TABLE under other seeds, plus two field-coded streams of conftest.FIELD_MATRIX."""
import ctypes

import numpy as np
import pytest

import cscutil
import deintutil as du
import scaleutil
import spsutil
import tensorutil as tu
from conftest import FIELD_MATRIX, MATRIX, POC_MATRIX, pictures_of
from test_output_convert import RECTS, TABLE

EINVAL = -1
FIELD, BLEND, EDGE = du.FIELD, du.BLEND, du.EDGE
BT601, BILIN = cscutil.BT601, cscutil.BILINEAR
COMBOS = [(FIELD, 0), (FIELD, 1), (BLEND, 0), (EDGE, 0), (EDGE, 1)]  # every mode x parity the rule allows
# name: (generator recipe, crop) -- the smallest shapes at which K10 can go wrong (what each one is for: test_output_convert.TABLE and the issue's list)
SHAPES = {name: (dict(TABLE[name][0], seed=2301 + i), TABLE[name][1]) for i, name in enumerate(sorted(TABLE))}
SHAPES["field_bottom_first"] = (FIELD_MATRIX["field_bottom_first"], (0, 0, 0, 0))
SHAPES["field_mixed_paff"] = (FIELD_MATRIX["field_mixed_paff"], (0, 0, 0, 0))


class Case:
    def __init__(self, sg, name):
        self.kw, self.crop = SHAPES[name]
        raw, rec, _ = sg.encode(**self.kw)
        W, H = self.kw["width"], self.kw["height"]
        self.stream, self.info = spsutil.recrop(raw, *self.crop) if any(self.crop) else (raw, dict(coded_w=W, coded_h=H))
        self.rect = RECTS[name] if name in RECTS else (0, 0, W, H)
        if any(self.crop):
            assert spsutil.crop_rect(self.info, *self.crop) == self.rect
            self.i420 = spsutil.expected_frames(rec, self.info, *self.crop)
        else:
            self.i420 = rec
        self.w, self.h = self.rect[2:]
        self.n = self.kw["frames"]
        self.pictures = pictures_of(self.kw)
        self.i420.setflags(write=False)
        self._want = {}

    def want(self, mode, parity, frame):
        """The yardstick's deinterlaced frame (computed once and never written to)."""
        key = (mode, parity, frame)
        if key not in self._want:
            v = du.frame(self.i420[frame], self.w, self.h, mode, parity)
            v.setflags(write=False)
            self._want[key] = v
        return self._want[key]


@pytest.fixture(scope="module")
def cases(sg):
    return {name: Case(sg, name) for name in SHAPES}


# ------------------------------------------------------------------------------------------------ CPU


def _col(values, mode, parity):
    return du.plane(np.array(values, np.uint8).reshape(-1, 1), mode, parity, True).reshape(-1).tolist()


def test_field_known_answers():
    """A 1 x 5 column, both parities: kept rows copied, the rest the rounded mean of the rows above and below, the edge rows their one neighbour."""
    col = [10, 20, 40, 80, 160]
    assert _col(col, FIELD, 0) == [10, (10 + 40 + 1) >> 1, 40, (40 + 160 + 1) >> 1, 160] == [10, 25, 40, 100, 160]
    assert _col(col, FIELD, 1) == [20, 20, (20 + 80 + 1) >> 1, 80, 80] == [20, 20, 50, 80, 80]  # row 0: up = dn = 1; row 4: dn = up = 3
    assert _col([10, 21], FIELD, 0) == [10, 10] and _col([10, 21], FIELD, 1) == [21, 21]
    assert _col([77], FIELD, 1) == [77] and _col([77], EDGE, 1) == [77] and _col([77], FIELD, 0) == [77]  # 1 x 1, parity 1: neither row exists


def test_blend_known_answers_one_rounding():
    """(S[y - 1] + 2 S[y] + S[y + 1] + 2) >> 2 with the clamps; row 1 of [0, 0, 1, ...] is 0 -- two chained rounded averages would give 1."""
    assert _col([0, 0, 1, 3, 2], BLEND, 0) == [0, (0 + 0 + 1 + 2) >> 2, (0 + 2 + 3 + 2) >> 2, (1 + 6 + 2 + 2) >> 2, (3 + 4 + 2 + 2) >> 2] == [0, 0, 1, 2, 2]
    chained = (((0 + 0 + 1) >> 1) + ((0 + 1 + 1) >> 1) + 1) >> 1
    assert chained == 1
    assert _col([10, 20, 40, 80, 160], BLEND, 0) == [13, 23, 45, 90, 140]


def test_edge_known_answers():
    """4 x 3 luma patches, parity 0: row 1 from rows 0 and 2.  cost_d = |up[cx(x + d)] - dn[cx(x - d)]| for d = 0, -1, +1, the first strictly smallest."""
    def mid(up, dn, parity=0):
        return du.plane(np.array([up, [1, 2, 3, 4], dn], np.uint8), EDGE, parity, True)[1].tolist()
    # x = 1: costs 200, |50 - 50| = 0, |90 - 7| = 83: d = -1, (50 + 50 + 1) >> 1.  x = 3: 200, 110, then d = +1 with |0 - 50| = 50 (the right clamp on up)
    assert mid([50, 200, 90, 0], [7, 0, 50, 200]) == [29, 50, 200, 25]
    # x = 1: costs 111, 70, |120 - 118| = 2: d = +1, (120 + 118 + 1) >> 1.  x = 0: 118, 121 (the left clamp on up), 108: d = +1 with dn clamped
    assert mid([0, 10, 120, 60], [118, 121, 70, 99]) == [64, 119, 95, 65]
    # x = 1: all three costs are 20, with values 50, 90, 10: the tie falls to d = 0
    assert mid([100, 40, 0, 7], [20, 60, 80, 7]) == [30, 50, 24, 7]
    # kept rows are copied; a missing row at the plane's edge is the row beside it
    p = du.plane(np.array([[50, 200, 90, 0], [1, 2, 3, 4], [7, 0, 50, 200]], np.uint8), EDGE, 1, True)
    assert p.tolist() == [[1, 2, 3, 4]] * 3


def test_invariants():
    rnd = np.random.RandomState(2310)
    for w, h in ((1, 1), (2, 2), (5, 3), (16, 16), (33, 18), (34, 7)):
        f = rnd.randint(0, 256, spsutil.i420_size(w, h)).astype(np.uint8)
        y = cscutil.planes(f, w, h)[0]
        for mode, parity in COMBOS:
            out = du.frame(f, w, h, mode, parity)
            assert out.shape == f.shape and out.dtype == np.uint8
            if mode != BLEND:  # kept rows are unchanged, in every plane
                for a, b in zip(cscutil.planes(f, w, h), cscutil.planes(out, w, h)):
                    assert np.array_equal(a[parity::2], b[parity::2]), (w, h, mode, parity)
            flat = np.full_like(f, 93)  # a constant plane is a fixed point
            assert np.array_equal(du.frame(flat, w, h, mode, parity), flat)
        for parity in (0, 1):
            a, b = du.frame(f, w, h, EDGE, parity), du.frame(f, w, h, FIELD, parity)
            assert np.array_equal(a[w * h:], b[w * h:]), "chroma under EDGE is chroma under FIELD"
            rows = np.repeat(y[:, :1], w, axis=1)  # constant along rows: every direction sees the same two samples
            assert np.array_equal(du.plane(rows, EDGE, parity, True), du.plane(rows, FIELD, parity, True))


def test_deint_rows_equal_the_yardstick(H):
    """h264mi_deint_rows -- the rule as the library states it, no GPU -- for n_rows 1 .. 9, every y, mode and parity."""
    L = H.lib()
    k, u, d = ctypes.c_int32(-9), ctypes.c_int32(-9), ctypes.c_int32(-9)
    out = (ctypes.byref(k), ctypes.byref(u), ctypes.byref(d))
    for n_rows in range(1, 10):
        for y in range(n_rows):
            for mode, parity in COMBOS:
                assert L.h264mi_deint_rows(mode, parity, n_rows, y, *out) == 0, (mode, parity, n_rows, y)
                assert (k.value, u.value, d.value) == du.rows(mode, parity, n_rows, y) == H.deint_rows(mode, parity, n_rows, y), (mode, parity, n_rows, y)
    assert du.rows(FIELD, 1, 1, 0) == (1, 0, 0) and du.rows(FIELD, 1, 5, 0) == (0, 1, 1) and du.rows(EDGE, 0, 5, 3) == (0, 2, 4)
    assert du.rows(BLEND, 0, 5, 0) == (0, 0, 1) and du.rows(BLEND, 0, 5, 4) == (0, 3, 4) and du.rows(FIELD, 0, 4, 3) == (0, 2, 2)
    assert L.h264mi_deint_rows(FIELD, 0, 16384, 16383, *out) == 0 and (k.value, u.value, d.value) == (0, 16382, 16382)
    bad = [(3, 0, 4, 0), (-1, 0, 4, 0), (FIELD, 2, 4, 0), (EDGE, -1, 4, 0), (BLEND, 1, 4, 0), (FIELD, 0, 0, 0), (FIELD, 0, 16385, 0), (FIELD, 0, 4, -1),
           (FIELD, 0, 4, 4), (BLEND, 0, 1, 1)]
    for args in bad:
        assert L.h264mi_deint_rows(*args, *out) == EINVAL, args
        assert du.rows(*args) is None
    for i in range(3):
        ptrs = list(out)
        ptrs[i] = None
        assert L.h264mi_deint_rows(FIELD, 0, 4, 0, *ptrs) == EINVAL


def test_the_pseudo_stream_is_above_every_stream_the_suite_names(H):
    assert H.STREAM_DERIVED == 0x40000000 and H.DEINT_PARITY_FIRST == -1 == du.PARITY_FIRST
    assert (H.DEINT_FIELD, H.DEINT_BLEND, H.DEINT_EDGE) == (FIELD, BLEND, EDGE)


# ------------------------------------------------------------------------------------------------ GPU
D = 0x40000000  # H264MI_STREAM_DERIVED


def _decoder(H, c, streams=1, **kw):
    return H.Decoder(max_streams=streams, max_width=c.info["coded_w"], max_height=c.info["coded_h"], max_frames_per_batch=c.pictures, max_slices_per_frame=1, **kw)


def _read_derived(dec, k, w, h):
    """h264mi_frame_read(crop = 1) of derived frame k into a buffer of exactly the tight size."""
    buf = np.full(spsutil.i420_size(w, h), 0xA5, np.uint8)
    assert dec._L.h264mi_frame_read(dec._h, D, k, 1, buf.ctypes.data, buf.nbytes) == 0
    return buf


def _device_buffer(nbytes):
    import torch
    return torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")


def _filled(buf, nbytes):
    got = buf.cpu().numpy()
    assert (got[nbytes:] == 0xA5).all(), "an output kernel wrote past its destination"
    return got[:nbytes]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_gpu_every_mode_and_parity_equals_the_yardstick(name, cases, H):
    c = cases[name]
    dec = _decoder(H, c)
    try:
        dec.decode([c.stream])
        assert dec.frame_count(0) == c.n
        src = np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(c.n)])
        assert np.array_equal(src, c.i420), "the I420 frames themselves"
        for mode, parity in COMBOS:
            assert dec.deinterlace(mode=mode, items=[(0, f, parity) for f in range(c.n)]) == c.n == dec.frame_count(D)
            for f in range(c.n):
                got, want = _read_derived(dec, f, c.w, c.h), c.want(mode, parity, f)
                assert np.array_equal(got, want), (name, mode, parity, f, int(np.flatnonzero(got != want)[0]))
        # a derived frame reports its source's values
        a, b = dec.frame_info(D, c.n - 1), dec.frame_info(0, c.n - 1)
        assert bytes(a) == bytes(b) and (a.width, a.height, a.crop_x, a.crop_y) == (c.w, c.h) + c.rect[:2]
        assert dec.frame_colour(D, 0) == dec.frame_colour(0, 0) and bytes(dec.frame_fields(D, 1)) == bytes(dec.frame_fields(0, 1))
        # ... and K10 wrote nothing into the frame pool
        assert np.array_equal(np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(c.n)]), c.i420)
    finally:
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["aligned_origin", "left_1", "mono_odd"])
def test_gpu_derived_frames_through_the_output_calls(name, cases, H):
    """The pseudo-stream through K6, K7, K8 and K9: each equals its yardstick applied to the yardstick's deinterlaced frames."""
    c = cases[name]
    w, h, n = c.w, c.h, c.n
    dec = _decoder(H, c)
    try:
        dec.decode([c.stream])
        for mode, parity in ((EDGE, 1), (BLEND, 0)):
            assert dec.deinterlace(mode=mode, items=[(0, f, parity) for f in range(n)]) == n
            frames = [c.want(mode, parity, f) for f in range(n)]
            want = np.concatenate(frames)  # K6
            buf = _device_buffer(want.size)
            assert dec.pack_batch(buf.data_ptr(), want.size, stream=D) == want.size
            dec.sync()
            assert np.array_equal(_filled(buf, want.size), want), (name, mode, "pack")
            want = cscutil.convert_all(frames, w, h, "rgbp", BT601 | BILIN)  # K7: planar RGB, bilinear chroma
            buf = _device_buffer(want.size)
            assert dec.convert_batch(buf.data_ptr(), want.size, "rgbp", BT601 | BILIN, stream=D) == want.size
            dec.sync()
            assert np.array_equal(_filled(buf, want.size), want), (name, mode, "convert")
            ow, oh = 77, 51  # K8: an odd size
            want = scaleutil.scale_convert_all(frames, w, h, ow, oh, scaleutil.BILINEAR, "i420")
            buf = _device_buffer(want.size)
            assert dec.scale_batch(buf.data_ptr(), want.size, "i420", (ow, oh), stream=D) == want.size
            dec.sync()
            assert np.array_equal(_filled(buf, want.size), want), (name, mode, "scale")
            size, region = (48, 40), (2, 2, min(w - 2, 90), min(h - 2, 30))  # K9: a region, letterboxed
            spec = H.tensor_spec(size, "rgbp", "u8", csc=BT601, letterbox=True)
            want = tu.elements(tu.item(frames[1], w, h, region, size, tu.LETTERBOX, scaleutil.BILINEAR, BT601, (114, 114, 114)), tu.U8)
            buf = _device_buffer(want.size)
            assert dec.tensor_items(buf.data_ptr(), want.size, spec, [(D, 1) + region]) == want.size
            dec.sync()
            assert np.array_equal(_filled(buf, want.size), want), (name, mode, "tensor")
        # one frame of the pseudo-stream on its own
        one = spsutil.i420_size(w, h)
        buf = _device_buffer(one)
        assert dec._L.h264mi_frame_pack_device(dec._h, D, 2, buf.data_ptr(), one) == 0
        dec.sync()
        assert np.array_equal(_filled(buf, one), c.want(BLEND, 0, 2))
        assert dec._L.h264mi_frame_pack_device(dec._h, D, n, buf.data_ptr(), one) == EINVAL
    finally:
        dec.close()


def _fields(dec, stream, frame):
    ff = dec.frame_fields(stream, frame)
    return ff.field_coded, ff.first_parity, ff.top_field_order_cnt, ff.bottom_field_order_cnt


def _coded_as_fields(H, stream):
    """Per frame of the stream, in decoding order: coded as two field pictures?  Read from the slice headers (field_pic_flag of the slice that starts
    each picture; one slice group, slices in order) by the host parser; the two fields of a frame follow each other."""
    vs, pics = H.VideoStream(), []
    for nu in H.read_nal_units(stream):
        if nu.Type == 7:
            vs.SPS = H.NewSPS(nu.RBSP())
        elif nu.Type == 8:
            vs.PPS = H.NewPPS(vs.SPS, nu.RBSP())
        elif nu.Type in (1, 5):
            hd = H.NewSliceContext(vs, nu, nu.RBSP()).Slice.Header
            if hd.first_mb_in_slice == 0:
                pics.append(hd.field_pic)
    out, i = [], 0
    while i < len(pics):
        out.append(1 if pics[i] else 0)
        i += 2 if pics[i] else 1
    return out


@pytest.mark.gpu
def test_gpu_frame_fields(sg, cases, H):
    recipes = {"top_first": cases["field_pics"], "bottom_first": cases["field_bottom_first"], "mixed": cases["field_mixed_paff"]}
    for label, c in recipes.items():
        dec = _decoder(H, c)
        try:
            dec.decode([c.stream])
            got = [_fields(dec, 0, f) for f in range(c.n)]
            if label == "mixed":
                want = _coded_as_fields(H, c.stream)
                assert len(want) == c.n and 0 in want and 1 in want, want
                assert [g[0] for g in got] == want
                assert all(g[1] == 0 for g in got)  # top field first, and frame pictures with equal counts
            else:
                assert [g[:2] for g in got] == [(1, 1 if label == "bottom_first" else 0)] * c.n, got
                for f, (fc, first, top, bot) in enumerate(got):
                    assert (bot < top) == bool(first) and top != bot
                    assert dec.frame_info(0, f).pic_order_cnt == min(top, bot)
        finally:
            dec.close()
    for name, want in (("poc_bottom_first", (0, 1)), ("cabac_IPP", (0, 0))):
        kw = (POC_MATRIX if name in POC_MATRIX else MATRIX)[name]
        stream = sg.encode(want_recon=False, **kw)[0]
        dec = H.Decoder(max_streams=1, max_width=kw["width"], max_height=kw["height"], max_frames_per_batch=kw["frames"], max_slices_per_frame=1)
        try:
            dec.decode([stream])
            assert dec.frame_count(0) == kw["frames"]
            n_early = 0
            for f in range(kw["frames"]):
                fc, first, top, bot = _fields(dec, 0, f)
                # (the IDR pictures of poc_bottom_first carry delta_pic_order_cnt_bottom 0 -- 8.2.1 wants Min(top, bottom) = 0 there and the generator sends
                # pic_order_cnt_lsb 0 --, so their counts are equal and the top field is first; every other frame has the earlier bottom field)
                early_bottom = name == "poc_bottom_first" and not dec.frame_info(0, f).idr
                assert (fc, first) == (want if name != "poc_bottom_first" or early_bottom else (0, 0)), (name, f)
                assert (bot < top) if early_bottom else (bot == top), (name, f, top, bot)
                n_early += early_bottom
                assert dec.frame_info(0, f).pic_order_cnt == min(top, bot)
            assert n_early == (kw["frames"] - 2 if name == "poc_bottom_first" else 0)  # frames 0 and 5 are the IDR pictures
        finally:
            dec.close()


@pytest.mark.gpu
def test_gpu_batch_deinterlace_rate_and_first_parity(cases, H):
    c = cases["field_bottom_first"]
    dec = _decoder(H, c)
    try:
        dec.decode([c.stream])
        assert dec.deinterlace(0, "field", rate=1) == c.n  # PARITY_FIRST on a bottom-first stream keeps the odd rows
        for f in range(c.n):
            got = _read_derived(dec, f, c.w, c.h)
            assert np.array_equal(got, c.want(FIELD, 1, f)) and not np.array_equal(got, c.want(FIELD, 0, f))
            assert np.array_equal(cscutil.planes(got, c.w, c.h)[0][1::2], cscutil.planes(c.i420[f], c.w, c.h)[0][1::2])
        assert dec.deinterlace(-1, "edge", rate=2) == 2 * c.n == dec.frame_count(D)  # (first, second) per frame
        bob = [_read_derived(dec, k, c.w, c.h) for k in range(2 * c.n)]
        for f in range(c.n):
            assert np.array_equal(bob[2 * f], c.want(EDGE, 1, f)) and np.array_equal(bob[2 * f + 1], c.want(EDGE, 0, f)), f
        # ... which is the item call spelled out, with H264MI_DEINT_PARITY_FIRST or the parities themselves
        for items in ([(0, f, p) for f in range(c.n) for p in (du.PARITY_FIRST, 0)], [(0, f, p) for f in range(c.n) for p in (1, 0)]):
            assert dec.deinterlace(mode="edge", items=items) == 2 * c.n
            assert all(np.array_equal(_read_derived(dec, k, c.w, c.h), bob[k]) for k in range(2 * c.n))
        assert dec.deinterlace(0, "blend", rate=1) == c.n
        assert np.array_equal(_read_derived(dec, 1, c.w, c.h), c.want(BLEND, 0, 1))
        for args in ((0, BLEND, 2), (0, FIELD, 0), (0, FIELD, 3), (0, 3, 1), (1, FIELD, 1), (-2, FIELD, 1), (D, FIELD, 1)):
            assert dec._L.h264mi_batch_deinterlace(dec._h, *args, None) == EINVAL, args
        assert dec.frame_count(D) == c.n, "a refused call leaves the list as it was"
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_lifetime_errors_memory_and_fence(cases, H):
    c = cases["aligned_origin"]
    L = H.lib()
    pending = H.load_hooks().h264mi_internal_pack_pending
    pending.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]

    def is_pending(dec):
        v = ctypes.c_int32(-1)
        assert pending(dec._h, ctypes.byref(v)) == 0
        return v.value
    slot = c.info["coded_w"] * c.info["coded_h"] * 3 // 2
    assert slot % 256 == 0
    dec = _decoder(H, c)
    try:
        dec.prepare([c.stream])
        dec.execute()
        dec.sync()
        first = np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(c.n)])
        assert np.array_equal(first, c.i420)
        assert dec.frame_count(D) == 0
        before = dec.device_bytes()
        assert dec.deinterlace(mode="field", items=[(0, 0, 0), (0, 2, 1)]) == 2
        assert dec.device_bytes() == before + 2 * slot, "the arena: a frame slot of the coded size per derived frame"
        assert dec.deinterlace(mode="edge", items=[(0, 1, 1), (0, 1, 0)]) == 2  # replaced by a second call
        assert dec.device_bytes() == before + 2 * slot, "an equal call allocates nothing"
        assert np.array_equal(_read_derived(dec, 0, c.w, c.h), c.want(EDGE, 1, 1)) and np.array_equal(_read_derived(dec, 1, c.w, c.h), c.want(EDGE, 0, 1))
        # refused items: nothing is launched and the list stays
        item = H._lib.DeintItem
        for bad, mode in (((D, 0, 0), FIELD), ((0, c.n, 0), FIELD), ((0, -1, 0), FIELD), ((1, 0, 0), FIELD), ((0, 0, 1), BLEND), ((0, 0, -1), BLEND),
                          ((0, 0, 2), EDGE), ((0, 0, -2), FIELD), ((0, 0, 0), 3), ((0, 0, 0), -1)):
            arr = (item * 2)(item(0, 0, 0), item(*bad))
            n = ctypes.c_int32(-7)
            assert L.h264mi_items_deinterlace(dec._h, mode, arr, 2, ctypes.byref(n)) == EINVAL, (bad, mode)
            assert n.value == -7 and dec.frame_count(D) == 2
        assert L.h264mi_items_deinterlace(dec._h, FIELD, None, 1, None) == EINVAL and L.h264mi_items_deinterlace(dec._h, FIELD, None, -1, None) == EINVAL
        assert np.array_equal(_read_derived(dec, 0, c.w, c.h), c.want(EDGE, 1, 1))
        # the accessors that refuse the pseudo-stream
        buf = np.zeros(slot, np.uint8)
        vp, i32 = ctypes.c_void_p(), ctypes.c_int32()
        assert L.h264mi_frame_read(dec._h, D, 0, 0, buf.ctypes.data, buf.nbytes) == EINVAL
        assert L.h264mi_frame_read(dec._h, D, 2, 1, buf.ctypes.data, buf.nbytes) == EINVAL
        assert L.h264mi_frame_device_planes(dec._h, D, 0, ctypes.byref(vp), None, None, None, None, None, None) == EINVAL
        assert L.h264mi_frame_read_mbrecs(dec._h, D, 0, buf.ctypes.data, buf.nbytes) == EINVAL
        assert L.h264mi_frame_read_mbmv1(dec._h, D, 0, buf.ctypes.data, buf.nbytes) == EINVAL
        assert L.h264mi_frame_concealed(dec._h, D, 0, ctypes.byref(i32)) == EINVAL
        assert L.h264mi_stream_output_order(dec._h, D, None, 0, ctypes.byref(i32)) == EINVAL
        assert L.h264mi_stream_status(dec._h, D, ctypes.byref(i32)) == EINVAL and L.h264mi_stream_reset(dec._h, D) == EINVAL
        # n = 0 empties the list
        assert dec.deinterlace(items=[]) == 0 == dec.frame_count(D)
        assert L.h264mi_frame_read(dec._h, D, 0, 1, buf.ctypes.data, buf.nbytes) == EINVAL
        # the next pass waits for a K10 launch before it rewrites the frames K10 reads: the same batch executed again right behind it
        assert dec.deinterlace(0, "blend") == c.n
        assert is_pending(dec) == 1, "the K10 launch is recorded for the next pass to wait for"
        dec.execute()
        assert is_pending(dec) == 0 and dec.frame_count(D) == 0, "the list is empty after execute"
        dec.sync()
        assert np.array_equal(np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(c.n)]), first)
        assert dec.deinterlace(0, "blend") == c.n
        assert np.array_equal(_read_derived(dec, 2, c.w, c.h), c.want(BLEND, 0, 2))
        dec.reset_stream(0)
        assert dec.frame_count(D) == 0
        assert dec.device_bytes() == before + 3 * slot, "the arena grew to the largest call and is kept"
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_frames_tensor_deinterlace(cases, H):
    import torch
    c = cases["field_pics"]
    dec = _decoder(H, c)
    try:
        dec.decode([c.stream])
        t = dec.frames_tensor(0, "rgbp", BT601, deinterlace="field")
        assert t.dtype == torch.uint8 and tuple(t.shape) == (c.n, 3, c.h, c.w)
        assert dec.deinterlace(0, "field", 1) == c.n  # the explicit two-step route
        t2 = dec.frames_tensor(H.STREAM_DERIVED, "rgbp", BT601)
        assert torch.equal(t, t2)
        want = cscutil.convert_all([c.want(FIELD, 0, f) for f in range(c.n)], c.w, c.h, "rgbp", BT601)
        assert np.array_equal(t.cpu().numpy().reshape(-1), want)
        size = (64, 48)
        t = dec.frames_tensor(0, size=size, dtype="f32", csc=BT601, deinterlace="edge", field_rate=True, scale=(0.5, 0.5, 0.5))
        assert tuple(t.shape) == (2 * c.n, 3, 48, 64) and dec.frame_count(H.STREAM_DERIVED) == 2 * c.n
        canvas = tu.item(c.want(EDGE, 1, 1), c.w, c.h, None, size, tu.STRETCH, scaleutil.BILINEAR, BT601, (114, 114, 114))
        assert np.array_equal(t[3].cpu().numpy().reshape(-1).view(np.uint8), tu.elements(canvas, tu.F32, scale=(0.5, 0.5, 0.5)))
        with pytest.raises(ValueError):
            dec.frames_tensor(0, field_rate=True)
        assert torch.equal(dec.frames_tensor(0, "rgbp", BT601), torch.from_numpy(cscutil.convert_all(c.i420, c.w, c.h, "rgbp", BT601).reshape(c.n, 3, c.h, c.w)).cuda())
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_c_example_deinterlaces(cases, tmp_path):
    """examples/h264mi_decode.c --deinterlace MODE [--field-rate]: the derived frames through the I420 read-back and through the RGB conversion."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    c = cases["field_bottom_first"]
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    src = tmp_path / "in.h264"
    src.write_bytes(c.stream)
    first = [c.want(EDGE, 1, f) for f in range(c.n)]                                  # the bottom field comes first in this stream
    bob = [c.want(FIELD, p, f) for f in range(c.n) for p in (1, 0)]
    for flags, want in ((["--deinterlace", "edge"], np.concatenate(first)),
                        (["--deinterlace", "field", "--field-rate"], np.concatenate(bob)),
                        (["--rgb", "--deinterlace", "edge"], cscutil.convert_all(first, c.w, c.h, "rgb24", BT601))):
        dst = tmp_path / "out.bin"
        subprocess.run([os.path.join(root, "examples", "h264mi_decode"), str(src), str(dst), str(c.pictures)] + flags, stderr=subprocess.PIPE, check=True, timeout=120)
        assert np.array_equal(np.frombuffer(dst.read_bytes(), dtype=np.uint8), want), flags
