"""JPEG snapshots on the device (K13, k_jpeg): baseline JPEG files of decoded frames and of caller-held I420 frames.

The yardstick is tests/jpegutil.py -- the contract "JPEG snapshots" of include/h264mi.h in numpy / Python -- applied to the generator's reconstruction
(cropped by spsutil.expected_frames) or to crafted frames.  The bytes of an item are a function of the tight I420 frame, of whether the stream is
monochrome and of the spec alone, and all of it is integer arithmetic: every comparison is an equality of bytes.  Every destination is pre-filled
(tod._device_buffer) and has a guard region behind it.  The shapes are the smallest at which the kernel's structure can go wrong: one and several MCUs and
MCU rows, odd and cropped sizes (replicated edges in both planes), monochrome, field-coded frames, intervals that span rows and whose index wraps."""
import io

import numpy as np
import pytest

import jpegutil as ju
import test_output_deinterlace as tod
import vuiutil
from conftest import pictures_of
from test_output_convert import IPP

D = tod.D
QUALITIES = (1, 50, 75, 100)
KEEP, FULL, AUTO = ju.RANGE_KEEP, ju.RANGE_FULL, ju.RANGE_AUTO
SMALL = {"ipp_cavlc_48x32": dict(IPP, width=48, height=32, profile_idc=66, cabac=0, seed=1301),
         "ipp_cabac_48x32": dict(IPP, width=48, height=32, profile_idc=77, cabac=1, seed=1302)}
# of test_output_deinterlace.SHAPES: cropped 174 x 144 with chroma origin 1; cropped, odd and monochrome 173 x 137; cropped to 2 x 2 (a block that is all
# replicated edge); cropped frames of field pairs 172 x 116; PAFF
SHAPED = ["left_1", "mono_odd", "two_by_two", "field_pics", "field_mixed_paff"]


class Small:
    """A 48 x 32 stream of the generator in the shape of tod.Case."""

    def __init__(self, sg, kw):
        self.kw = kw
        self.stream, self.i420, _ = sg.encode(**kw)
        self.w, self.h, self.n, self.pictures = kw["width"], kw["height"], kw["frames"], pictures_of(kw)
        self.info = dict(coded_w=self.w, coded_h=self.h)
        self.i420.setflags(write=False)


@pytest.fixture(scope="module")
def cases(sg):
    out = {name: Small(sg, kw) for name, kw in SMALL.items()}
    out.update({name: tod.Case(sg, name) for name in SHAPED})
    return out


def _mono(c):
    return bool(c.kw.get("mono"))


def _head(n):
    return (16 * n + 255) & ~255


def _run(dec, n, slot, launch):
    """One call into a pre-filled buffer with a guard behind it: (results [n, 4], the slots [n, slot])."""
    total = _head(n) + n * slot
    buf = tod._device_buffer(total)
    assert launch(buf.data_ptr(), total, slot) == total
    dec.sync()
    raw = tod._filled(buf, total)
    return raw[:16 * n].view(np.uint32).reshape(n, 4), raw[_head(n):].reshape(n, slot)


def _files(res, slots):
    assert (res[:, 1] == 0).all(), res
    return [slots[k, :res[k, 0]].tobytes() for k in range(len(res))]


def _slot_for(want):
    return (max(len(f) for f in want) + 15) & ~15


def _first_diff(got, want):
    return next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))


def _check(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, k, len(g), len(w), _first_diff(g, w))


# ------------------------------------------------------------------------------------------------ the crafted set (chosen on the CPU)
def _crafted():
    """(name, planes, w, h, mono, quality, restart_mcus): flat, 0 / 255 checkerboards of blocks, of samples and of half blocks, uniform noise, a ramp."""
    rng = np.random.default_rng(1313)

    def chroma(w, h, v=None):
        cw, ch = (w + 1) // 2, (h + 1) // 2
        return [rng.integers(0, 256, (ch, cw)) for _ in range(2)] if v is None else [np.full((ch, cw), v), np.full((ch, cw), 255 - v)]
    out = []
    out.append(("flat", [np.full((32, 32), 128)] + chroma(32, 32, 128), 32, 32, False, 50, 0))
    y, x = np.mgrid[0:24, 0:40]
    out.append(("block_checkerboard", [((x // 8 + y // 8) % 2) * 255] + chroma(40, 24, 0), 40, 24, False, 100, 0))  # DC differences of category 11
    y, x = np.mgrid[0:19, 0:17]
    out.append(("sample_checkerboard_mono", [((x + y) % 2) * 255], 17, 19, True, 100, 0))  # coefficient 63: no EOB
    y, x = np.mgrid[0:16, 0:32]
    out.append(("half_block_stripes", [((x // 4) % 2) * 255] + chroma(32, 16, 255), 32, 16, False, 100, 0))  # the sign-aligned extreme of row 1 of M: AC category 10
    out.append(("noise_q100_r1", [rng.integers(0, 256, (32, 48))] + chroma(48, 32), 48, 32, False, 100, 1))  # stuffing, pad bits that complete 0xFF
    out.append(("noise_q10_odd", [rng.integers(0, 256, (17, 33))] + chroma(33, 17), 33, 17, False, 10, 0))  # long runs: ZRL
    out.append(("noise_q1_mono", [rng.integers(0, 256, (9, 71))], 71, 9, True, 1, 4))
    y, x = np.mgrid[0:48, 0:64]
    out.append(("ramp_r3", [(3 * x + 2 * y) % 256] + [(x[:24, :32] * 7) % 256, (y[:24, :32] * 9) % 256], 64, 48, False, 75, 3))
    out.append(("rst_wrap_16x160", [rng.integers(0, 256, (160, 16))] + chroma(16, 160), 16, 160, False, 90, 0))  # ten intervals: RST7 is followed by RST0
    out.append(("ramp_48x32_r1", [(5 * x[:32, :48] + y[:32, :48]) % 256] + chroma(48, 32, 90), 48, 32, False, 90, 1))
    out.append(("noise_48x32_r3", [rng.integers(0, 256, (32, 48))] + chroma(48, 32), 48, 32, False, 90, 3))  # an interval per MCU row, named by its length
    out.append(("noise_80x32_r3", [rng.integers(0, 256, (32, 80))] + chroma(80, 32), 80, 32, False, 90, 3))  # 5 MCUs a row: an interval spans rows
    return [(name, ju.i420_of(p), w, h, mono, q, r) for name, p, w, h, mono, q, r in out]


@pytest.fixture(scope="module")
def crafted():
    k = ju.Counters()
    rows = []
    for name, data, w, h, mono, q, r in _crafted():
        want = ju.encode(data, w, h, mono, q, False, r, counters=k)
        rows.append((name, data, w, h, mono, q, r, want))
    return rows, k


def test_the_crafted_set_is_not_a_tame_one(crafted):
    """CPU: over the crafted frames every counter of the yardstick is non-zero -- ZRL codes, stuffed bytes, blocks without EOB, EOB-only blocks, pad bits
    that completed a 0xFF byte, intervals -- and the largest categories are the largest there are: 11 for DC, 10 for AC."""
    rows, k = crafted
    assert k.all_nonzero(), vars(k)
    assert (k.max_dc_cat, k.max_ac_cat) == (11, 10), vars(k)
    files = {r[0]: r[-1] for r in rows}
    assert b"\xff\xd7" in files["rst_wrap_16x160"] and files["rst_wrap_16x160"].count(b"\xff\xd0") >= 2, "the RST index wraps"


# ------------------------------------------------------------------------------------------------ GPU
def _i420_files(dec, data, w, h, mono, q, rng, r, slot=None, want=None):
    import torch
    src = torch.from_numpy(np.ascontiguousarray(data).reshape(1, -1).copy()).cuda()
    torch.cuda.synchronize()
    slot = slot if slot is not None else _slot_for(want)
    res, slots = _run(dec, 1, slot, lambda p, cap, s: dec.jpeg_i420(p, cap, s, src.data_ptr(), w, h, 1, mono, q, rng, r))
    return res, slots


@pytest.fixture(scope="module")
def gpu_dec(H):
    dec = H.Decoder(max_streams=1, max_width=48, max_height=32, max_frames_per_batch=4, max_slices_per_frame=1)
    yield dec
    dec.close()


@pytest.mark.gpu
def test_gpu_crafted_frames_equal_the_yardstick(crafted, gpu_dec):
    rows, _ = crafted
    for name, data, w, h, mono, q, r, want in rows:
        res, slots = _i420_files(gpu_dec, data, w, h, mono, q, KEEP, r, want=[want])
        assert tuple(res[0]) == (len(want), 0, w, h), (name, res)
        _check(_files(res, slots), [want], name)
    name, data, w, h, mono, q, r, _ = rows[7]  # ... and the range rule on a frame that holds every value: the ramp
    want = ju.encode(data, w, h, mono, q, True, r)
    res, slots = _i420_files(gpu_dec, data, w, h, mono, q, FULL, r, want=[want])
    _check(_files(res, slots), [want], name + " full")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SMALL) + SHAPED)
def test_gpu_decoded_frames_equal_the_yardstick(name, cases, H):
    """Every frame of the stream at qualities 1, 50, 75 and 100, the range going round KEEP, FULL, AUTO (a stream without a VUI is limited range: AUTO is
    FULL), and all three at quality 75; batch call and item call."""
    c = cases[name]
    mono = _mono(c)
    dec = tod._decoder(H, c)
    try:
        dec.decode([c.stream])
        assert dec.frame_count(0) == c.n and np.array_equal(np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(c.n)]), c.i420), "the I420 frames themselves"
        combos = [(q, (KEEP, FULL, AUTO)[i % 3]) for i, q in enumerate(QUALITIES)] + [(75, FULL), (75, AUTO)]
        for q, rng in combos:
            want = [ju.encode(c.i420[f], c.w, c.h, mono, q, rng != KEEP, 0) for f in range(c.n)]
            slot = _slot_for(want)
            res, slots = _run(dec, c.n, slot, lambda p, cap, s: dec.jpeg_batch(p, cap, s, 0, q, rng, 0))
            assert [tuple(r) for r in res] == [(len(w), 0, c.w, c.h) for w in want], (name, q, rng, res)
            _check(_files(res, slots), want, (name, q, rng))
        items = [(0, c.n - 1), (0, 0)]
        want = [ju.encode(c.i420[f], c.w, c.h, mono, 50, False, 2) for _, f in items]
        res, slots = _run(dec, 2, _slot_for(want), lambda p, cap, s: dec.jpeg_items(p, cap, s, items, 50, KEEP, 2))
        _check(_files(res, slots), want, (name, "items"))
        assert np.array_equal(np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(c.n)]), c.i420), "nothing was written into the frame pool"
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_auto_keeps_a_full_range_stream(cases, H):
    c = cases["ipp_cabac_48x32"]
    dec = tod._decoder(H, c)
    try:
        dec.decode([vuiutil.with_video_signal_type(c.stream, 1)])
        assert dec.frame_colour(0, 0)[1] == 1
        keep, full = ([ju.encode(c.i420[f], c.w, c.h, False, 75, fr, 0) for f in range(c.n)] for fr in (False, True))
        assert keep != full
        for rng, want in ((AUTO, keep), (KEEP, keep), (FULL, full)):
            res, slots = _run(dec, c.n, _slot_for(want), lambda p, cap, s: dec.jpeg_batch(p, cap, s, -1, 75, rng, 0))
            _check(_files(res, slots), want, rng)
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_derived_frames_are_sources(cases, H):
    c = cases["field_pics"]
    dec = tod._decoder(H, c)
    try:
        dec.decode([c.stream])
        assert dec.deinterlace(mode="field", items=[(0, f, 0) for f in range(c.n)]) == c.n
        want = [ju.encode(c.want(tod.FIELD, 0, f), c.w, c.h, False, 75, True, 0) for f in range(c.n)]
        res, slots = _run(dec, c.n, _slot_for(want), lambda p, cap, s: dec.jpeg_batch(p, cap, s, D, 75, AUTO, 0))
        _check(_files(res, slots), want, "derived")
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_truncation_reports_the_size_and_stays_in_its_slot(crafted, gpu_dec, H):
    import torch
    rows, _ = crafted
    by = {r[0]: r for r in rows}
    _, noise, w, h, _, q, r, big = by["noise_q100_r1"]
    small = ju.encode(by["ramp_48x32_r1"][1], 48, 32, False, q, False, r)
    slot = ((len(big) + 15) & ~15) - 16  # one 16-byte step too small for the noise, enough for the ramp
    assert len(small) + 16 <= slot < len(big)
    for order in ((0, 1, 0), (0, 1), (1, 1, 0)):
        src = torch.from_numpy(np.stack([by["ramp_48x32_r1"][1], noise])[list(order)].copy()).cuda()
        torch.cuda.synchronize()
        res, slots = _run(gpu_dec, len(order), slot, lambda p, cap, s: gpu_dec.jpeg_i420(p, cap, s, src.data_ptr(), w, h, len(order), False, q, KEEP, r))
        for k, which in enumerate(order):
            if which:
                assert tuple(res[k]) == (len(big), ju.TRUNCATED, w, h), (order, k, res)
            else:
                assert tuple(res[k]) == (len(small), 0, w, h) and slots[k, :len(small)].tobytes() == small, (order, k)
                assert (slots[k, len(small):] == 0xA5).all(), "the canary behind a neighbour's file"
    # (behind the last slot: tod._filled, in _run).  The size it asked for fits; bound_bytes never truncates
    res, slots = _i420_files(gpu_dec, noise, w, h, False, q, KEEP, r, slot=(len(big) + 15) & ~15)
    _check(_files(res, slots), [big], "retry")
    hb, bound = H.jpeg_size(w, h, False, q, "keep", r)
    assert hb == ju.header_bytes(False) and bound % 16 == 0 and bound > len(big)
    res, slots = _i420_files(gpu_dec, noise, w, h, False, q, KEEP, r, slot=bound)
    _check(_files(res, slots), [big], "bound")


@pytest.mark.gpu
def test_gpu_forty_items_next_batch_and_the_python_layer(cases, H):
    """40 items with repeats in one call; frames_jpeg (default slot, the retry of truncated items) equals the yardstick; after the next batch's decode a
    second call matches that batch; K8 to I420 at 24 x 14, then JPEG, equals the yardstick of K8's output; Pillow opens a device-made file."""
    from PIL import Image
    a, b = cases["ipp_cavlc_48x32"], cases["ipp_cabac_48x32"]
    dec = tod._decoder(H, a)
    try:
        dec.decode([a.stream])
        items = [(0, (7 * k) % a.n) for k in range(40)]
        want = [ju.encode(a.i420[f], a.w, a.h, False, 75, True, 0) for f in range(a.n)]
        res, slots = _run(dec, 40, _slot_for(want), lambda p, cap, s: dec.jpeg_items(p, cap, s, items, 75, AUTO, 0))
        _check(_files(res, slots), [want[f] for _, f in items], "40 items")
        hi = [ju.encode(a.i420[f], a.w, a.h, False, 100, False, 0) for f in range(a.n)]
        assert max(len(f) for f in hi) > ju.header_bytes(False) + a.w * a.h // 2 + 16, "quality 100 does not fit the default slot: frames_jpeg has to try again"
        _check(dec.frames_jpeg(0, quality=100, range="keep"), hi, "frames_jpeg")
        im = Image.open(io.BytesIO(dec.frames_jpeg(items=[(0, 1)], quality=90)[0]))
        im.load()
        assert im.size == (a.w, a.h) and im.mode == "RGB"
        # the next batch
        dec.decode([b.stream])
        want = [ju.encode(b.i420[f], b.w, b.h, False, 75, True, 0) for f in range(b.n)]
        _check(dec.frames_jpeg(-1, quality=75), want, "the next batch")
        # thumbnails: K8's I420 output is the source
        t = dec.frames_tensor(0, "i420", size=(24, 14), filter="area")
        scaled = t.cpu().numpy()
        want = [ju.encode(scaled[f], 24, 14, False, 75, False, 0) for f in range(b.n)]
        _check(dec.i420_jpeg(t, 24, 14, quality=75), want, "K8 then K13")
        _check(dec.frames_jpeg(0, quality=75, range="keep", size=(24, 14)), want, "frames_jpeg(size=)")
    finally:
        dec.close()
