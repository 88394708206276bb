"""Motion-adaptive deinterlacing on the device (k_deint_motion): derived frames from a frame and its predecessor, across batch boundaries too.

The yardstick is tests/deintmotionutil.py -- the rule of include/h264mi.h ("Motion-adaptive deinterlacing") in numpy -- applied to the generator's
reconstruction.  A derived frame is a function of the source's tight I420 frame, the predecessor's (or none), the spatial mode and the parity alone, so
every comparison is an equality.  The shapes are those of test_output_deinterlace.SHAPES, the smallest at which K10's structure can go wrong: aligned and
byte paths, odd display sizes, crop origins, monochrome, field-coded.  A derived frame lives in the decoder's own arena, of which only display rectangles
are readable: what a kernel wrote beside its rectangle shows in the rectangles of the frames around it (every frame of a launch is compared after the
launch) and, for the readers of the arena, in the guard region behind the K6 copy of the whole list."""
import os
import subprocess

import numpy as np
import pytest

import concealutil2 as c2
import cscutil
import deintmotionutil as dmu
import deintutil as du
import test_output_deinterlace as tod
from conftest import MATRIX

FIELD, EDGE = du.FIELD, du.EDGE
NONE, HISTORY = dmu.PREV_NONE, dmu.PREV_HISTORY
D = tod.D
BT601 = cscutil.BT601
SHAPES = tod.SHAPES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Case(tod.Case):
    def want_motion(self, mode, parity, frame, prev):
        """The yardstick's frame of `frame` against frame `prev` (None: no predecessor), computed once and never written to."""
        if prev is None:
            return self.want(mode, parity, frame)
        key = (mode, parity, frame, prev)
        if key not in self._want:
            v = dmu.frame(self.i420[frame], self.i420[prev], self.w, self.h, mode, parity)
            v.setflags(write=False)
            self._want[key] = v
        return self._want[key]

    def shows_motion(self, mode, parity):
        """Some frame's result against the frame before it differs from the spatial one in a missing-row sample, and from the weave in one: otherwise
        equality with the yardstick would not tell the three apart."""
        miss = dmu.missing_rows(self.w, self.h, parity)
        pulled = any((self.want_motion(mode, parity, f, f - 1) != self.want(mode, parity, f))[miss].any() for f in range(1, self.n))
        moved = any((self.want_motion(mode, parity, f, f - 1) != self.i420[f])[miss].any() for f in range(1, self.n))
        return pulled and moved


@pytest.fixture(scope="module")
def cases(sg):
    return {name: Case(sg, name) for name in SHAPES}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_shape_shows_motion(name, cases):
    """CPU: the streams the GPU tests use move enough between frames, and are still enough, for the predecessor to matter."""
    for mode in (FIELD, EDGE):
        for parity in (0, 1):
            assert cases[name].shows_motion(mode, parity), (name, mode, parity)


# ------------------------------------------------------------------------------------------------ GPU
def _derived(dec, c):
    return [tod._read_derived(dec, k, c.w, c.h) for k in range(dec.frame_count(D))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_gpu_items_equal_the_yardstick(name, cases, H):
    """Per shape, both spatial modes and parities: every frame against the frame before it in decoding order, against none and against itself, in one
    launch.  The latter two are also the existing yardstick's frame and the source frame."""
    c = cases[name]
    n = c.n
    dec = tod._decoder(H, c)
    try:
        dec.decode([c.stream])
        assert dec.frame_count(0) == n
        assert np.array_equal(np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(n)]), c.i420), "the I420 frames themselves"
        for mode_name, mode in sorted(dmu.MODES.items()):
            for parity in (0, 1):
                assert c.shows_motion(mode, parity), (name, mode, parity)
                prevs = [f - 1 if f else NONE for f in range(n)] + [NONE] * n + list(range(n))
                items = [(0, k % n, parity, p) for k, p in enumerate(prevs)]
                assert dec.deinterlace(mode=mode_name, items=items) == 3 * n == dec.frame_count(D)
                assert [dec.derived_prev(k) for k in range(3 * n)] == prevs
                got = _derived(dec, c)
                want = [c.want_motion(mode, parity, k % n, None if p == NONE else p) for k, p in enumerate(prevs)]
                for k in range(3 * n):
                    assert np.array_equal(got[k], want[k]), (name, mode_name, parity, k, prevs[k], int(np.flatnonzero(got[k] != want[k])[0]))
                for f in range(n):
                    assert np.array_equal(got[n + f], c.want(mode, parity, f)), "no predecessor: the spatial mode's frame"
                    assert np.array_equal(got[2 * n + f], c.i420[f]), "its own predecessor: the source frame"
                flat = np.concatenate(want)  # the whole list through K6, with a guard region behind it
                buf = tod._device_buffer(flat.size)
                assert dec.pack_batch(buf.data_ptr(), flat.size, stream=D) == flat.size
                dec.sync()
                assert np.array_equal(tod._filled(buf, flat.size), flat), (name, mode_name, parity)
        a, b = dec.frame_info(D, n - 1), dec.frame_info(0, n - 1)
        assert bytes(a) == bytes(b), "a derived frame reports its source's values"
        assert np.array_equal(np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(n)]), c.i420), "nothing was written into the frame pool"
    finally:
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["aligned_origin", "left_1"])
def test_gpu_history_across_batches(name, cases, H):
    """One stream decoded whole, and again in two batches with H264MI_DEINT_HISTORY: every derived frame of the two routes is equal.  Without the flag,
    and after reset_stream, the first frame of a batch is its spatial frame instead."""
    c = cases[name]
    n, mode, first = c.n, EDGE, 0
    aus = c2.access_units(c.stream)
    assert len(aus) == n == 3
    a, b = b"".join(aus[:2]), b"".join(aus[2:])
    want = [c.want_motion(mode, p, f, f - 1 if f else None) for f in range(n) for p in (first, 1 - first)]
    assert not np.array_equal(c.want_motion(mode, first, 2, 1), c.want(mode, first, 2)) and not np.array_equal(c.want_motion(mode, first, 0, 1), c.want(mode, first, 0))
    dec = tod._decoder(H, c)
    try:
        pool = dec.device_bytes()
        dec.decode([c.stream])
        assert dec.deinterlace(0, "motion_edge", rate=2, history=True) == 2 * n
        whole = _derived(dec, c)
        assert [dec.derived_prev(k) for k in range(2 * n)] == [NONE, NONE, 0, 0, 1, 1]
        for k in range(2 * n):
            assert np.array_equal(whole[k], want[k]), (name, k)
        slot = (c.info["coded_w"] * c.info["coded_h"] * 3 // 2 + 255) & ~255
        assert dec.device_bytes() == pool + (2 * n + 1) * slot, "the derived frames and one history slot per stream"
        # in two batches, with the flag (a new start: the whole stream's last frame is no predecessor of its first)
        dec.reset_stream(0)
        dec.decode([a])
        assert dec.deinterlace(0, "motion_edge", rate=2, history=True) == 4 and [dec.derived_prev(k) for k in range(4)] == [NONE, NONE, 0, 0]
        parts = _derived(dec, c)
        dec.decode([b])
        assert dec.deinterlace(0, "motion_edge", rate=2, history=True) == 2 and [dec.derived_prev(k) for k in range(2)] == [HISTORY, HISTORY]
        parts += _derived(dec, c)
        for k in range(2 * n):
            assert np.array_equal(parts[k], whole[k]), (name, k)
        assert np.array_equal(dec.read_frame_tight(0, 0, crop=True), c.i420[2])  # (frame 0 of the second batch is frame 2 of the stream)
        # without the flag the first frame of the second batch is its spatial frame
        dec.decode([a])
        assert dec.deinterlace(0, "motion_edge", rate=1) == 2
        dec.decode([b])
        assert dec.deinterlace(0, "motion_edge", rate=1) == 1 and dec.derived_prev(0) == NONE
        assert np.array_equal(tod._read_derived(dec, 0, c.w, c.h), c.want(mode, first, 2))
        # ... and after reset_stream: the history of the batch before is dated right, and yet it is not used
        dec.decode([a])
        assert dec.deinterlace(0, "motion_edge", rate=1, history=True) == 2
        dec.reset_stream(0)
        dec.decode([a])
        assert dec.deinterlace(0, "motion_edge", rate=1, history=True) == 2 and [dec.derived_prev(k) for k in range(2)] == [NONE, 0]
        got = _derived(dec, c)
        assert np.array_equal(got[0], c.want(mode, first, 0)) and np.array_equal(got[1], c.want_motion(mode, first, 1, 0))
        dec.decode([b])  # (the plain case once more: the frames of `a` are the references of `b`)
        assert dec.deinterlace(0, "motion_edge", rate=1, history=True) == 1 and dec.derived_prev(0) == HISTORY
        assert np.array_equal(tod._read_derived(dec, 0, c.w, c.h), c.want_motion(mode, first, 2, 1))
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_two_streams_keep_their_own_history_and_the_launch_is_fenced(cases, H):
    """Two streams of unlike coded size in one decoder, stream = -1, two batches: each stream's first frame of the second batch is pulled from its own
    stream's last frame.  The next pass waits for the launch and the history copies (h264mi_internal_pack_pending)."""
    import ctypes
    pending = H.load_hooks().h264mi_internal_pack_pending
    pending.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]

    def is_pending(dec):
        v = ctypes.c_int32(-1)
        assert pending(dec._h, ctypes.byref(v)) == 0
        return v.value
    cs = [cases["aligned_origin"], cases["left_1"]]  # coded 192 x 144 and 176 x 144
    aus = [c2.access_units(c.stream) for c in cs]
    assert all(len(a) == 3 for a in aus)
    dec = H.Decoder(max_streams=2, max_width=192, max_height=144, max_frames_per_batch=3, max_slices_per_frame=1)
    try:
        dec.decode([b"".join(a[:2]) for a in aus])
        assert dec.deinterlace(-1, "motion", rate=1, history=True) == 4 and [dec.derived_prev(k) for k in range(4)] == [NONE, 0, NONE, 0]  # stream-major
        for i, c in enumerate(cs):
            for f in range(2):
                assert np.array_equal(tod._read_derived(dec, 2 * i + f, c.w, c.h), c.want_motion(FIELD, 0, f, f - 1 if f else None)), (i, f)
        dec.prepare([a[2] for a in aus])
        dec.execute()
        dec.sync()
        assert is_pending(dec) == 0
        assert dec.deinterlace(-1, "motion", rate=1, history=True) == 2 and [dec.derived_prev(k) for k in range(2)] == [HISTORY, HISTORY]
        assert is_pending(dec) == 1, "the launch and the history copies are recorded for the next pass to wait for"
        for i, c in enumerate(cs):
            assert np.array_equal(tod._read_derived(dec, i, c.w, c.h), c.want_motion(FIELD, 0, 2, 1)), i
        # one stream only: the other stream's history is left alone, and ends with the batch that did not renew it
        assert dec.deinterlace(1, "motion", rate=1, history=True) == 1 and dec.derived_prev(0) == NONE, "the same batch again: its own history is no predecessor"
        dec.execute()  # the same batch right behind the launch: the pass waits for it
        assert is_pending(dec) == 0 and dec.frame_count(D) == 0
        dec.sync()
        for i, c in enumerate(cs):
            assert np.array_equal(dec.read_frame_tight(i, 0, crop=True), c.i420[2]), i
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_batch_call_takes_predecessors_by_output_order(sg, H):
    """A stream with B pictures: the predecessor is the frame before in OUTPUT order, which is not the one before in decoding order."""
    kw = MATRIX["b_ibp_cabac"]
    stream, rec, _ = sg.encode(**kw)
    n, w, h = kw["frames"], kw["width"], kw["height"]
    dec = H.Decoder(max_streams=1, max_width=w, max_height=h, max_frames_per_batch=n, max_slices_per_frame=1)
    try:
        dec.decode([stream])
        order = list(dec.output_order(0))
        assert sorted(order) == list(range(n)) and order != list(range(n))
        assert np.array_equal(np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(n)]), rec)
        pred = {order[0]: NONE}
        pred.update({order[i]: order[i - 1] for i in range(1, n)})
        assert dec.deinterlace(0, "motion", rate=1) == n
        assert [dec.derived_prev(f) for f in range(n)] == [pred[f] for f in range(n)]
        differs = 0
        for f in range(n):
            parity = dec.frame_fields(0, f).first_parity
            want = dmu.frame(rec[f], None if pred[f] == NONE else rec[pred[f]], w, h, FIELD, parity)
            assert np.array_equal(tod._read_derived(dec, f, w, h), want), (f, pred[f])
            if f and pred[f] != f - 1:
                differs += not np.array_equal(want, dmu.frame(rec[f], rec[f - 1], w, h, FIELD, parity))
        assert differs, "some frame's result tells output order from decoding order"
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_frames_tensor_motion(cases, H):
    """frames_tensor(deinterlace="motion", ...): K7's yardstick of the yardstick's frames."""
    import torch
    c = cases["field_pics"]
    dec = tod._decoder(H, c)
    try:
        dec.decode([c.stream])
        t = dec.frames_tensor(0, "rgbp", BT601, deinterlace="motion")
        assert t.dtype == torch.uint8 and tuple(t.shape) == (c.n, 3, c.h, c.w)
        frames = [c.want_motion(FIELD, 0, f, f - 1 if f else None) for f in range(c.n)]
        assert np.array_equal(t.cpu().numpy().reshape(-1), cscutil.convert_all(frames, c.w, c.h, "rgbp", BT601))
        assert dec.deinterlace(0, "motion", 1) == c.n  # the explicit two-step route
        assert torch.equal(t, dec.frames_tensor(H.STREAM_DERIVED, "rgbp", BT601))
        t = dec.frames_tensor(0, "rgbp", BT601, deinterlace="motion_edge", field_rate=True, deinterlace_history=True)
        assert tuple(t.shape) == (2 * c.n, 3, c.h, c.w) and dec.derived_prev(0) == NONE and dec.derived_prev(3) == 0
        frames = [c.want_motion(EDGE, p, f, f - 1 if f else None) for f in range(c.n) for p in (0, 1)]
        assert np.array_equal(t.cpu().numpy().reshape(-1), cscutil.convert_all(frames, c.w, c.h, "rgbp", BT601))
        for bad in (dict(deinterlace_history=True), dict(deinterlace="field", deinterlace_history=True)):
            with pytest.raises(ValueError):
                dec.frames_tensor(0, "rgbp", BT601, **bad)
        with pytest.raises(ValueError):
            dec.deinterlace(mode="motion", items=[(0, 0, 0, NONE)], history=True)
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_c_example_deinterlaces_motion(cases, tmp_path):
    """examples/h264mi_decode.c --deinterlace motion | motion-edge: a file decoded in several batches comes out as if decoded in one, because the example
    sets H264MI_DEINT_HISTORY."""
    c = cases["field_bottom_first"]
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    src = tmp_path / "in.h264"
    src.write_bytes(c.stream)
    one = [c.want_motion(FIELD, 1, f, f - 1 if f else None) for f in range(c.n)]  # the bottom field comes first in this stream
    bob = [c.want_motion(EDGE, p, f, f - 1 if f else None) for f in range(c.n) for p in (1, 0)]
    assert not np.array_equal(one[2], c.want(FIELD, 1, 2))
    for per_batch, flags, want in ((c.pictures, ["--deinterlace", "motion"], np.concatenate(one)),
                                   (4, ["--deinterlace", "motion"], np.concatenate(one)),  # two frames (four field pictures) per batch: 2 + 2 + 1
                                   (4, ["--deinterlace", "motion-edge", "--field-rate"], np.concatenate(bob))):
        dst = tmp_path / "out.bin"
        subprocess.run([os.path.join(ROOT, "examples", "h264mi_decode"), str(src), str(dst), str(per_batch)] + flags, stderr=subprocess.PIPE, check=True, timeout=120)
        assert np.array_equal(np.frombuffer(dst.read_bytes(), dtype=np.uint8), want), (per_batch, flags)
