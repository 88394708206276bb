"""Frame statistics on the device (K12, k_stats): sums, a histogram and differences against a predecessor, per frame and per cell of a grid.

The yardstick is tests/statsutil.py -- the contract "Frame statistics" of include/h264mi.h in numpy on int64 -- applied to the generator's
reconstruction.  The statistics of an item are a function of the source's tight I420 frame, the predecessor's (or none), the cell size and the threshold
alone, and all of it is integer arithmetic, so every comparison is an equality of bytes.  The shapes are those of test_output_deinterlace.SHAPES, the
smallest at which the kernel's structure can go wrong: the 16-byte and the byte path, odd display sizes and partial cells, crop origins, monochrome,
field-coded.  Every destination is pre-filled (tod._device_buffer) and has a guard region behind it: a kernel that adds into a destination nobody cleared,
or writes past its items, fails."""
import os
import re
import subprocess

import numpy as np
import pytest

import concealutil2 as c2
import statsutil as su
from h264decode_amd import STATS_CELL_SAD, STATS_CELL_SUM, STATS_PREV_HISTORY, STATS_PREV_NONE  # (the package's names of the contract's constants)
import test_output_deinterlace as tod
from conftest import MATRIX

D = tod.D
NONE, HISTORY = su.PREV_NONE, su.PREV_HISTORY
assert (NONE, HISTORY, su.CELL_SUM, su.CELL_SAD) == (STATS_PREV_NONE, STATS_PREV_HISTORY, STATS_CELL_SUM, STATS_CELL_SAD)
SHAPES = tod.SHAPES
# |S - P| > THRESH: one threshold at which, in every shape but two_by_two, some samples of every successive pair of frames count and some do not
THRESH = 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Case(tod.Case):
    def item(self, frame, prev, cell=0, planes=0, S=None, P=None):
        """The yardstick's bytes of one item (computed once and never written to); S / P: frames that are not the stream's own (derived ones)."""
        key = ("stats", frame, prev, cell, planes)
        if key not in self._want:
            src = self.i420[frame] if S is None else S
            pre = P if P is not None else (None if prev is None else self.i420[prev])
            v = su.item(src, pre, self.w, self.h, cell, planes, THRESH)
            v.setflags(write=False)
            self._want[key] = v
        return self._want[key]

    def items(self, todo, cell=0, planes=0):
        return np.concatenate([self.item(f, None if p == NONE else p, cell, planes) for _, f, p in todo])


@pytest.fixture(scope="module")
def cases(sg):
    return {name: Case(sg, name) for name in SHAPES}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_shape_has_something_to_measure(name, cases):
    """CPU: in the streams the GPU tests use, successive frames differ (sad_y > 0), some but not all luma samples change by more than THRESH, and the
    luma takes more than one value -- otherwise equality with the yardstick would not tell a difference field from 0, changed_y from 0 or w * h, or the
    histogram from one bin.  two_by_two (four samples, and its last two frames alike) is held to the first two conditions through its first pair of
    frames only, and not to the one on changed_y; every pair of every other shape is held to all of them."""
    c = cases[name]
    recs = [su.parse(c.item(f, f - 1)) for f in range(1, c.n)]
    assert recs[0]["sad_y"] > 0 and recs[0]["sse_y"] > 0
    for f in range(c.n):
        assert np.count_nonzero(su.parse(c.item(f, None))["hist_y"]) >= 2, (name, f)
    if name != "two_by_two":
        for r in recs:
            assert r["sad_y"] > 0 and 0 < r["changed_y"] < c.w * c.h, (name, r["changed_y"])
    assert name == "mono_odd" or any(r["sad_cb"] > 0 and r["sad_cr"] > 0 for r in recs)
    if name == "mono_odd":
        wc, hc = (c.w + 1) // 2, (c.h + 1) // 2
        assert all((r["sum_cb"], r["sum_cr"], r["sad_cb"], r["sad_cr"]) == (128 * wc * hc, 128 * wc * hc, 0, 0) for r in recs), "monochrome: chroma is 128 throughout"


# ------------------------------------------------------------------------------------------------ GPU
def _pool(dec, c):
    return np.stack([dec.read_frame_tight(0, f, crop=True) for f in range(c.n)])


def _launch(dec, buf, total, todo, cell, planes):
    assert dec.stats_items(buf.data_ptr(), total, todo, cell, planes, THRESH) == total
    dec.sync()
    return tod._filled(buf, total)


def _first_diff(got, want):
    return int(np.flatnonzero(got != want)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_gpu_items_equal_the_yardstick(name, cases, H):
    """Per shape, one launch of 3 n items: every frame against the frame before it (decoding order), against none and against itself; without a grid,
    and with both planes at every cell size.  Byte for byte, twice into the same pre-filled buffer, nothing behind it, nothing in the frame pool."""
    c = cases[name]
    n = c.n
    dec = tod._decoder(H, c)
    try:
        dec.decode([c.stream])
        assert dec.frame_count(0) == n and np.array_equal(_pool(dec, c), c.i420), "the I420 frames themselves"
        todo = [(0, f, f - 1 if f else NONE) for f in range(n)] + [(0, f, NONE) for f in range(n)] + [(0, f, f) for f in range(n)]
        for cell, planes in [(0, 0)] + [(cell, 3) for cell in su.CELLS]:
            want = c.items(todo, cell, planes)
            assert want.size == 3 * n * su.item_bytes(c.w, c.h, cell, planes) == 3 * n * H.Decoder.stats_size(c.w, c.h, cell, planes)[2]
            buf = tod._device_buffer(want.size)
            got = _launch(dec, buf, want.size, todo, cell, planes)
            assert np.array_equal(got, want), (name, cell, _first_diff(got, want), _first_diff(got, want) % (want.size // (3 * n)))
            again = _launch(dec, buf, want.size, todo, cell, planes)  # into what the first launch left: the destination is cleared, not added to
            assert np.array_equal(again, want), (name, cell, "second launch", _first_diff(again, want))
        one = su.item_bytes(c.w, c.h, 16, 3)
        for k, (_, f, p) in enumerate(todo):  # (the invariants, on what the device wrote)
            r = su.parse(got[k * su.item_bytes(c.w, c.h, 64, 3):], 3)
            su.check_invariants(r, 3)
            assert r["has_prev"] == (p != NONE) and (r["gw"], r["gh"]) == su.grid_size(c.w, c.h, 64)
        # one plane only, and the other one: what follows the record is the selected plane
        for planes in (1, 2):
            want = c.items(todo[:n], 16, planes)
            assert want.size <= n * one
            got = _launch(dec, tod._device_buffer(want.size), want.size, todo[:n], 16, planes)
            assert np.array_equal(got, want), (name, planes, _first_diff(got, want))
        assert np.array_equal(_pool(dec, c), c.i420), "nothing was written into the frame pool"
    finally:
        dec.close()


class _Plane:
    """A device pointer as torch takes it (no copy)."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def _pool_luma(dec, frame, W, Hc):
    """The coded luma plane of frame `frame` of stream 0 in the frame pool, as a writable torch view [Hc, W]."""
    import ctypes
    import torch
    y = ctypes.c_void_p()
    assert dec._L.h264mi_frame_device_planes(dec._h, 0, frame, ctypes.byref(y), None, None, None, None, None, None) == 0
    return torch.as_tensor(_Plane(y.value, W * Hc), device="cuda").view(Hc, W)


STRIPES = (10, 60, 110, 200)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["aligned_origin", "left_1", "mono_odd"])
def test_gpu_words_a_wavefront_holds_alike(name, cases, H):
    """The histogram counts a word that every active lane of a wavefront holds alike once, with the lane count: in one add where its four bytes are
    alike, in four otherwise.  The generator's frames never get there, so the pool's luma is overwritten: frame 0 flat, frame 1 vertical stripes of
    period 4 (every word of a row alike, its bytes not), frame 2 flat in its upper part and as decoded below.  aligned_origin takes the 16-byte path;
    left_1 and mono_odd the byte path, where the last word of a row is partial (2 and 1 samples), so words that are counted once and words that are
    not mix in one row; wavefronts at the end of a band are partly active in all three.  What the pool then holds is read back and goes through the
    yardstick: byte for byte, with and without predecessors and cells."""
    import torch
    c = cases[name]
    W, Hc = c.info["coded_w"], c.info["coded_h"]
    dec = tod._decoder(H, c)
    try:
        dec.decode([c.stream])
        assert dec.frame_count(0) == c.n == 3
        dec.sync()
        _pool_luma(dec, 0, W, Hc).fill_(119)
        _pool_luma(dec, 1, W, Hc)[:] = torch.tensor(STRIPES, dtype=torch.uint8, device="cuda").repeat(W // 4)
        _pool_luma(dec, 2, W, Hc)[:c.rect[1] + 2 * c.h // 3].fill_(200)
        torch.cuda.synchronize()
        frames = _pool(dec, c)
        ys = [su.planes(f, c.w, c.h)[0] for f in frames]
        assert (ys[0] == 119).all() and sorted(np.unique(ys[1])) == sorted(STRIPES) and (ys[1] == ys[1][:1]).all()
        assert (ys[2][:c.h // 2] == 200).all() and len(np.unique(ys[2])) > 16
        todo = [(0, 0, NONE), (0, 1, NONE), (0, 2, NONE), (0, 1, 0), (0, 2, 1), (0, 0, 2), (0, 0, 0)]
        for cell, planes in ((0, 0), (8, 3), (64, 3)):
            want = np.concatenate([su.item(frames[f], None if p == NONE else frames[p], c.w, c.h, cell, planes, THRESH) for _, f, p in todo])
            got = _launch(dec, tod._device_buffer(want.size), want.size, todo, cell, planes)
            assert np.array_equal(got, want), (name, cell, _first_diff(got, want), _first_diff(got, want) % (want.size // len(todo)))
        one = su.item_bytes(c.w, c.h, 64, 3)
        flat, striped, part = (su.parse(got[k * one:], 3) for k in range(3))
        assert (flat["min_y"], flat["max_y"], flat["hist_y"][119]) == (119, 119, c.w * c.h) and np.count_nonzero(flat["hist_y"]) == 1
        assert (striped["min_y"], striped["max_y"]) == (10, 200) and np.count_nonzero(striped["hist_y"]) == 4 and striped["hist_y"][list(STRIPES)].sum() == c.w * c.h
        assert part["hist_y"][200] >= (c.h // 2) * c.w and part["max_y"] >= 200
        for r in (flat, striped, part):
            su.check_invariants(r, 3)
    finally:
        dec.close()


def _scalars(rec):
    return {k: int(rec[k]) for k in su.U64 + su.U32}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["aligned_origin", "left_1"])
def test_gpu_history_across_batches_and_the_views(name, cases, H):
    """One stream decoded whole, and again in two batches with H264MI_STATS_HISTORY: the records of the two routes are equal.  Without the flag, and after
    reset_stream, the first frame of a batch has no predecessor.  Decoder.frame_stats' views are held to the same records."""
    import torch
    c = cases[name]
    n = c.n
    aus = c2.access_units(c.stream)
    assert len(aus) == n == 3
    a, b = b"".join(aus[:2]), b"".join(aus[2:])
    want = [su.parse(c.item(f, f - 1 if f else None, 32, 3), 3) for f in range(n)]
    dec = tod._decoder(H, c)
    try:
        pool = dec.device_bytes()
        dec.decode([c.stream])
        assert dec.stats_plan(0, history=True) == [(0, f, f - 1 if f else NONE) for f in range(n)]
        whole = dec.frame_stats(0, 32, ("cell_sum", "cell_sad"), THRESH, history=True)
        slot = (c.info["coded_w"] * c.info["coded_h"] * 3 // 2 + 255) & ~255
        assert dec.device_bytes() == pool + slot, "one history slot per stream"
        assert len(whole) == n
        for f, (g, w) in enumerate(zip(whole, want)):
            assert all(g[k].dtype == torch.int64 and g[k].dim() == 0 for k in su.U64) and all(g[k].dtype == torch.int32 and g[k].dim() == 0 for k in su.U32)
            assert _scalars(g) == {k: w[k] for k in su.U64 + su.U32}, (name, f)
            assert g["hist_y"].dtype == torch.int32 and tuple(g["hist_y"].shape) == (256,) and np.array_equal(g["hist_y"].cpu().numpy(), w["hist_y"])
            for k in ("cell_sum", "cell_sad"):
                assert g[k].dtype == torch.int32 and tuple(g[k].shape) == (w["gh"], w["gw"]) and np.array_equal(g[k].cpu().numpy(), w[k]), (name, f, k)
            assert g["hist_y"].untyped_storage().data_ptr() == whole[0]["hist_y"].untyped_storage().data_ptr(), "views of ONE device buffer"
        assert sorted(dec.frame_stats(0, items=[(0, 2, 0)])[0]) == sorted(su.U64 + su.U32 + ("hist_y",)), "no grid: no plane views"
        assert _scalars(dec.frame_stats(0, thresh=THRESH, items=[(0, 2, 0)])[0]) == _scalars(su.parse(c.item(2, 0)))
        # in two batches, with the flag (a new start: the whole stream's last frame is no predecessor of its first)
        dec.reset_stream(0)
        dec.decode([a])
        assert dec.stats_plan(0, history=True) == [(0, 0, NONE), (0, 1, 0)]
        parts = dec.frame_stats(0, 32, 3, THRESH, history=True)
        dec.decode([b])
        assert dec.stats_plan(0, history=True) == [(0, 0, HISTORY)] and dec.stats_plan(0) == [(0, 0, NONE)]
        # the item call names the history itself, byte for byte against the yardstick (before the batch call dates the slot with this batch)
        want2 = c.item(2, 1, 8, 3)
        got = _launch(dec, tod._device_buffer(want2.size), want2.size, [(0, 0, HISTORY)], 8, 3)
        assert np.array_equal(got, want2), (name, _first_diff(got, want2))
        parts += dec.frame_stats(0, 32, 3, THRESH, history=True)
        with pytest.raises(H.H264MIError):  # ... after which this batch's own history is no predecessor
            dec.stats_items(tod._device_buffer(4096).data_ptr(), 4096, [(0, 0, HISTORY)])
        assert want[2]["sad_y"] > 0 and want[2]["cell_sad"].any()
        for f in range(n):
            assert _scalars(parts[f]) == _scalars(whole[f]), (name, f)
            assert all(torch.equal(parts[f][k], whole[f][k]) for k in ("hist_y", "cell_sum", "cell_sad")), (name, f)
        assert np.array_equal(dec.read_frame_tight(0, 0, crop=True), c.i420[2])  # (frame 0 of the second batch is frame 2 of the stream)
        # without the flag the first frame of the second batch has no predecessor
        dec.decode([a])
        assert len(dec.frame_stats(0, thresh=THRESH)) == 2
        dec.decode([b])
        (r,) = dec.frame_stats(0, thresh=THRESH)
        assert _scalars(r) == _scalars(su.parse(c.item(2, None))) and int(r["has_prev"]) == 0
        # ... and after reset_stream: the history of the batch before is dated right, and yet it is not used
        dec.decode([a])
        assert len(dec.frame_stats(0, thresh=THRESH, history=True)) == 2
        dec.reset_stream(0)
        dec.decode([a])
        r = dec.frame_stats(0, thresh=THRESH, history=True)
        assert [int(x["has_prev"]) for x in r] == [0, 1] and _scalars(r[1]) == _scalars(su.parse(c.item(1, 0)))
        dec.decode([b])  # (the plain case once more: the frames of `a` are the references of `b`)
        (r,) = dec.frame_stats(0, thresh=THRESH, history=True)
        assert _scalars(r) == _scalars(su.parse(c.item(2, 1)))
        with pytest.raises(ValueError):
            dec.frame_stats(0, items=[(0, 0, NONE)], history=True)
        assert dec.device_bytes() == pool + slot
    finally:
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stats_first", [True, False])
def test_gpu_statistics_and_deinterlacer_keep_a_history_each(stats_first, cases, H):
    """One batch runs both deinterlace(mode="motion", history=True) and frame_stats(history=True), in either order; in the next batch both find their
    predecessor: the frame the batch before ended with."""
    import deintmotionutil as dmu
    c = cases["aligned_origin"]
    aus = c2.access_units(c.stream)
    a, b = b"".join(aus[:2]), b"".join(aus[2:])
    dec = tod._decoder(H, c)
    try:
        out = []
        for chunk in (a, b):
            dec.decode([chunk])
            calls = [lambda: out.append(dec.frame_stats(0, thresh=THRESH, history=True)), lambda: dec.deinterlace(0, "motion", rate=1, history=True)]
            for call in (calls if stats_first else calls[::-1]):
                call()
        (r,) = out[1]
        assert _scalars(r) == _scalars(su.parse(c.item(2, 1))) and int(r["has_prev"]) == 1
        assert dec.frame_count(D) == 1 and dec.derived_prev(0) == dmu.PREV_HISTORY
        assert np.array_equal(tod._read_derived(dec, 0, c.w, c.h), dmu.frame(c.i420[2], c.i420[1], c.w, c.h, tod.FIELD, 0))
    finally:
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["left_1", "field_bottom_first"])
def test_gpu_derived_sources(name, cases, H):
    """The statistics of a deinterlaced frame are the yardstick's of deintutil's frame; a derived frame's predecessor is another derived frame or none."""
    c = cases[name]
    dec = tod._decoder(H, c)
    try:
        dec.decode([c.stream])
        assert dec.deinterlace(mode="edge", items=[(0, f, 1) for f in range(c.n)]) == c.n
        frames = [c.want(tod.EDGE, 1, f) for f in range(c.n)]
        todo = [(D, f, f - 1 if f else NONE) for f in range(c.n)] + [(D, 1, 1)]
        want = np.concatenate([su.item(frames[f], None if p == NONE else frames[p], c.w, c.h, 16, 3, THRESH) for _, f, p in todo])
        got = _launch(dec, tod._device_buffer(want.size), want.size, todo, 16, 3)
        assert np.array_equal(got, want), (name, _first_diff(got, want))
        assert not np.array_equal(want[:1120], c.item(0, None, 16, 3)[:1120]), "the deinterlaced frame is not the woven one"
        for bad in ((D, 0, HISTORY), (D, c.n, NONE), (D, 0, c.n)):
            with pytest.raises(H.H264MIError):
                dec.stats_items(tod._device_buffer(4096).data_ptr(), 4096, [bad])
        with pytest.raises(H.H264MIError):
            dec.stats_plan(D)
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_mixed_geometries_in_one_batch_call(cases, H):
    """Two streams of unlike size in one batch call, stream-major: items of unlike length back to back, each at the sum of the item_bytes before it."""
    cs = [cases["aligned_origin"], cases["mono_odd"]]
    dec = H.Decoder(max_streams=2, max_width=max(c.info["coded_w"] for c in cs), max_height=max(c.info["coded_h"] for c in cs), max_frames_per_batch=3, max_slices_per_frame=1)
    try:
        dec.decode([c.stream for c in cs])
        plan = dec.stats_plan(-1)
        assert plan == [(s, f, f - 1 if f else NONE) for s in range(2) for f in range(3)]
        want = np.concatenate([cs[s].item(f, None if p == NONE else p, 8, 3) for s, f, p in plan])
        sizes = [su.item_bytes(cs[s].w, cs[s].h, 8, 3) for s, _, _ in plan]
        assert sizes[0] != sizes[3] and want.size == sum(sizes)
        buf = tod._device_buffer(want.size)
        assert dec.stats_batch(buf.data_ptr(), want.size, -1, 8, 3, THRESH) == want.size
        dec.sync()
        got = tod._filled(buf, want.size)
        assert np.array_equal(got, want), _first_diff(got, want)
        assert su.parse(got[sum(sizes[:4]):], 3)["w"] == cs[1].w and su.parse(got[sum(sizes[:2]):], 3)["w"] == cs[0].w
        # one stream of the two; capacity: *bytes is set and nothing is written; an unaligned destination
        buf = tod._device_buffer(want.size)
        assert dec.stats_batch(buf.data_ptr(), want.size, 1, 8, 3, THRESH) == sum(sizes[3:])
        dec.sync()
        assert np.array_equal(tod._filled(buf, sum(sizes[3:])), want[sum(sizes[:3]):])
        import ctypes
        n = ctypes.c_size_t(0)
        spec = H.stats_spec(8, 3, THRESH)
        buf = tod._device_buffer(want.size)
        assert dec._L.h264mi_batch_stats_device(dec._h, -1, ctypes.byref(spec), 0, buf.data_ptr(), want.size - 1, ctypes.byref(n)) == -7 and n.value == want.size
        assert dec._L.h264mi_batch_stats_device(dec._h, -1, ctypes.byref(spec), 0, buf.data_ptr() + 8, want.size, ctypes.byref(n)) == -1
        dec.sync()
        assert (buf.cpu().numpy() == 0xA5).all()
        views = dec.frame_stats(-1, 8, ("cell_sum",), THRESH)
        assert [(int(v["w"]), int(v["h"])) for v in views] == [(cs[s].w, cs[s].h) for s, _, _ in plan]
        for v, (s, f, p) in zip(views, plan):
            w = su.parse(cs[s].item(f, None if p == NONE else p, 8, 1), 1)
            assert _scalars(v) == {k: w[k] for k in su.U64 + su.U32} and np.array_equal(v["cell_sum"].cpu().numpy(), w["cell_sum"]) and "cell_sad" not in v
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
        pred = {order[0]: NONE}
        pred.update({order[i]: order[i - 1] for i in range(1, n)})
        assert dec.stats_plan(0) == [(0, f, pred[f]) for f in range(n)]
        want = np.concatenate([su.item(rec[f], None if pred[f] == NONE else rec[pred[f]], w, h, 64, 2, THRESH) for f in range(n)])
        by_decoding_order = np.concatenate([su.item(rec[f], rec[f - 1] if f else None, w, h, 64, 2, THRESH) for f in range(n)])
        assert not np.array_equal(want, by_decoding_order), "the records tell output order from decoding order"
        buf = tod._device_buffer(want.size)
        assert dec.stats_batch(buf.data_ptr(), want.size, 0, 64, 2, THRESH) == want.size
        dec.sync()
        got = tod._filled(buf, want.size)
        assert np.array_equal(got, want), _first_diff(got, want)
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_c_example_prints_stats(cases, tmp_path):
    """examples/h264mi_decode.c --stats: one line per frame; a file decoded in several batches has a predecessor for every frame but the first, because the
    example sets H264MI_STATS_HISTORY on every batch."""
    c = cases["field_bottom_first"]  # (five frames, ten field pictures: four pictures per batch are batches of 2 + 2 + 1 frames)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    src = tmp_path / "in.h264"
    src.write_bytes(c.stream)
    want = [su.parse(c.item(f, f - 1 if f else None)) for f in range(c.n)]
    assert want[2]["sad_y"] > 0 and want[4]["sad_y"] > 0, "the first frames of the second and the third batch"
    p = subprocess.run([os.path.join(ROOT, "examples", "h264mi_decode"), str(src), str(tmp_path / "out.yuv"), "4", "--stats"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       check=True, timeout=120)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("stats ")]
    assert len(lines) == c.n == 5
    px = c.w * c.h
    for f, (ln, w) in enumerate(zip(lines, want)):
        m = re.fullmatch(r"stats (\d+): mean_y ([\d.]+) sad_y/px ([\d.]+) changed_y (\d+) \(sum_y (\d+) sad_y (\d+) has_prev (\d)\)", ln)
        assert m, ln
        assert (int(m[1]), int(m[4]), int(m[5]), int(m[6]), int(m[7])) == (f, w["changed_y"], w["sum_y"], w["sad_y"], w["has_prev"]), (ln, w)
        assert m[2] == "%.3f" % (w["sum_y"] / px) and m[3] == "%.3f" % (w["sad_y"] / px), ln
    assert np.array_equal(np.frombuffer((tmp_path / "out.yuv").read_bytes(), np.uint8), c.i420.reshape(-1)), "the frames are written as without --stats"
