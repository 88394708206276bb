"""Motion-adaptive deinterlacing, the host state without a GPU: the product's host side built against the null device of tools/hoststub (kernels are not
run, device memory is host memory), as tests/test_host_frame_fields.py does it.  Which predecessor every derived frame gets, when a stream's history is
valid, which calls are refused and what the history arena costs are host state; h264mi_derived_prev makes them testable without a sample.  The samples
themselves: tests/test_output_deinterlace_motion.py, on the device."""
import ctypes
import shutil

import pytest

import concealutil2 as c2
from conftest import FIELD_MATRIX, MATRIX, pictures_of
from test_host_frame_fields import Host, host  # noqa: F401  (the fixture: the null-device build)

EINVAL = -1
D = 0x40000000  # H264MI_STREAM_DERIVED
FIELD, BLEND, EDGE = 0, 1, 2
NONE, HISTORY = -1, -2  # H264MI_DEINT_PREV_NONE, _PREV_HISTORY
FLAG = 1                # H264MI_DEINT_HISTORY
pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")


class MHost(Host):
    def __init__(self, L, H, stream, kw):
        self.MItem = H._lib.DeintMotionItem
        L.h264mi_batch_deinterlace_motion.argtypes = [ctypes.c_void_p] + [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_int32)]
        super().__init__(L, H, stream, kw)

    def feed(self, chunk):
        self.bufs, self.lens = (ctypes.c_char_p * 1)(chunk), (ctypes.c_size_t * 1)(len(chunk))
        self.decode()

    def batch(self, mode=FIELD, rate=1, flags=0, stream=-1):
        n = ctypes.c_int32(-7)
        return self.L.h264mi_batch_deinterlace_motion(self.h, stream, mode, rate, flags, ctypes.byref(n)), n.value

    def mitems(self, mode, items):
        arr = (self.MItem * max(len(items), 1))(*[self.MItem(*it) for it in items])
        n = ctypes.c_int32(-7)
        return self.L.h264mi_items_deinterlace_motion(self.h, mode, arr, len(items), ctypes.byref(n)), n.value

    def prevs(self):
        out = []
        for k in range(self.count(D)):
            v = ctypes.c_int32(-9)
            assert self.L.h264mi_derived_prev(self.h, k, ctypes.byref(v)) == 0
            out.append(v.value)
        return out

    def order(self, stream=0):
        n = self.count(stream)
        arr, k = (ctypes.c_int32 * max(n, 1))(), ctypes.c_int32(-1)
        assert self.L.h264mi_stream_output_order(self.h, stream, arr, n, ctypes.byref(k)) == 0 and k.value == n
        return list(arr[:n])


def _slot(kw):
    return (((kw["width"] + 15) & ~15) * ((kw["height"] + 15) & ~15) * 3 // 2 + 255) & ~255


@pytest.mark.parametrize("name,rate", [("cabac_IPP", 1), ("b_ibp_cabac", 1), ("b_ibp_cabac", 2), ("field_bottom_first", 2)])
def test_host_predecessors_follow_output_order(name, rate, host, sg, H):
    """A frame's predecessor is the frame before it in output order; the first has none; both derived frames of a rate-2 frame share it."""
    kw = dict(MATRIX, **FIELD_MATRIX)[name]
    d = MHost(host, H, sg.encode(want_recon=False, **kw)[0], kw)
    try:
        n, order = kw["frames"], d.order()
        assert d.count() == n and sorted(order) == list(range(n))
        assert (order != list(range(n))) == bool(kw.get("bframes")), "output order differs from decoding order exactly where there are B pictures"
        want = {order[0]: NONE}
        want.update({order[i]: order[i - 1] for i in range(1, n)})
        assert d.batch(EDGE, rate) == (0, rate * n) and d.count(D) == rate * n
        assert d.prevs() == [want[f] for f in range(n) for _ in range(rate)]
        assert d.fields(D, rate * n - 1) == d.fields(0, n - 1), "a derived frame reports its source's values"
        # the same through the item call; a frame may be its own predecessor
        assert d.mitems(FIELD, [(0, f, -1, want[f]) for f in range(n)] + [(0, 1, 1, 1)]) == (0, n + 1)
        assert d.prevs() == [want[f] for f in range(n)] + [1]
        # derived frames of the spatial modes have none
        assert d.items(EDGE, [(0, 0, 0), (0, 1, 1)]) == (0, 2) and d.prevs() == [NONE, NONE]
        v = ctypes.c_int32(-9)
        for k in (-1, 2):
            assert host.h264mi_derived_prev(d.h, k, ctypes.byref(v)) == EINVAL
        assert host.h264mi_derived_prev(d.h, 0, None) == EINVAL and v.value == -9
    finally:
        d.close()


def test_host_history_validity_over_consecutive_batches(host, sg, H):
    kw = MATRIX["cabac_IPP"]
    stream = sg.encode(want_recon=False, **kw)[0]
    aus = c2.access_units(stream)
    assert len(aus) == kw["frames"] == 4
    a, b = b"".join(aus[:2]), b"".join(aus[2:])  # cut at an access-unit boundary; `a` starts with the IDR picture and the parameter sets
    d = MHost(host, H, stream, kw)
    try:
        d.feed(a)
        assert d.count() == 2
        assert d.batch(FIELD, 1, FLAG) == (0, 2) and d.prevs() == [NONE, 0], "no history yet"
        d.feed(b)
        assert d.batch(FIELD, 2, FLAG) == (0, 4) and d.prevs() == [HISTORY, HISTORY, 0, 0], "the last frame of the batch before"
        # executing the same prepared batch again: its own history is not its predecessor, and the one before is gone
        assert host.h264mi_batch_execute(d.h) == 0 and host.h264mi_batch_sync(d.h) == 0
        assert d.batch(FIELD, 1, FLAG) == (0, 2) and d.prevs() == [NONE, 0]
        assert d.mitems(FIELD, [(0, 0, 0, 0), (0, 0, 0, HISTORY)]) == (EINVAL, -7) and d.prevs() == [NONE, 0]
        # the flag off: the history that is there is not used, and none is taken
        d.feed(a)
        assert d.batch(FIELD, 1, 0) == (0, 2) and d.prevs() == [NONE, 0]
        assert d.mitems(FIELD, [(0, 0, 0, HISTORY)]) == (0, 1), "(it is valid all the same: an item may still name it)"
        d.feed(b)
        assert d.batch(FIELD, 1, FLAG) == (0, 2) and d.prevs() == [NONE, 0], "the batch before took none"
        # a batch in between that was not deinterlaced
        d.feed(a)
        d.feed(b)
        assert d.batch(FIELD, 1, FLAG) == (0, 2) and d.prevs() == [NONE, 0]
        # ... and the plain case again, then a reset of the stream, then a reset of the decoder
        d.feed(a)
        assert d.batch(EDGE, 1, FLAG) == (0, 2) and d.prevs() == [HISTORY, 0]
        d.feed(b)
        assert d.batch(EDGE, 1, FLAG) == (0, 2) and d.prevs() == [HISTORY, 0]
        assert host.h264mi_stream_reset(d.h, 0) == 0 and d.count(D) == 0
        d.feed(a)
        assert d.batch(EDGE, 1, FLAG) == (0, 2) and d.prevs() == [NONE, 0], "h264mi_stream_reset ends the history"
        assert host.h264mi_decoder_reset(d.h) == 0
        d.feed(a)
        assert d.batch(EDGE, 1, FLAG) == (0, 2) and d.prevs() == [NONE, 0], "h264mi_decoder_reset ends the history"
        d.feed(b)
        assert d.batch(EDGE, 1, FLAG) == (0, 2) and d.prevs() == [HISTORY, 0]
    finally:
        d.close()


def test_host_refused_calls_leave_the_list_intact_and_sizes_must_match(host, sg, H):
    """Two sequences of unlike size in one batch: a predecessor of another size is refused by the item call and resolves to none in the batch call."""
    kw = MATRIX["cabac_IPP"]
    small = dict(kw, width=96, height=80, seed=kw.get("seed", 0) + 77)
    stream = sg.encode(want_recon=False, **kw)[0] + sg.encode(want_recon=False, **small)[0]
    both = dict(kw, frames=2 * kw["frames"])
    d = MHost(host, H, stream, both)
    try:
        n = kw["frames"]
        assert d.count() == 2 * n and d.order() == list(range(2 * n))
        assert d.batch(FIELD, 1, 0) == (0, 2 * n)
        assert d.prevs() == [NONE] + list(range(n - 1)) + [NONE] + list(range(n, 2 * n - 1)), "the first frame of the other size has no predecessor"
        assert d.mitems(EDGE, [(0, 0, 0, NONE), (0, n, 1, n + 1)]) == (0, 2) and d.prevs() == [NONE, n + 1]
        bad = [(FIELD, (0, n, 0, n - 1)), (FIELD, (0, n - 1, 0, n)),  # a predecessor of another size
               (FIELD, (0, 0, 0, 2 * n)), (FIELD, (0, 0, 0, -3)), (FIELD, (0, 0, 0, D)),  # a bad prev_frame
               (FIELD, (0, 0, 0, HISTORY)),  # no history was ever taken
               (FIELD, (D, 0, 0, NONE)), (FIELD, (0, 2 * n, 0, NONE)), (FIELD, (1, 0, 0, NONE)),  # the derived pseudo-stream as a source; no such frame; no such stream
               (FIELD, (0, 0, 2, NONE)), (EDGE, (0, 0, -2, NONE)),  # a bad parity
               (BLEND, (0, 0, 0, NONE)), (3, (0, 0, 0, NONE)), (-1, (0, 0, 0, NONE))]  # BLEND has no parity; no such mode
        for mode, item in bad:
            assert d.mitems(mode, [(0, 1, 0, 0), item]) == (EINVAL, -7), (mode, item)
            assert d.count(D) == 2 and d.prevs() == [NONE, n + 1], (mode, item)
        assert host.h264mi_items_deinterlace_motion(d.h, FIELD, None, 1, None) == EINVAL and host.h264mi_items_deinterlace_motion(d.h, FIELD, None, -1, None) == EINVAL
        for args in ((0, BLEND, 1, 0), (0, 3, 1, 0), (0, FIELD, 0, 0), (0, FIELD, 3, 0), (0, FIELD, 1, 2), (0, FIELD, 1, -1), (0, EDGE, 2, 3), (D, FIELD, 1, 0),
                     (1, FIELD, 1, 0), (-2, FIELD, 1, 0)):
            assert host.h264mi_batch_deinterlace_motion(d.h, *args, None) == EINVAL, args
            assert d.count(D) == 2 and d.prevs() == [NONE, n + 1], args
        assert d.mitems(FIELD, []) == (0, 0) and d.count(D) == 0  # n = 0 empties the list
    finally:
        d.close()


def test_host_history_arena_is_accounted(host, sg, H):
    kw = MATRIX["cabac_IPP"]
    stream = sg.encode(want_recon=False, **kw)[0]
    d = MHost(host, H, stream, kw)
    try:
        n, slot, before = kw["frames"], _slot(kw), d.memory()
        assert d.batch(FIELD, 1, 0) == (0, n) and d.memory() == before + n * slot, "without the flag: the derived frames only"
        assert d.mitems(EDGE, [(0, 0, 0, NONE)]) == (0, 1) and d.memory() == before + n * slot
        assert d.batch(FIELD, 1, FLAG) == (0, n) and d.memory() == before + (n + 1) * slot, "the history arena: a frame slot per stream, on first use"
        assert d.batch(EDGE, 2, FLAG) == (0, 2 * n) and d.memory() == before + (2 * n + 1) * slot, "kept: a second call allocates no history"
        assert host.h264mi_decoder_reset(d.h) == 0 and d.memory() == before + (2 * n + 1) * slot
        # a refused call with the flag allocates nothing either (a fresh decoder)
        e = MHost(host, H, stream, kw)
        try:
            start = e.memory()
            assert host.h264mi_batch_deinterlace_motion(e.h, 0, BLEND, 1, FLAG, None) == EINVAL and e.memory() == start
        finally:
            e.close()
    finally:
        d.close()
