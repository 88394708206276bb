"""Frame statistics (K12), the host state without a GPU: the product's host side built against the null device of tools/hoststub (kernels are not run,
device memory is host memory), as tests/test_host_deint_motion.py does it.  Which predecessor every item gets (h264mi_batch_stats_plan), when a stream's
statistics history is valid -- and that it is not the deinterlacer's --, what is refused, what `*bytes` says and what the history arena costs are host
state.  The records themselves: tests/test_output_stats.py, on the device."""
import ctypes
import shutil

import pytest

import concealutil2 as c2
import statsutil as su
from conftest import MATRIX
from test_host_deint_motion import FIELD, MHost, _slot
from test_host_frame_fields import host  # noqa: F401  (the fixture: the null-device build)

EINVAL, ECAPACITY = -1, -7
D = 0x40000000  # H264MI_STREAM_DERIVED
NONE, HISTORY = su.PREV_NONE, su.PREV_HISTORY
FLAG = 1  # H264MI_STATS_HISTORY, and H264MI_DEINT_HISTORY
pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")
I32, SZ, VP = ctypes.c_int32, ctypes.c_size_t, ctypes.c_void_p


class SHost(MHost):
    def __init__(self, L, H, stream, kw):
        self.Spec, self.SItem = H._lib.StatsSpec, H._lib.StatsItem
        L.h264mi_items_stats_device.argtypes = [VP, ctypes.POINTER(self.Spec), ctypes.POINTER(self.SItem), I32, VP, SZ, ctypes.POINTER(SZ)]
        L.h264mi_batch_stats_device.argtypes = [VP, I32, ctypes.POINTER(self.Spec), I32, VP, SZ, ctypes.POINTER(SZ)]
        L.h264mi_batch_stats_plan.argtypes = [VP, I32, I32, ctypes.POINTER(self.SItem), I32, ctypes.POINTER(I32)]
        self.raw = ctypes.create_string_buffer((1 << 20) + 16)  # "device" memory of the null device, aligned to 16 bytes
        self.dst = (ctypes.addressof(self.raw) + 15) & ~15
        super().__init__(L, H, stream, kw)

    def plan(self, flags=0, stream=-1, cap=64):
        arr, n = (self.SItem * max(cap, 1))(), I32(-7)
        code = self.L.h264mi_batch_stats_plan(self.h, stream, flags, arr, cap, ctypes.byref(n))
        return code, [(a.stream, a.frame, a.prev_frame) for a in arr[:max(n.value, 0)]] if code == 0 else n.value

    def prevs(self, flags=FLAG):
        code, items = self.plan(flags)
        assert code == 0
        return [p for _, _, p in items]

    def sbatch(self, flags=0, stream=-1, spec=(0, 0, 0, 0), cap=1 << 20, dst=None):
        n = SZ(12345)
        return self.L.h264mi_batch_stats_device(self.h, stream, ctypes.byref(self.Spec(*spec)), flags, self.dst if dst is None else dst, cap, ctypes.byref(n)), n.value

    def sitems(self, items, spec=(0, 0, 0, 0), cap=1 << 20, dst=None):
        arr, n = (self.SItem * max(len(items), 1))(*[self.SItem(*it) for it in items]), SZ(12345)
        return self.L.h264mi_items_stats_device(self.h, ctypes.byref(self.Spec(*spec)), arr, len(items), self.dst if dst is None else dst, cap, ctypes.byref(n)), n.value


@pytest.mark.parametrize("name", ["cabac_IPP", "b_ibp_cabac"])
def test_host_plan_follows_output_order(name, host, sg, H):
    kw = MATRIX[name]
    d = SHost(host, H, sg.encode(want_recon=False, **kw)[0], kw)
    try:
        n, order = kw["frames"], d.order()
        assert d.count() == n and (order != list(range(n))) == bool(kw.get("bframes"))
        want = {order[0]: NONE}
        want.update({order[i]: order[i - 1] for i in range(1, n)})
        for stream in (-1, 0):
            for flags in (0, FLAG):
                assert d.plan(flags, stream) == (0, [(0, f, want[f]) for f in range(n)]), "decoding order; predecessors by output order; no history yet"
        one = su.item_bytes(kw["width"], kw["height"], 16, 3)
        assert d.sbatch(0, spec=(16, 3, 10, 0)) == (0, n * one), "the batch call is the plan through the item call"
        assert d.sitems([(0, f, want[f]) for f in range(n)] + [(0, 1, 1)], spec=(16, 3, 10, 0)) == (0, (n + 1) * one), "a frame may be its own predecessor"
        # the plan's own arguments
        assert d.plan(0, cap=n - 1) == (ECAPACITY, n) and d.plan(0, cap=n)[0] == 0
        k = I32(-7)
        assert host.h264mi_batch_stats_plan(d.h, -1, 0, None, 0, ctypes.byref(k)) == ECAPACITY and k.value == n
        assert host.h264mi_batch_stats_plan(d.h, -1, 0, None, 1, ctypes.byref(k)) == EINVAL and host.h264mi_batch_stats_plan(d.h, -1, 0, None, 0, None) == EINVAL
        for stream, flags in ((D, 0), (1, 0), (-2, 0), (0, 2), (0, 3), (0, -1)):
            assert d.plan(flags, stream)[0] == EINVAL, (stream, flags)
            assert d.sbatch(flags, stream) == (EINVAL, 12345), (stream, flags)
    finally:
        d.close()


def _halves(sg, kw):
    stream = sg.encode(want_recon=False, **kw)[0]
    aus = c2.access_units(stream)
    assert len(aus) == kw["frames"] == 4
    return stream, b"".join(aus[:2]), b"".join(aus[2:]), [b"".join(aus[:2]), aus[2], aus[3]]


def test_host_history_validity_over_consecutive_batches(host, sg, H):
    kw = MATRIX["cabac_IPP"]
    stream, a, b, thirds = _halves(sg, kw)
    d = SHost(host, H, stream, kw)
    try:
        one = su.item_bytes(kw["width"], kw["height"])
        d.feed(a)
        assert d.prevs() == [NONE, 0] and d.sbatch(FLAG) == (0, 2 * one), "no history yet; this call takes one"
        assert d.prevs() == [NONE, 0], "the batch's own history is not its predecessor"
        d.feed(b)
        assert d.prevs() == [HISTORY, 0] and d.prevs(0) == [NONE, 0], "the last frame of the batch before -- with the flag only"
        assert d.sitems([(0, 0, HISTORY), (0, 1, HISTORY)]) == (0, 2 * one), "an item may name it itself"
        assert d.sbatch(FLAG) == (0, 2 * one)
        # executing the same prepared batch again: its own history is not its predecessor, and the one before is gone
        assert host.h264mi_batch_execute(d.h) == 0 and host.h264mi_batch_sync(d.h) == 0
        assert d.prevs() == [NONE, 0] and d.sitems([(0, 0, 0), (0, 0, HISTORY)]) == (EINVAL, 12345)
        # three batches in a row, the flag every time: the first one has the re-executed batch's history (taken just above), the others the one before them
        assert d.sbatch(FLAG) == (0, 2 * one)
        for k, chunk in enumerate(thirds):
            d.feed(chunk)
            assert d.prevs()[0] == HISTORY and d.prevs(0)[0] == NONE, k
            assert d.sbatch(FLAG)[0] == 0
        # the flag off: the history that is there is not used by the plan, and none is taken
        d.feed(a)
        assert d.prevs(0) == [NONE, 0] and d.prevs() == [HISTORY, 0], "(the host cannot know that `a` is a new start: dates and geometry are what count)"
        assert d.sbatch(0) == (0, 2 * one)
        d.feed(b)
        assert d.prevs() == [NONE, 0], "the batch before took none"
        # a batch in between that took none ends it
        assert d.sbatch(FLAG)[0] == 0
        d.feed(a)
        d.feed(b)
        assert d.prevs() == [NONE, 0]
        # the plain case again, then a reset of the stream, then of the decoder
        d.feed(a)
        assert d.sbatch(FLAG)[0] == 0
        d.feed(b)
        assert d.prevs() == [HISTORY, 0] and d.sbatch(FLAG)[0] == 0
        assert host.h264mi_stream_reset(d.h, 0) == 0
        d.feed(a)
        assert d.prevs() == [NONE, 0], "h264mi_stream_reset ends the history"
        assert d.sbatch(FLAG)[0] == 0
        assert host.h264mi_decoder_reset(d.h) == 0
        d.feed(b[:0] + a)
        assert d.prevs() == [NONE, 0], "h264mi_decoder_reset ends the history"
        assert d.sbatch(FLAG)[0] == 0
        d.feed(b)
        assert d.prevs() == [HISTORY, 0]
    finally:
        d.close()


@pytest.mark.parametrize("stats_first", [True, False])
def test_host_the_two_histories_do_not_share_a_slot(stats_first, host, sg, H):
    """A statistics call and a motion-adaptive deinterlacing call in the same batch, in either order: in the next batch BOTH find their predecessor.  With
    one shared slot the second call of a batch would date it anew, and in the next batch ... both would still agree; but the call that runs second within
    the NEXT batch finds the slot dated by the first one of that batch, and no predecessor."""
    kw = MATRIX["cabac_IPP"]
    stream, a, b, _ = _halves(sg, kw)
    d = SHost(host, H, stream, kw)

    def both(want_stats, want_deint):
        calls = [lambda: (d.prevs(), d.sbatch(FLAG)[0]) == (want_stats, 0), lambda: d.batch(FIELD, 1, FLAG) == (0, 2) and MHost.prevs(d) == want_deint]
        for call in (calls if stats_first else calls[::-1]):
            assert call(), (stats_first, want_stats, want_deint)
    try:
        d.feed(a)
        both([NONE, 0], [NONE, 0])
        d.feed(b)
        both([HISTORY, 0], [HISTORY, 0])
        d.feed(a)  # only the deinterlacer this time: the statistics history ends, the deinterlacer's goes on
        assert d.batch(FIELD, 1, FLAG) == (0, 2) and MHost.prevs(d) == [HISTORY, 0]
        d.feed(b)
        both([NONE, 0], [HISTORY, 0])
        d.feed(a)  # ... and the other way round
        assert d.prevs() == [HISTORY, 0] and d.sbatch(FLAG)[0] == 0
        d.feed(b)
        both([HISTORY, 0], [NONE, 0])
    finally:
        d.close()


def test_host_history_arena_is_accounted(host, sg, H):
    kw = MATRIX["cabac_IPP"]
    stream = sg.encode(want_recon=False, **kw)[0]
    d = SHost(host, H, stream, kw)
    try:
        slot, before = _slot(kw), d.memory()
        assert d.sbatch(0)[0] == 0 and d.sitems([(0, 0, NONE)])[0] == 0 and d.plan(FLAG)[0] == 0 and d.memory() == before, "without the flag, and in the plan: nothing"
        one = su.item_bytes(kw["width"], kw["height"])
        assert d.sbatch(FLAG, cap=0) == (ECAPACITY, kw["frames"] * one) and d.sbatch(FLAG, cap=one) == (ECAPACITY, kw["frames"] * one) and d.memory() == before, \
            "a size query, or a destination that is too small, allocates nothing"
        assert d.prevs() == [NONE] + list(range(kw["frames"] - 1)), "... and takes no history"
        assert d.sbatch(FLAG)[0] == 0 and d.memory() == before + slot, "the history arena: a frame slot per stream, on first use"
        assert d.sbatch(FLAG, spec=(8, 3, 0, 0))[0] == 0 and d.memory() == before + slot, "kept: a second call allocates nothing"
        assert d.batch(FIELD, 1, FLAG)[0] == 0 and d.memory() == before + 2 * slot + kw["frames"] * slot, "the deinterlacer's history is another arena (and its derived frames)"
        assert host.h264mi_decoder_reset(d.h) == 0 and d.memory() == before + 2 * slot + kw["frames"] * slot
        e = SHost(host, H, stream, kw)  # a refused call with the flag allocates nothing (a fresh decoder)
        try:
            start = e.memory()
            assert e.sbatch(FLAG, spec=(8, 0, 0, 0)) == (EINVAL, 12345) and e.sbatch(FLAG | 2) == (EINVAL, 12345) and e.memory() == start
        finally:
            e.close()
    finally:
        d.close()


def test_host_capacity_sizes_and_refusals(host, sg, H):
    """Two sequences of unlike size in one batch: items are sized one by one, and a predecessor of another size is refused by the item call and resolves
    to none in the plan."""
    kw = MATRIX["cabac_IPP"]
    small = dict(kw, width=96, height=80, seed=kw.get("seed", 0) + 77)
    stream = sg.encode(want_recon=False, **kw)[0] + sg.encode(want_recon=False, **small)[0]
    d = SHost(host, H, stream, dict(kw, frames=2 * kw["frames"]))
    try:
        n = kw["frames"]
        assert d.count() == 2 * n
        assert d.prevs(0) == [NONE] + list(range(n - 1)) + [NONE] + list(range(n, 2 * n - 1)), "the first frame of the other size has no predecessor"
        spec = (32, 3, 7, 0)
        big, sml = su.item_bytes(kw["width"], kw["height"], 32, 3), su.item_bytes(96, 80, 32, 3)
        assert big != sml and d.sbatch(0, spec=spec) == (0, n * big + n * sml)
        # capacity: *bytes is set, nothing is written
        ctypes.memset(d.dst, 0xA5, 4096)
        assert d.sbatch(0, spec=spec, cap=n * big + n * sml - 1) == (ECAPACITY, n * big + n * sml)
        assert d.sitems([(0, 0, NONE), (0, n, NONE)], spec=spec, cap=big) == (ECAPACITY, big + sml)
        assert ctypes.string_at(d.dst, 4096) == b"\xa5" * 4096
        assert d.sitems([(0, 0, NONE), (0, n, NONE)], spec=spec, cap=big + sml) == (0, big + sml)
        assert big + sml < 4096 and ctypes.string_at(d.dst, 4096) == bytes(big + sml) + b"\xa5" * (4096 - big - sml), \
            "exactly the destination range is cleared ahead of the launch (the null device runs no kernel)"
        # n = 0 succeeds with *bytes = 0, whatever the capacity
        assert d.sitems([], cap=0) == (0, 0) and host.h264mi_items_stats_device(d.h, ctypes.byref(d.Spec(0, 0, 0, 0)), None, 0, d.dst, 0, None) == 0
        # refusals: nothing is written
        ctypes.memset(d.dst, 0xA5, 4096)
        bad = [(0, n, n - 1), (0, n - 1, n),  # a predecessor of another geometry
               (0, 0, 2 * n), (0, 0, -3), (0, 0, D),  # a bad prev_frame
               (0, 0, HISTORY),  # no history was ever taken
               (0, 2 * n, NONE), (1, 0, NONE), (-1, 0, NONE), (D, 0, NONE)]  # no such frame, no such stream, no derived frame yet
        for item in bad:
            assert d.sitems([(0, 1, 0), item]) == (EINVAL, 12345), item
        for sp in ((8, 0, 0, 0), (0, 1, 0, 0), (16, 4, 0, 0), (24, 1, 0, 0), (16, 1, 256, 0), (16, 1, -1, 0), (16, 1, 0, 1)):
            assert d.sitems([(0, 0, NONE)], spec=sp) == (EINVAL, 12345) and d.sitems([], spec=sp) == (EINVAL, 12345), sp
        assert d.sitems([(0, 0, NONE)], dst=d.dst + 8) == (EINVAL, 12345) and d.sitems([(0, 0, NONE)], dst=d.dst + 1) == (EINVAL, 12345), "an unaligned destination"
        assert d.sbatch(0, dst=d.dst + 4) == (EINVAL, 12345)
        sp0 = ctypes.byref(d.Spec(0, 0, 0, 0))
        assert host.h264mi_items_stats_device(d.h, sp0, None, 1, d.dst, 1 << 20, None) == EINVAL and host.h264mi_items_stats_device(d.h, sp0, None, -1, d.dst, 1 << 20, None) == EINVAL
        assert host.h264mi_items_stats_device(d.h, None, None, 0, d.dst, 0, None) == EINVAL and host.h264mi_items_stats_device(d.h, sp0, None, 0, None, 0, None) == EINVAL
        assert ctypes.string_at(d.dst, 4096) == b"\xa5" * 4096
        # derived sources: another derived frame or none; the history is refused there
        assert d.mitems(FIELD, [(0, 0, 0, NONE), (0, 1, 0, 0), (0, n, 0, NONE)]) == (0, 3)
        one = su.item_bytes(kw["width"], kw["height"])
        assert d.sitems([(D, 0, NONE), (D, 1, 0), (D, 1, 1)]) == (0, 3 * one)
        assert d.sbatch(FLAG)[0] == 0  # (so that a history exists at all)
        for item in ((D, 0, HISTORY), (D, 3, NONE), (D, 0, 3), (D, 2, 0), (D, 0, 2)):  # ... no such derived frame; a derived predecessor of another geometry
            assert d.sitems([item]) == (EINVAL, 12345), item
    finally:
        d.close()
