"""JPEG snapshots (K13), the host state without a GPU: the product's host side built against the null device of tools/hoststub (kernels are not run,
device memory is host memory), as tests/test_host_stats.py does it.  What is refused, what `*bytes` says, that nothing is written on failure, and what the
interval table costs and when are host state.  The files themselves: tests/test_output_jpeg.py, on the device."""
import ctypes
import shutil

import pytest

import jpegutil as ju
from conftest import MATRIX
from test_host_deint_motion import FIELD, MHost
from test_host_frame_fields import host  # noqa: F401  (the fixture: the null-device build)

EINVAL, ECAPACITY = -1, -7
D = 0x40000000  # H264MI_STREAM_DERIVED
AUTO, KEEP, FULL = ju.RANGE_AUTO, ju.RANGE_KEEP, ju.RANGE_FULL
pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")
I32, SZ, VP = ctypes.c_int32, ctypes.c_size_t, ctypes.c_void_p
HDR = 629
SLOT = 2048


class JHost(MHost):
    def __init__(self, L, H, stream, kw):
        self.Spec, self.JItem = H._lib.JpegSpec, H._lib.JpegItem
        L.h264mi_items_jpeg_device.argtypes = [VP, ctypes.POINTER(self.Spec), ctypes.POINTER(self.JItem), I32, SZ, VP, SZ, ctypes.POINTER(SZ)]
        L.h264mi_batch_jpeg_device.argtypes = [VP, I32, ctypes.POINTER(self.Spec), SZ, VP, SZ, ctypes.POINTER(SZ)]
        L.h264mi_i420_jpeg_device.argtypes = [VP, ctypes.POINTER(self.Spec), VP, I32, I32, I32, I32, SZ, VP, SZ, ctypes.POINTER(SZ)]
        L.h264mi_jpeg_size.argtypes = [ctypes.POINTER(self.Spec), I32, I32, I32, ctypes.POINTER(SZ), ctypes.POINTER(SZ)]
        self.raw = ctypes.create_string_buffer((1 << 20) + 16)  # "device" memory of the null device, aligned to 16 bytes
        self.dst = (ctypes.addressof(self.raw) + 15) & ~15
        self.src = ctypes.create_string_buffer(1 << 16)
        super().__init__(L, H, stream, kw)

    def jbatch(self, stream=-1, spec=(90, AUTO, 0, 0), slot=SLOT, cap=1 << 20, dst=None):
        n = SZ(12345)
        return self.L.h264mi_batch_jpeg_device(self.h, stream, ctypes.byref(self.Spec(*spec)), slot, self.dst if dst is None else dst, cap, ctypes.byref(n)), n.value

    def jitems(self, items, spec=(90, AUTO, 0, 0), slot=SLOT, cap=1 << 20, dst=None):
        arr, n = (self.JItem * max(len(items), 1))(*[self.JItem(*it) for it in items]), SZ(12345)
        return self.L.h264mi_items_jpeg_device(self.h, ctypes.byref(self.Spec(*spec)), arr, len(items), slot, self.dst if dst is None else dst, cap, ctypes.byref(n)), n.value

    def ji420(self, n_frames, w=16, h=16, mono=0, spec=(90, KEEP, 0, 0), slot=SLOT, cap=1 << 20, dst=None, src=True):
        n = SZ(12345)
        return self.L.h264mi_i420_jpeg_device(self.h, ctypes.byref(self.Spec(*spec)), ctypes.addressof(self.src) if src else None, w, h, mono, n_frames, slot,
                                              self.dst if dst is None else dst, cap, ctypes.byref(n)), n.value


def _total(n, slot=SLOT):
    return ((16 * n + 255) & ~255) + n * slot if n else 0


def test_host_sizes_capacity_and_refusals(host, sg, H):
    kw = MATRIX["cabac_IPP"]
    d = JHost(host, H, sg.encode(want_recon=False, **kw)[0], kw)
    try:
        n = kw["frames"]
        assert d.count() == n
        hb, bb = SZ(0), SZ(0)
        assert host.h264mi_jpeg_size(ctypes.byref(d.Spec(90, KEEP, 0, 0)), kw["width"], kw["height"], 0, ctypes.byref(hb), ctypes.byref(bb)) == 0 and hb.value == HDR
        # sizes: the results, rounded up to 256 bytes, then a slot per item; also on H264MI_ECAPACITY, where nothing is written
        ctypes.memset(d.dst, 0xA5, 8192)
        assert d.jbatch() == (0, _total(n)) and d.jbatch(stream=0, slot=HDR + 11) == (0, _total(n, HDR + 11)) and d.jitems([(0, 1), (0, 1), (0, 0)]) == (0, _total(3))
        assert d.jitems([(0, 0)] * 17) == (0, 512 + 17 * SLOT), "17 results need two times 256 bytes"
        assert d.jbatch(cap=_total(n) - 1) == (ECAPACITY, _total(n)) and d.jbatch(cap=0) == (ECAPACITY, _total(n)) and d.jitems([(0, 0)], cap=SLOT) == (ECAPACITY, _total(1))
        assert d.ji420(3) == (0, _total(3)) and d.ji420(3, cap=_total(3) - 1) == (ECAPACITY, _total(3)) and d.ji420(2, w=33, h=17, mono=1, slot=336) == (0, _total(2, 336))
        assert ctypes.string_at(d.dst, 8192) == b"\xa5" * 8192, "the null device runs no kernel, and the host writes nothing itself"
        # n = 0 succeeds with *bytes = 0, whatever the capacity
        assert d.jitems([], cap=0) == (0, 0) and d.ji420(0, cap=0) == (0, 0) and d.ji420(0, cap=0, src=False) == (0, 0)
        assert host.h264mi_items_jpeg_device(d.h, ctypes.byref(d.Spec(90, AUTO, 0, 0)), None, 0, SLOT, d.dst, 0, None) == 0
        # every refusal: the spec ...
        for sp in ((0, KEEP, 0, 0), (101, KEEP, 0, 0), (-5, KEEP, 0, 0), (90, 3, 0, 0), (90, -1, 0, 0), (90, KEEP, -1, 0), (90, KEEP, 65536, 0), (90, KEEP, 0, 1), (90, KEEP, 0, -2)):
            assert d.jitems([(0, 0)], spec=sp) == (EINVAL, 12345) and d.jitems([], spec=sp) == (EINVAL, 12345) and d.jbatch(spec=sp) == (EINVAL, 12345), sp
            assert d.ji420(1, spec=sp) == (EINVAL, 12345) and d.ji420(0, spec=sp) == (EINVAL, 12345), sp
        assert d.ji420(1, spec=(90, AUTO, 0, 0)) == (EINVAL, 12345), "AUTO needs a stream"
        assert b"AUTO" in host.h264mi_last_error_string()
        # ... the slot: not a multiple of 16, below the header (334 bytes for mono)
        for slot in (SLOT + 8, SLOT - 1, HDR - 5, 624, 0):
            assert d.jitems([(0, 0)], slot=slot) == (EINVAL, 12345) and d.jbatch(slot=slot) == (EINVAL, 12345) and d.ji420(1, slot=slot) == (EINVAL, 12345), slot
        assert d.jitems([(0, 0)], slot=640)[0] == 0 and d.ji420(1, mono=1, slot=336)[0] == 0 and d.ji420(1, mono=1, slot=320) == (EINVAL, 12345)
        # ... the destination: unaligned, null
        for off in (1, 4, 8):
            assert d.jitems([(0, 0)], dst=d.dst + off) == (EINVAL, 12345) and d.jbatch(dst=d.dst + off) == (EINVAL, 12345) and d.ji420(1, dst=d.dst + off) == (EINVAL, 12345)
        sp0 = ctypes.byref(d.Spec(90, KEEP, 0, 0))
        assert host.h264mi_items_jpeg_device(d.h, sp0, None, 0, SLOT, None, 0, None) == EINVAL and host.h264mi_items_jpeg_device(d.h, None, None, 0, SLOT, d.dst, 0, None) == EINVAL
        assert host.h264mi_items_jpeg_device(d.h, sp0, None, 1, SLOT, d.dst, 1 << 20, None) == EINVAL and host.h264mi_items_jpeg_device(d.h, sp0, None, -1, SLOT, d.dst, 1 << 20, None) == EINVAL
        assert host.h264mi_items_jpeg_device(None, sp0, None, 0, SLOT, d.dst, 0, None) == EINVAL
        # ... a frame that does not exist; a stream that does not
        for item in ((0, n), (0, -1), (1, 0), (-1, 0), (D, 0)):
            assert d.jitems([(0, 0), item]) == (EINVAL, 12345), item
        for stream in (1, -2):
            assert d.jbatch(stream=stream) == (EINVAL, 12345)
        # ... the size of caller-held frames
        for w, h in ((0, 16), (16, 0), (16385, 16), (16, -3)):
            assert d.ji420(1, w=w, h=h) == (EINVAL, 12345)
        assert d.ji420(-1) == (EINVAL, 12345) and d.ji420(1, src=False) == (EINVAL, 12345)
        assert ctypes.string_at(d.dst, 8192) == b"\xa5" * 8192
        # derived frames are sources; the batch call of the pseudo-stream takes them all
        assert d.mitems(FIELD, [(0, 0, 0, -1), (0, 1, 1, -1)]) == (0, 2)
        assert d.jitems([(D, 1), (0, 0), (D, 0)]) == (0, _total(3)) and d.jbatch(stream=D) == (0, _total(2)) and d.jitems([(D, 2)]) == (EINVAL, 12345)
    finally:
        d.close()


def test_host_interval_table_is_accounted(host, sg, H):
    kw = MATRIX["cabac_IPP"]
    stream = sg.encode(want_recon=False, **kw)[0]
    d = JHost(host, H, stream, kw)
    try:
        n, before = kw["frames"], d.memory()
        rows, mcus = (kw["height"] + 15) // 16, ((kw["width"] + 15) // 16) * ((kw["height"] + 15) // 16)
        assert d.jbatch(spec=(0, KEEP, 0, 0)) == (EINVAL, 12345) and d.jbatch(slot=SLOT + 1) == (EINVAL, 12345) and d.jitems([(0, n)]) == (EINVAL, 12345)
        assert d.jbatch(cap=0)[0] == ECAPACITY and d.jitems([]) == (0, 0) and d.memory() == before, "a refused call, a size query and an empty call allocate nothing"
        assert d.jitems([(0, 0)])[0] == 0 and d.memory() == before + 4 * rows, "4 bytes per restart interval: one per MCU row"
        assert d.jitems([(0, 1)])[0] == 0 and d.jbatch(spec=(0, KEEP, 0, 0))[0] == EINVAL and d.memory() == before + 4 * rows, "kept"
        assert d.jbatch()[0] == 0 and d.memory() == before + 4 * n * rows, "grown to the largest call"
        assert d.jbatch(spec=(50, FULL, 1, 0))[0] == 0 and d.memory() == before + 4 * n * mcus, "an interval per MCU"
        assert d.jitems([(0, 0)])[0] == 0 and d.ji420(1)[0] == 0 and d.memory() == before + 4 * n * mcus, "... and never shrunk"
        assert host.h264mi_decoder_reset(d.h) == 0 and d.memory() == before + 4 * n * mcus
    finally:
        d.close()
