"""h264mi_frame_fields and the list of derived frames on the CPU: the product's host side built against the null device of tools/hoststub (kernels are
not run, device memory is host memory), loaded through ctypes.  What a frame's fields are is picture management (8.2.1 and the field bookkeeping of
mi_picture.cpp), and the lifetime of the derived frames is host state: both can be held to the generator's recipes without a GPU.  What this cannot show
is a single sample -- tests/test_output_deinterlace.py does that on the device."""
import ctypes
import os
import shutil

import pytest

import hostprog
from conftest import FIELD_MATRIX, MATRIX, pictures_of

EINVAL = -1
D = 0x40000000  # H264MI_STREAM_DERIVED
pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")


@pytest.fixture(scope="module")
def host(tmp_path_factory, H):
    prog = hostprog.build("host_pocs.sh", tmp_path_factory.mktemp("host_fields"))
    L = ctypes.CDLL(os.path.join(os.path.dirname(prog), "libh264mi_host.so"))
    L.h264mi_last_error_string.restype = ctypes.c_char_p
    return L


class Host:
    """One decoder of the null-device build with one stream prepared and executed."""

    def __init__(self, L, H, stream, kw):
        self.L, self.h = L, ctypes.c_void_p()
        cfg = H._lib.Config()
        cfg.struct_size, cfg.max_streams = ctypes.sizeof(cfg), 1
        cfg.max_width, cfg.max_height = (kw["width"] + 15) & ~15, (kw["height"] + 15) & ~15
        cfg.max_frames_per_batch, cfg.max_slices_per_frame, cfg.max_bitstream_bytes = pictures_of(kw), 8, len(stream) + 4096
        assert L.h264mi_decoder_create(ctypes.byref(cfg), ctypes.byref(self.h)) == 0, L.h264mi_last_error_string()
        self.bufs, self.lens = (ctypes.c_char_p * 1)(stream), (ctypes.c_size_t * 1)(len(stream))
        self.info = H._lib.BatchInfo()
        self.FieldInfo, self.Item = H._lib.FieldInfo, H._lib.DeintItem
        self.decode()

    def decode(self):
        assert self.L.h264mi_batch_prepare(self.h, 1, self.bufs, self.lens, ctypes.byref(self.info)) == 0, self.L.h264mi_last_error_string()
        assert self.L.h264mi_batch_execute(self.h) == 0 and self.L.h264mi_batch_sync(self.h) == 0

    def count(self, stream=0):
        n = ctypes.c_int32(-1)
        assert self.L.h264mi_stream_frame_count(self.h, stream, ctypes.byref(n)) == 0
        return n.value

    def fields(self, stream, frame):
        ff = self.FieldInfo()
        assert self.L.h264mi_frame_fields(self.h, stream, frame, ctypes.byref(ff)) == 0
        return ff.field_coded, ff.first_parity, ff.top_field_order_cnt, ff.bottom_field_order_cnt

    def items(self, mode, items):
        arr = (self.Item * max(len(items), 1))(*[self.Item(*it) for it in items])
        n = ctypes.c_int32(-7)
        return self.L.h264mi_items_deinterlace(self.h, mode, arr, len(items), ctypes.byref(n)), n.value

    def memory(self):
        v = ctypes.c_int64(0)
        assert self.L.h264mi_decoder_memory(self.h, ctypes.byref(v)) == 0
        return v.value

    def close(self):
        assert self.L.h264mi_decoder_destroy(self.h) == 0


def _as_fields(kw, t):
    """Frame t (decoding order, no B pictures) is coded as two fields: streamgen's choice for field_pics 3 (sg_enc.c), every frame for 1 and 2."""
    if kw.get("field_pics") == 3:
        return int(((kw["seed"] * 7 + t * 5 + t // 3) & 0xffffffff) % 3 != 0)
    return int(bool(kw.get("field_pics")))


CASES = ["cabac_IPP", "poc_bottom_first", "poc_bottom_later", "poc_bottom_first_mmco5", "interlace_sps_cabac", "field_IP", "field_bottom_first", "field_mixed_paff",
         "field_poc2_qpjitter", "field_wp_poc1", "field_fmo_explicit_bff"]


@pytest.mark.parametrize("name", CASES)
def test_host_frame_fields_match_the_recipe(name, host, sg, H):
    kw = dict(MATRIX, **FIELD_MATRIX)[name]
    stream = sg.encode(want_recon=False, **kw)[0]
    pocs = sg.last_pocs()
    d = Host(host, H, stream, kw)
    try:
        assert d.count() == kw["frames"]
        early = 0
        for f in range(kw["frames"]):
            fc, first, top, bot = d.fields(0, f)
            assert fc == _as_fields(kw, f), (name, f)
            assert min(top, bot) == pocs[f], (name, f, top, bot, pocs[f])
            if top != bot:
                assert first == int(bot < top), (name, f, top, bot)  # (operation 5 subtracts the same value from both: the relation survives it)
            if fc:  # the field decoded first; pic_order_cnt_type 2 gives both fields of a reference frame one count (output order is decoding order there)
                assert first == int(kw["field_pics"] == 2) and (top != bot or kw.get("poc_type") == 2), (name, f, top, bot)
            elif kw.get("poc_bottom_delta", 0) > 0:
                assert bot - top == kw["poc_bottom_delta"]
            elif not kw.get("poc_bottom_delta"):
                assert top == bot
            early += first
        if kw.get("poc_bottom_delta", 0) < 0:  # every frame but the IDR pictures (delta_pic_order_cnt_bottom 0 there: Min(top, bottom) must be 0)
            assert 0 < early < kw["frames"]
            assert d.fields(0, 0)[1] == 0 and d.fields(0, 1)[1:] == (1,) + d.fields(0, 1)[2:]
        ff = d.FieldInfo()
        assert host.h264mi_frame_fields(d.h, 0, kw["frames"], ctypes.byref(ff)) == EINVAL and host.h264mi_frame_fields(d.h, 1, 0, ctypes.byref(ff)) == EINVAL
        assert host.h264mi_frame_fields(d.h, 0, 0, None) == EINVAL and host.h264mi_frame_fields(d.h, D, 0, ctypes.byref(ff)) == EINVAL
    finally:
        d.close()


def test_host_derived_list_lifetime(host, sg, H):
    kw = FIELD_MATRIX["field_bottom_first"]
    stream = sg.encode(want_recon=False, **kw)[0]
    slot = kw["width"] * kw["height"] * 3 // 2
    d = Host(host, H, stream, kw)
    try:
        n, before = kw["frames"], d.memory()
        assert d.count(D) == 0
        assert d.items(0, [(0, 1, -1), (0, 2, 0)]) == (0, 2) and d.count(D) == 2
        assert d.memory() == before + 2 * slot
        assert d.fields(D, 0) == d.fields(0, 1) and d.fields(D, 1) == d.fields(0, 2), "a derived frame reports its source's values"
        for mode, bad in ((0, (D, 0, 0)), (0, (0, n, 0)), (1, (0, 0, 1)), (1, (0, 0, -1)), (2, (0, 0, 2)), (3, (0, 0, 0))):
            assert d.items(mode, [(0, 0, 0), bad]) == (EINVAL, -7) and d.count(D) == 2, (mode, bad)
        assert d.items(2, [(0, 0, 1)]) == (0, 1) and d.count(D) == 1 and d.memory() == before + 2 * slot  # replaced; the arena is kept
        k = ctypes.c_int32(-1)
        assert host.h264mi_batch_deinterlace(d.h, -1, 0, 2, ctypes.byref(k)) == 0 and k.value == 2 * n == d.count(D)
        assert d.memory() == before + 2 * n * slot
        assert host.h264mi_batch_deinterlace(d.h, 0, 1, 2, ctypes.byref(k)) == EINVAL and host.h264mi_batch_deinterlace(d.h, D, 0, 1, ctypes.byref(k)) == EINVAL
        assert d.count(D) == 2 * n
        assert d.items(0, []) == (0, 0) and d.count(D) == 0  # n = 0 empties it
        assert d.items(1, [(0, 0, 0)]) == (0, 1)
        assert host.h264mi_batch_execute(d.h) == 0 and d.count(D) == 0, "emptied by execute"
        assert d.items(1, [(0, 0, 0)]) == (0, 1)
        assert host.h264mi_stream_reset(d.h, 0) == 0 and d.count(D) == 0 and d.count(0) == 0, "emptied by a stream reset"
        d.decode()
        assert d.items(1, [(0, 0, 0)]) == (0, 1)
        assert host.h264mi_decoder_reset(d.h) == 0 and d.count(D) == 0, "emptied by a decoder reset"
        assert d.memory() == before + 2 * n * slot
    finally:
        d.close()


@pytest.mark.parametrize("name", ["idr_second_cavlc_refs2_idc0", "first_field_cavlc_refs3_idc2"])
def test_host_frame_fields_of_a_frame_that_lost_a_field(name, host, sg, H):
    """A frame that went out with one field missing is field_coded 1, both counts are the count of the field there is, and that field's parity is the
    first: lost second (bottom) fields, and lost first (top) fields whose survivor is taken for a first field."""
    import concealutil4 as c4
    kw, stream, lone = c4.build_case(name, sg)
    whole = Host(host, H, stream, kw)
    d = Host(host, H, lone.damaged, kw)
    try:
        assert d.count() == kw["frames"] == len(lone.frames)
        hit = 0
        for f, fr in enumerate(lone.frames):
            fc, first, top, bot = d.fields(0, f)
            want = whole.fields(0, f)
            if not fr["inserted"]:
                assert (fc, first, top, bot) == want, (name, f)
                continue
            (lost,) = [i["parity"] for i in fr["inserted"]]
            assert (fc, first) == (1, 1 - lost) and top == bot == want[2 + (1 - lost)], (name, f, top, bot, want)
            hit += 1
        assert hit == 2
    finally:
        d.close()
        whole.close()
