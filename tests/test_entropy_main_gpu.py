"""The pictures of k_entropy_m, the Main build of the I/P entropy kernel (CABAC, no 8x8 transform, 4:2:0 as constants), and of its neighbours on
the other two routes: each Main-eligible recipe decoded alone (level 0 on k_entropy_m), in one batch with a stream that has the 8x8 transform
switched on (level 0 on k_entropy_c) and in one batch with a CAVLC stream (level 0 on k_entropy), against the generator's reconstruction, bit
for bit -- there is no tolerance anywhere in this file.  QCIF and smaller, 2 .. 10 pictures.  (Budget, spill tables and the routing rule itself:
test_entropy_main_kernel.py, without a GPU.)"""
import ctypes

import numpy as np
import pytest

from conftest import FIELD_CABAC_MATRIX, MATRIX, pictures_of

MAIN_CASES = ("cabac_I", "cabac_IPP", "pcm_qpjitter_cabac", "slices_idc_cycle", "multiref_cabac", "sub8x8_heavy", "slice_qp_delta")
GENERAL, FMO, CABAC, MAIN = 0, 1, 2, 3
_gen_cache = {}


def _gen(sg, name, matrix=MATRIX):
    """(stream, rec) of a matrix recipe, generated once per run and left unchanged"""
    if name not in _gen_cache:
        stream, rec, _ = sg.encode(**matrix[name])
        rec.setflags(write=False)
        _gen_cache[name] = (stream, rec)
    return _gen_cache[name]


def _main_eligible(kw):
    """CABAC on, the 8x8 transform off (no recipe switches it on without saying so), not monochrome, no slice groups"""
    return kw["cabac"] == 1 and not kw.get("transform8x8", 0) and not kw.get("mono", 0) and kw.get("slice_groups", 1) <= 1


def _nslices(kw):
    return max(1, kw.get("slices", 1)) * max(1, kw.get("slice_groups", 1))


def _route(H, kws):
    """the kernel level 0 of a batch of these streams runs on, by the library's own rule (B pictures are not in level 0)"""
    f4 = H.load_hooks().h264mi_internal_entropy_kernel_choice4
    I32 = ctypes.c_int32
    f4.restype, f4.argtypes = I32, [I32, I32, I32, I32]
    n = [0, 0]
    n_t8x8_mono = 0
    for kw in kws:
        n[kw["cabac"]] += pictures_of(kw) * _nslices(kw)
        if kw.get("transform8x8", 0) or kw.get("mono", 0):
            n_t8x8_mono += pictures_of(kw)
    return f4(n[1], n[0], int(any(kw.get("slice_groups", 1) > 1 for kw in kws)), n_t8x8_mono)


def _decode(H, items, **cfg):
    """items: [(kw, stream)] decoded as ONE batch; per stream its frames, uncropped (every size here is a multiple of 16)"""
    W = max((kw["width"] + 15) & ~15 for kw, _ in items)
    Hc = max((kw["height"] + 15) & ~15 for kw, _ in items)
    dec = H.Decoder(max_streams=len(items), max_width=W, max_height=Hc, max_frames_per_batch=max(pictures_of(kw) for kw, _ in items),
                    max_slices_per_frame=max(_nslices(kw) for kw, _ in items), max_bitstream_bytes=sum(len(s) for _, s in items) * 2 + (1 << 20), **cfg)
    try:
        dec.decode([s for _, s in items])
        return [dec.read_frames(i, crop=True, size=kw["width"] * kw["height"] * 3 // 2) for i, (kw, _) in enumerate(items)]
    finally:
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", MAIN_CASES)
def test_gpu_three_routes_give_the_same_pictures(name, H, sg):
    kw = MATRIX[name]
    assert _main_eligible(kw) and kw["width"] <= 176 and kw["height"] <= 144 and 2 <= kw["frames"] <= 6
    stream, rec = _gen(sg, name)
    t8_kw, cav_kw = MATRIX["high8x8_cabac"], MATRIX["cavlc_I"]
    assert t8_kw["cabac"] == 1 and t8_kw["transform8x8"] == 1 and cav_kw["cabac"] == 0
    assert _route(H, [kw]) == MAIN and _route(H, [kw, t8_kw]) == CABAC and _route(H, [kw, cav_kw]) == GENERAL
    t8, t8_rec = _gen(sg, "high8x8_cabac")
    cav, cav_rec = _gen(sg, "cavlc_I")
    alone = _decode(H, [(kw, stream)])                      # level 0: k_entropy_m
    assert alone[0].shape == rec.shape and np.array_equal(alone[0], rec), "k_entropy_m != generator reconstruction"
    with8 = _decode(H, [(kw, stream), (t8_kw, t8)])         # one stream with the 8x8 transform in the batch: k_entropy_c
    assert np.array_equal(with8[0], rec), "k_entropy_c != generator reconstruction"
    assert np.array_equal(with8[1], t8_rec), "the 8x8 stream of the mixed batch"
    mixed = _decode(H, [(kw, stream), (cav_kw, cav)])       # one CAVLC slice in the launch: k_entropy
    assert np.array_equal(mixed[0], rec), "k_entropy != generator reconstruction"
    assert np.array_equal(mixed[1], cav_rec), "the CAVLC stream of the mixed batch"


@pytest.mark.gpu
def test_gpu_level0_on_the_main_kernel_with_b_slices_behind_it(H, sg):
    kw = MATRIX["b_ibbp_cabac"]
    assert _main_eligible(kw)
    stream, rec = _gen(sg, "b_ibbp_cabac")
    out = _decode(H, [(kw, stream)])
    assert out[0].shape == rec.shape and np.array_equal(out[0], rec)


@pytest.mark.gpu
def test_gpu_field_cabac_on_request_through_the_main_kernel(H, sg):
    """the field scan and the field significance contexts of 4x4 blocks are selected per picture inside the same source"""
    kw = FIELD_CABAC_MATRIX["field_IP_cabac"]
    assert _main_eligible(kw) and _route(H, [kw]) == MAIN
    stream, rec = _gen(sg, "field_IP_cabac", FIELD_CABAC_MATRIX)
    out = _decode(H, [(kw, stream)], allow_unpinned_field_cabac=1)
    assert out[0].shape == rec.shape and np.array_equal(out[0], rec)


@pytest.mark.gpu
def test_gpu_damaged_slice_ends_the_main_kernel_in_order(H, sg):
    """One byte of the second picture's slice data flipped, no concealment, both streams of the batch Main-eligible: the call returns, the
    stream's status is 0 (the damage decoded as something) or H264MI_ECORRUPT (-8), the intact stream beside it is exact."""
    kw, good_kw = MATRIX["cabac_IPP"], MATRIX["cabac_I"]
    assert _main_eligible(kw) and _main_eligible(good_kw) and _route(H, [kw, good_kw]) == MAIN
    stream, rec = _gen(sg, "cabac_IPP")
    nals = H.read_nal_units(stream)
    slices = [i for i, n in enumerate(nals) if n.Type in (1, 5)]
    second = slices[1]
    begin = nals[second].Offset
    end = nals[second + 1].Offset - 4 if second + 1 < len(nals) else len(stream)
    assert end - begin > 64
    b = bytearray(stream)
    b[begin + (end - begin) // 2] ^= 0xFF
    good, good_rec = _gen(sg, "cabac_I")
    dec = H.Decoder(max_streams=2, max_width=176, max_height=144, max_frames_per_batch=kw["frames"], max_bitstream_bytes=1 << 20)
    try:
        dec.set_isolation(True)
        dec.decode([bytes(b), good])
        status = dec.stream_status(0)
        print("status of the damaged stream: %d" % status)
        assert status in (0, -8)
        assert dec.stream_status(1) == 0
        assert np.array_equal(dec.read_frames(1, crop=True, size=good_kw["width"] * good_kw["height"] * 3 // 2), good_rec)
        assert np.array_equal(dec.read_frames(0, crop=False)[0], rec[0]), "the intact first picture of the damaged stream"
    finally:
        dec.close()
