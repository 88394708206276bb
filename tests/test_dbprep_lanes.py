"""k_dbprep_ip, the one-lane-per-macroblock kernel for launches of I / P pictures (k_dbprep.hip), against k_dbprep and the oracle.

Every GPU case decodes a short generator stream and asserts three things: (a) the frames equal the oracle's bit for bit, (b) the hook
h264mi_internal_dbprep_check -- k_dbprep run once more over the same records into scratch buffers -- finds no byte of a DbPrm record or of the
intra mask that differs, (c) the pass launched k_dbprep_ip and never k_dbprep.  One I B B P stream asserts the opposite of (c).  There is no
tolerance anywhere in this file.

Every case runs three times: with the strip height the launch rule gives (single rows for batches this small), with strips of two rows and
with whole columns (test hook h264mi_internal_set_dbprep_rows).

Sizes: one macroblock; 5 x 3 macroblocks (row changes inside one 64-lane iteration); 64 x 2 (a row is exactly one iteration); 65 x 3 (the left
neighbour across the iteration boundary, the upper neighbour in another iteration); field pictures of 64 x 1 and 5 x 3 macroblocks."""
import ctypes

import numpy as np
import pytest

from conftest import pictures_of

P = dict(idr_period=0, frames=4)
CASES = {
    # 16 x 16: one macroblock
    "mb1_cabac_intra_pcm": dict(P, width=16, height=16, profile_idc=77, cabac=1, intra_in_p_permille=300, pcm_permille=100, qp_jitter=4, seed=701),
    "mb1_cavlc_idc1": dict(P, width=16, height=16, profile_idc=66, cabac=0, deblock_idc=1, seed=702),
    # 80 x 48: 5 x 3
    "w5_cabac_slices_idc2_qp": dict(P, width=80, height=48, profile_idc=77, cabac=1, slices=3, deblock_idc=2, chroma_qp_offset=3, slice_qp_delta=4,
                                    sub8x8_permille=600, seed=703),
    "w5_cavlc_slices_idc1": dict(P, width=80, height=48, profile_idc=66, cabac=0, slices=3, deblock_idc=1, intra_in_p_permille=150, seed=704),
    "w5_cabac_multiref_rplm": dict(P, frames=5, width=80, height=48, profile_idc=77, cabac=1, num_ref_frames=3, rplm=1, intra_in_p_permille=150,
                                   pcm_permille=40, sub8x8_permille=400, alpha_off_div2=2, beta_off_div2=-1, seed=705),
    "w5_cavlc_mono_8x8": dict(P, width=80, height=48, profile_idc=100, cabac=0, mono=1, transform8x8=1, intra_in_p_permille=200, seed=706),
    # 1024 x 32: 64 x 2
    "w64_cabac_8x8_sub8x8": dict(P, frames=3, width=1024, height=32, profile_idc=100, cabac=1, transform8x8=1, sub8x8_permille=500, qp_jitter=3, seed=707),
    "w64_cavlc_slices_idc2": dict(P, frames=3, width=1024, height=32, profile_idc=66, cabac=0, slices=3, deblock_idc=2, chroma_qp_offset=-2,
                                  slice_qp_delta=-3, intra_in_p_permille=100, seed=708),
    "w64_field_cavlc": dict(P, frames=3, width=1024, height=32, profile_idc=77, cabac=0, field_pics=1, sub8x8_permille=300, seed=709),
    # 1040 x 48: 65 x 3
    "w65_cabac_all": dict(P, frames=3, width=1040, height=48, profile_idc=77, cabac=1, slices=3, deblock_idc=2, num_ref_frames=3, rplm=1, sub8x8_permille=600,
                          intra_in_p_permille=120, pcm_permille=30, chroma_qp_offset=4, slice_qp_delta=3, qp_jitter=4, seed=710),
    "w65_cavlc_8x8_multiref": dict(P, frames=4, width=1040, height=48, profile_idc=100, cabac=0, transform8x8=1, num_ref_frames=3, rplm=1,
                                   sub8x8_permille=400, intra_in_p_permille=100, alpha_off_div2=-2, beta_off_div2=3, seed=711),
    "w65_cabac_mono": dict(P, frames=3, width=1040, height=48, profile_idc=100, cabac=1, mono=1, transform8x8=1, pcm_permille=30, seed=712),
    # field pictures of 5 x 3 macroblocks: bS 3 on horizontal macroblock edges, the vertical vector limit 2
    "w5_field_cavlc": dict(P, width=80, height=96, profile_idc=77, cabac=0, field_pics=1, num_ref_frames=2, sub8x8_permille=400, intra_in_p_permille=150, seed=713),
}
# one slice of every picture lost, concealment off: MBT_NONE records (IDR pictures only and no deblocking across slice edges, so that the
# oracle -- which starts every picture mid-grey -- reconstructs the same frames from the same damaged stream)
LOST = dict(width=80, height=48, frames=3, idr_period=1, profile_idc=77, cabac=1, slices=3, deblock_idc=2, seed=714)
IBBP = dict(width=80, height=48, frames=7, idr_period=0, profile_idc=77, cabac=1, bframes=2, num_ref_frames=3, seed=715)

_cache = {}


def _case(sg, oracle_mod, name, kw, damage=None):
    """(stream, the oracle's frames) of a recipe: generated and decoded once per run, shared, read-only"""
    if name not in _cache:
        stream, rec, _ = sg.encode(**kw)
        if damage:
            stream = damage(stream)
        ref, _ = oracle_mod.decode(stream, crop=False)
        if not damage:
            assert np.array_equal(ref, rec), "oracle != generator reconstruction"
        ref.setflags(write=False)
        _cache[name] = (stream, ref)
    return _cache[name]


def _drop_middle_slices(stream):
    import concealutil
    damaged, _, per_picture, n = concealutil.make(stream, picks=[(0, 1), (1, 1), (2, 1)], mode="lost", check=False, repair=False)
    assert n == 3 and all(per_picture)
    return damaged


def _nslices(kw):
    return max(1, kw.get("slices", 1))


# macroblock rows per wavefront of k_dbprep_ip: the rule (single rows for batches this small: every row loads its upper neighbours), strips of two
# rows (the upper neighbour from the wavefront's registers in every second row, a last strip of one row in pictures of three), whole columns
ROWS = (0, 2, 1000)


def _decode_and_check(H, kw, stream, rows=0):
    """frames of the stream decoded as one batch, and what the hook says about that pass: (frames, launches_ip, launches_generic, mismatching_bytes)"""
    W, Hc = (kw["width"] + 15) & ~15, (kw["height"] + 15) & ~15
    dec = H.Decoder(max_streams=1, max_width=W, max_height=Hc, max_frames_per_batch=pictures_of(kw), max_slices_per_frame=_nslices(kw),
                    max_bitstream_bytes=len(stream) * 2 + (1 << 20))
    try:
        assert H.load_hooks().h264mi_internal_set_dbprep_rows(dec._h, rows) == 0
        dec.decode([stream])
        out = dec.read_frames(0, crop=False, size=W * Hc * 3 // 2)
        ip, gen, bad = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
        assert H.load_hooks().h264mi_internal_dbprep_check(dec._h, ctypes.byref(ip), ctypes.byref(gen), ctypes.byref(bad)) == 0
        return out, ip.value, gen.value, bad.value
    finally:
        dec.close()


def test_dbprep_kernel_choice(H):
    f = H.load_hooks().h264mi_internal_dbprep_kernel_choice
    GENERIC, IP = 0, 1
    assert f(0, 0) == IP                                  # I / P pictures that leave no ColRec array
    assert f(1, 0) == GENERIC and f(30, 0) == GENERIC     # one picture with B slices is enough
    assert f(0, 1) == GENERIC and f(0, 255) == GENERIC    # one picture whose motion is kept
    assert f(3, 2) == GENERIC


def test_dbprep_ip_rows_rule(H):
    """mi_dbprep_ip_rows: whole columns once the launch has 8192 wavefronts without cutting them, single rows for a lone picture, and always
    1 <= rows <= hmb with ceil(hmb / rows) strips covering the picture"""
    f = H.load_hooks().h264mi_internal_dbprep_ip_rows
    assert f(7680, 120, 68) == 68          # the bench: 7680 pictures x 2 chunks of columns
    assert f(4096, 120, 68) == 68 and f(8192, 64, 68) == 68
    assert f(1, 120, 68) == 1 and f(8, 120, 68) == 1
    assert f(256, 120, 68) == 5            # 512 columns: 16 strips each
    for n, w, h in ((1, 1, 1), (3, 5, 3), (100, 65, 3), (5000, 1, 2), (300, 512, 320), (100000, 120, 68)):
        r = f(n, w, h)
        assert 1 <= r <= h, (n, w, h, r)
        chunks = (w + 63) // 64
        strips = -(-h // r)
        assert strips * r >= h and (strips == 1 or n * chunks * (strips - 1) < 8192), (n, w, h, r)


def test_recipes_cover_what_the_kernel_distinguishes():
    """the options the cases switch on, so that a recipe edited later cannot quietly lose one"""
    ks = list(CASES.values())
    for w, h in ((16, 16), (80, 48), (1024, 32), (1040, 48)):
        assert any(k["width"] == w and k["height"] == h for k in ks), (w, h)
    assert any(k["cabac"] for k in ks) and any(not k["cabac"] for k in ks)
    assert any(k.get("slices") == 3 and k.get("deblock_idc") == 2 for k in ks) and any(k.get("deblock_idc") == 1 for k in ks)
    assert any(k.get("chroma_qp_offset") and k.get("slice_qp_delta") for k in ks)
    assert any(k.get("sub8x8_permille", 0) >= 500 for k in ks)
    assert any(k.get("num_ref_frames") == 3 and k.get("rplm") for k in ks)
    assert any(k.get("intra_in_p_permille") and k.get("pcm_permille") for k in ks)
    assert any(k.get("transform8x8") for k in ks) and any(k.get("mono") for k in ks)
    assert any(k.get("field_pics") == 1 and not k["cabac"] for k in ks)
    assert all(3 <= k["frames"] <= 5 for k in ks)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_lane_kernel_writes_what_k_dbprep_writes(name, H, sg, oracle_mod):
    kw = CASES[name]
    stream, ref = _case(sg, oracle_mod, name, kw)
    for rows in ROWS:
        out, ip, gen, bad = _decode_and_check(H, kw, stream, rows)
        print("%s, rows %d: launches k_dbprep_ip %d, k_dbprep %d, mismatching bytes %d" % (name, rows, ip, gen, bad))
        assert out.shape == ref.shape and np.array_equal(out, ref), "GPU != oracle (rows %d)" % rows
        assert bad == 0, "rows %d: %d bytes of the DbPrm records / intra mask differ from k_dbprep's" % (rows, bad)
        assert ip > 0 and gen == 0, "the pass did not run on k_dbprep_ip alone"


@pytest.mark.gpu
def test_gpu_lane_kernel_with_undelivered_macroblocks(H, sg, oracle_mod):
    stream, ref = _case(sg, oracle_mod, "lost", LOST, _drop_middle_slices)
    for rows in ROWS:
        out, ip, gen, bad = _decode_and_check(H, LOST, stream, rows)
        print("lost, rows %d: launches k_dbprep_ip %d, k_dbprep %d, mismatching bytes %d" % (rows, ip, gen, bad))
        W = 80
        assert (out[:, 16 * W:32 * W] == 128).all(), "the lost macroblock row is not mid-grey: no MBT_NONE records in this case"
        assert out.shape == ref.shape and np.array_equal(out, ref), "GPU != oracle (rows %d)" % rows
        assert bad == 0
        assert ip > 0 and gen == 0


@pytest.mark.gpu
def test_gpu_pictures_with_b_slices_stay_on_k_dbprep(H, sg, oracle_mod):
    stream, ref = _case(sg, oracle_mod, "ibbp", IBBP)
    out, ip, gen, bad = _decode_and_check(H, IBBP, stream)
    print("ibbp: launches k_dbprep_ip %d, k_dbprep %d, mismatching bytes %d" % (ip, gen, bad))
    assert out.shape == ref.shape and np.array_equal(out, ref), "GPU != oracle"
    assert bad == 0
    assert gen > 0 and ip == 0, "a batch whose levels all hold B pictures or pictures that keep their motion runs on k_dbprep"
