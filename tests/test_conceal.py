"""Error concealment (h264mi_config.conceal_errors): lost and damaged slices of non-IDR frame pictures are reconstructed as a zero-motion copy of
entry 0 of the picture's initial P list, the picture stays a reference, the stream goes on.  The yardstick is the oracle's decode of the REPAIRED
stream (tests/concealutil.py); every GPU comparison is bit-exact."""
import ctypes
import os
import re

import numpy as np
import pytest

import concealutil as cu
from concealutil import CONCEAL_MATRIX
from conftest import FULL_MATRIX, pictures_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- CPU: the writer and the rule, independent of the product's device code
@pytest.mark.parametrize("name", sorted(CONCEAL_MATRIX))
def test_repaired_stream_is_a_valid_stream(name, sg, oracle_mod):
    """The oracle decodes the repaired stream without error, with the frame count and PicOrderCnt list of the original; the damage meets the
    conditions of the matrix (concealutil.check_picks) in both modes; pictures before the first damaged one are untouched."""
    kw = CONCEAL_MATRIX[name]
    assert kw["width"] >= 176 and kw["height"] >= 144
    assert kw["idr_period"] == 0 and 8 <= kw["frames"] <= 12 and 3 <= cu.nslices(kw) <= 4
    stream, rec, _ = sg.encode(**kw)
    ref, info = oracle_mod.decode(stream, crop=False)
    pocs = list(oracle_mod.last_pocs)
    for mode in ("lost", "damaged"):
        damaged, repaired, per_picture, n = cu.make(stream, mode=mode)
        assert damaged != stream and repaired != stream and n >= 3
        out, info2 = oracle_mod.decode(repaired, crop=False)
        assert info2.n_frames == info.n_frames == kw["frames"]
        assert list(oracle_mod.last_pocs) == pocs
        first = min(p for p, c in enumerate(per_picture) if c)
        assert np.array_equal(out[:first], ref[:first])
        assert not np.array_equal(out[first], ref[first])


@pytest.mark.parametrize("name", [n for n in sorted(CONCEAL_MATRIX) if CONCEAL_MATRIX[n].get("deblock_idc") == 1])
def test_replaced_macroblocks_are_a_copy_of_the_concealment_reference(name, sg, oracle_mod):
    """deblock_idc 1: the intact slices filter nothing, the replaced slices carry idc 0.  A replaced macroblock whose left and upper neighbours
    are replaced too (or outside the picture) equals the co-located samples of the concealment reference; the others differ from the copy only
    through the filter of their own left / top edge (three luma, one chroma sample deep).  These cases keep one reference frame and no
    non-reference pictures, so the concealment reference of a picture is the picture decoded before it."""
    kw = CONCEAL_MATRIX[name]
    assert sg.default_params(**kw).num_ref_frames == 1 and not kw.get("bframes") and not kw.get("nonref_period")
    stream, _, _ = sg.encode(**kw)
    _, repaired, _, _ = cu.make(stream)
    out, info = oracle_mod.decode(repaired, crop=False)
    lost, (wmb, hmb) = cu.lost_mbs(stream)
    W, Hh = wmb * 16, hmb * 16

    def planes(f):
        return f[:W * Hh].reshape(Hh, W), f[W * Hh:W * Hh * 5 // 4].reshape(Hh // 2, W // 2), f[W * Hh * 5 // 4:].reshape(Hh // 2, W // 2)
    n_full = n_edge = 0
    for p, mbs in lost.items():
        cur, prev = planes(out[p]), planes(out[p - 1])
        s = set(mbs)
        for a in mbs:
            x, y = a % wmb, a // wmb
            inner = (x == 0 or a - 1 in s) and (y == 0 or a - wmb in s)
            ky, kc = (0, 0) if inner else (3, 1)
            n_full += inner
            n_edge += not inner
            assert np.array_equal(cur[0][16 * y + ky:16 * y + 16, 16 * x + ky:16 * x + 16], prev[0][16 * y + ky:16 * y + 16, 16 * x + ky:16 * x + 16]), (p, a)
            for c in (1, 2):
                assert np.array_equal(cur[c][8 * y + kc:8 * y + 8, 8 * x + kc:8 * x + 8], prev[c][8 * y + kc:8 * y + 8, 8 * x + kc:8 * x + 8]), (p, a, c)
    assert n_full > 20 and n_edge > 5


def test_abi_has_the_switch_and_the_counters(H):
    """h264mi_config ends in conceal_errors, the two calls are declared, exported and bound, the Go binding carries them."""
    from h264decode_amd import _lib
    names = [f for f, _ in _lib.Config._fields_]
    assert names[-1] == "conceal_errors" and names[-2] == "allow_unpinned_field_cabac"
    assert ctypes.sizeof(_lib.Config) >= _lib.Config.conceal_errors.offset + 4
    L = H.lib()
    header = open(os.path.join(ROOT, "include", "h264mi.h")).read()
    for sym in ("h264mi_frame_concealed", "h264mi_decoder_concealed"):
        assert hasattr(L, sym) and sym in _lib.EXPORTS
        assert re.search(r"int32_t %s\(" % sym, header)
    go = open(os.path.join(ROOT, "go", "h264", "h264mi.go")).read()
    assert "ConcealErrors" in go and "conceal_errors:" in go and "C.h264mi_frame_concealed(" in go and "C.h264mi_decoder_concealed(" in go
    assert "conceal_errors" in open(os.path.join(ROOT, "examples", "h264mi_decode.c")).read()
    # the counters answer without a device too: argument checks come first
    assert L.h264mi_decoder_concealed(None, None, None) == -1
    assert L.h264mi_frame_concealed(None, 0, 0, None) == -1


# ---------------------------------------------------------------- GPU
class _x_wgs:
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.old = os.environ.get("H264MI_X_WGS")
        if self.n is not None:
            os.environ["H264MI_X_WGS"] = str(self.n)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("H264MI_X_WGS", None)
        else:
            os.environ["H264MI_X_WGS"] = self.old


def _decoder(H, kw, streams, frames=None, **cfg):
    W, Hc = (kw["width"] + 15) // 16 * 16, (kw["height"] + 15) // 16 * 16
    return H.Decoder(max_streams=len(streams), max_width=W, max_height=Hc, max_frames_per_batch=frames or pictures_of(kw), max_slices_per_frame=max(cu.nslices(kw), 1),
                     max_bitstream_bytes=sum(len(s) for s in streams) * 2 + (1 << 20), **cfg)


def _check_concealed(H, oracle_mod, kw, stream, mode):
    damaged, repaired, per_picture, n_slices = cu.make(stream, mode=mode)
    want, _ = oracle_mod.decode(repaired, crop=False)
    want_pocs = list(oracle_mod.last_pocs)
    for x in (None, 0, 512):
        with _x_wgs(x):
            dec = _decoder(H, kw, [damaged], conceal_errors=True)
            try:
                dec.decode([damaged])
                if mode == "damaged":  # precondition: the entropy kernels reported every damaged slice (otherwise the DAMAGE is at fault, not the feature)
                    assert dec.concealed()[0] == n_slices, "damage not detected: %r" % (dec.concealed(),)
                assert dec.stream_status(0) == 0
                assert dec.frame_count(0) == kw["frames"]
                out = dec.read_frames(0, crop=False)
                bad = [i for i in range(len(want)) if not np.array_equal(out[i], want[i])]
                assert not bad, "frames %r differ from the oracle's decode of the repaired stream (H264MI_X_WGS=%r)" % (bad, x)
                assert [dec.frame_info(0, f).pic_order_cnt for f in range(kw["frames"])] == want_pocs
                assert [dec.frame_concealed(0, f) for f in range(kw["frames"])] == per_picture
                assert dec.concealed() == (0 if mode == "lost" else n_slices, sum(per_picture))
            finally:
                dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CONCEAL_MATRIX))
def test_gpu_lost_slices_are_concealed(name, H, sg, oracle_mod):
    kw = CONCEAL_MATRIX[name]
    _check_concealed(H, oracle_mod, kw, sg.encode(**kw)[0], "lost")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CONCEAL_MATRIX))
def test_gpu_damaged_slices_are_concealed(name, H, sg, oracle_mod):
    kw = CONCEAL_MATRIX[name]
    _check_concealed(H, oracle_mod, kw, sg.encode(**kw)[0], "damaged")


@pytest.mark.gpu
def test_gpu_slices_with_unparsable_headers_are_lost_slices(H, sg, oracle_mod):
    """A slice NAL unit whose header does not parse is dropped and counted instead of failing the stream."""
    kw = CONCEAL_MATRIX["cabac_idc0_offsets_cqp"]
    _check_concealed(H, oracle_mod, kw, sg.encode(**kw)[0], "header")


def _access_units(stream):
    """The stream cut in front of every picture's first unit (parameter sets stay with the picture they precede)."""
    units, slices, pics = cu.parse(stream)
    first_unit = sorted(min(s.unit for s in p) for p in pics)
    cuts = [0]
    for u in first_unit[1:]:
        while u > 0 and (units[u - 1][cu._sc_len(units[u - 1])] & 31) in (7, 8):
            u -= 1
        cuts.append(u)
    cuts.append(len(units))
    return [b"".join(units[a:b]) for a, b in zip(cuts, cuts[1:])]


@pytest.mark.gpu
def test_gpu_several_streams_pipelined(H, sg, oracle_mod):
    """Four streams, one of them damaged, two batches as execute; prepare; execute; sync with the damage in the first: every stream equals its
    oracle result in both batches, the damaged one goes on in the second batch without an IDR picture."""
    names = ["cabac_wp1_multiref", "cavlc_idc2_offsets", "b_ibbp_cabac_implicit", "cabac_idc0_offsets_cqp"]
    kws = [dict(CONCEAL_MATRIX[n], frames=10) for n in names]
    streams = [sg.encode(**kw)[0] for kw in kws]
    damaged, repaired, per_picture, n_slices = cu.make(streams[0], mode="damaged")
    assert not any(per_picture[5:])
    want = [oracle_mod.decode(repaired if i == 0 else s, crop=False)[0] for i, s in enumerate(streams)]
    feed = [damaged] + streams[1:]
    aus = [_access_units(s) for s in feed]
    assert all(len(a) == 10 for a in aus)
    halves = [[b"".join(a[:5]) for a in aus], [b"".join(a[5:]) for a in aus]]
    dec = H.Decoder(max_streams=4, max_width=176, max_height=144, max_frames_per_batch=5, max_slices_per_frame=4, max_bitstream_bytes=1 << 21, conceal_errors=True)
    try:
        dec.prepare(halves[0])
        dec.execute()
        dec.prepare(halves[1])
        dec.execute()
        dec.sync()
        for i in range(4):
            assert dec.stream_status(i) == 0
            assert dec.frame_count(i) == 5
            assert np.array_equal(dec.read_frames(i, crop=False), want[i][5:]), "stream %d, second batch" % i
        assert dec.concealed() == (n_slices, sum(per_picture))
    finally:
        dec.close()
    # the first batch on its own (the frames of batch k are readable until the next prepare)
    dec = H.Decoder(max_streams=4, max_width=176, max_height=144, max_frames_per_batch=5, max_slices_per_frame=4, max_bitstream_bytes=1 << 21, conceal_errors=True)
    try:
        dec.decode(halves[0])
        for i in range(4):
            assert np.array_equal(dec.read_frames(i, crop=False), want[i][:5]), "stream %d, first batch" % i
        assert [dec.frame_concealed(0, f) for f in range(5)] == per_picture[:5]
        dec.decode(halves[1])
        for i in range(4):
            assert np.array_equal(dec.read_frames(i, crop=False), want[i][5:]), "stream %d, second batch" % i
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_clean_streams_with_the_switch_on(H, sg):
    """Every case of the parity matrix, field pictures included, decodes exactly and reports nothing concealed."""
    for name in sorted(FULL_MATRIX):
        kw = FULL_MATRIX[name]
        stream, rec, _ = sg.encode(**kw)
        dec = _decoder(H, kw, [stream], conceal_errors=True)
        try:
            dec.decode([stream])
            assert np.array_equal(dec.read_frames(0, crop=False), rec), name
            assert dec.concealed() == (0, 0), name
            assert all(dec.frame_concealed(0, f) == 0 for f in range(dec.frame_count(0))), name
        finally:
            dec.close()


def _status(H, kw, stream, conceal):
    dec = _decoder(H, kw, [stream], conceal_errors=conceal)
    try:
        code = 0
        try:
            dec.decode([stream])
        except H.H264MIError as e:
            code = e.code
        return code, dec.stream_status(0), dec.concealed()
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_not_concealable_stays_as_it_is(H, sg):
    """Damage in the IDR picture, and in a field picture: the same error and status with the switch on as with it off."""
    kw = CONCEAL_MATRIX["cavlc_idc2_offsets"]
    stream = sg.encode(**kw)[0]
    damaged, _, _, _ = cu.make(stream, [(0, 1)], mode="damaged", repair=False)
    off, on = _status(H, kw, damaged, False), _status(H, kw, damaged, True)
    assert off[0] == -8 and off[1] == -8 and on[:2] == off[:2] and on[2] == (0, 0)
    kwf = dict(width=176, height=128, frames=5, idr_period=0, profile_idc=77, cabac=0, field_pics=1, slices=3, num_ref_frames=2, seed=306)
    stream = sg.encode(**kwf)[0]
    damaged, _, _, _ = cu.make(stream, [(2, 1)], mode="damaged", repair=False)
    off, on = _status(H, kwf, damaged, False), _status(H, kwf, damaged, True)
    assert off[0] == -8 and off[1] == -8 and on[:2] == off[:2] and on[2] == (0, 0)
    # a slice header that does not parse is tolerated as a lost slice only in a concealable picture: in a field picture (a middle slice, and the
    # first slice, which is decided when the picture's next slice starts it) it fails the stream as with the switch off
    for place in (1, 0):
        damaged, _, _, _ = cu.make(stream, [(2, place)], mode="header", repair=False)
        off, on = _status(H, kwf, damaged, False), _status(H, kwf, damaged, True)
        assert off[0] == -2 and off[1] == -2 and on[:2] == off[:2] and on[2] == (0, 0), (place, off, on)


@pytest.mark.gpu
def test_gpu_c_program_with_conceal(H, sg, oracle_mod, tmp_path):
    """examples/h264mi_decode.c --conceal: the damaged stream decodes to the oracle's pictures of the repaired one, and the program reports the totals."""
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    kw = CONCEAL_MATRIX["cabac_idc0_offsets_cqp"]
    damaged, repaired, per_picture, n_slices = cu.make(sg.encode(**kw)[0], mode="damaged")
    want, info = oracle_mod.decode(repaired, crop=True)
    src, dst = tmp_path / "in.h264", tmp_path / "out.yuv"
    src.write_bytes(damaged)
    p = subprocess.run([os.path.join(ROOT, "examples", "h264mi_decode"), str(src), str(dst), "3", "--conceal"], stderr=subprocess.PIPE, check=True)
    got = np.frombuffer(dst.read_bytes(), dtype=np.uint8).reshape(-1, info.width * info.height * 3 // 2)
    assert np.array_equal(got, want)
    assert ("concealed: %d slices, %d macroblocks" % (n_slices, sum(per_picture))) in p.stderr.decode()


@pytest.mark.gpu
def test_gpu_switch_off_fails_as_before(H, sg):
    kw = CONCEAL_MATRIX["cavlc_idc2_offsets"]
    damaged, _, _, _ = cu.make(sg.encode(**kw)[0], mode="damaged")
    dec = _decoder(H, kw, [damaged])
    try:
        with pytest.raises(H.H264MIError) as e:
            dec.decode([damaged])
        assert e.value.code == -8
        assert dec.concealed() == (0, 0)
    finally:
        dec.close()
