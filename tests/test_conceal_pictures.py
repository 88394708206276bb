"""Error concealment of wholly lost pictures (h264mi_config.conceal_errors with H264MI_CONCEAL_PICTURES): a frame_num gap in a stream that does not
allow gaps is filled with frames that are copies of entry 0 of their initial P list, the stream goes on.  The yardstick is the oracle's decode of
the REPAIRED stream (tests/concealutil2.py); every GPU comparison is bit-exact."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import concealutil as cu
import concealutil2 as c2
import hostprog
from concealutil2 import CASES, MATRIX_CASES
from conftest import FULL_MATRIX, pictures_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICES, PICTURES, FIELDS = 1, 2, 4  # H264MI_CONCEAL_SLICES, H264MI_CONCEAL_PICTURES, H264MI_CONCEAL_FIELDS
LONG = dict(cu.B, profile_idc=77, cabac=1, slices=1, seed=711)  # one slice per picture; frames set by the tests of the cap (the generator's MaxFrameNum is 256)


def _unpinned(kw):
    return int(bool(kw.get("field_pics") and kw.get("cabac")))


# ---------------------------------------------------------------- CPU: the writer and the rule, independent of the product's device code
@pytest.mark.parametrize("name", sorted(CASES))
def test_repaired_stream_is_a_valid_stream(name, sg, oracle_mod):
    """The oracle refuses the damaged stream for its missing reference pictures and decodes the repaired one: the frame count of the original, the
    frames in front of the first loss untouched, every inserted frame a copy of the reference frame decoded last before it.  The cases of the
    matrix meet its conditions (concealutil2.check_lost)."""
    kw, lost = CASES[name]
    stream, _, _ = sg.encode(**kw)
    ref, info = oracle_mod.decode(stream, crop=False)
    r = c2.lose_pictures(stream, lost)
    with pytest.raises(oracle_mod.OracleError, match="reference pictures are missing"):
        oracle_mod.decode(r.damaged, crop=False)
    out, info2 = oracle_mod.decode(r.repaired, crop=False)
    pocs = list(oracle_mod.last_pocs)
    assert info2.n_frames == info.n_frames == kw["frames"] == len(r.inserted)
    assert np.array_equal(out[:r.first_touched], ref[:r.first_touched])
    assert sum(r.inserted) >= 1
    for i, ins in enumerate(r.inserted):
        if ins:
            assert np.array_equal(out[i], out[r.copy_of[i]]), i
    if name in MATRIX_CASES:
        c2.check_lost(r, pocs)
        if not kw.get("bframes") and not kw.get("nonref_period") and kw.get("poc_type", 0) != 1:
            oracle_mod.decode(stream, crop=False)
            assert pocs == list(oracle_mod.last_pocs)  # P pictures only: even the PicOrderCnt list of the original


def test_the_set_has_the_required_shapes():
    """A loss directly behind the IDR picture, two consecutive losses, one slice per picture, slice groups, both entropy coders, PAFF."""
    assert any(lost[0] == 1 for _, lost in CASES.values())
    assert any(a + 1 == b for _, lost in CASES.values() for a, b in zip(lost, lost[1:]))
    assert sum(kw.get("slices") == 1 for kw, _ in CASES.values()) >= 2
    assert any(kw.get("slice_groups") for kw, _ in CASES.values()) and any(kw.get("field_pics") for kw, _ in CASES.values())
    assert {kw.get("cabac") for kw, _ in CASES.values()} >= {0, 1}
    assert len(MATRIX_CASES) >= 15


@pytest.fixture(scope="module")
def host_pocs(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("host_pocs_conceal")
    return hostprog.build("host_pocs.sh", tmp), tmp


def _host(prog, tmp, stream, kw, conceal, frames=None):
    """The product's host side against the null device: (return code, [(PicOrderCnt, frame_num, nal_ref_idc, idr)] per frame, stderr)."""
    path = os.path.join(str(tmp), "s.h264")
    open(path, "wb").write(stream)
    W, Hc = (kw["width"] + 15) & ~15, (kw["height"] + 15) & ~15
    r = subprocess.run([prog, path, str(W), str(Hc), str(frames or pictures_of(kw)), str(max(8, cu.nslices(kw))), str(conceal), str(_unpinned(kw))],
                       capture_output=True, text=True, timeout=120)
    rows = [tuple(int(x) for x in line.split()[:4]) for line in r.stdout.splitlines() if line.strip() and not line.startswith("order")]
    return r.returncode, rows, r.stderr


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_inserts_the_missing_frames(name, host_pocs, sg, oracle_mod):
    """Picture management alone (no GPU): with value 3 the frame_num / PicOrderCnt list of the damaged stream is the oracle's list for the repaired
    stream, the inserted frames reported as reference frames that are not IDR pictures; with value 1 the stream is refused as ever."""
    prog, tmp = host_pocs
    kw, lost = CASES[name]
    r = c2.lose_pictures(sg.encode(want_recon=False, **kw)[0], lost)
    oracle_mod.decode(r.repaired, crop=False)
    pocs = [int(x) for x in oracle_mod.last_pocs]
    rc, rows, err = _host(prog, tmp, r.damaged, kw, SLICES | PICTURES)
    assert rc == 0, err[-2000:]
    assert [x[0] for x in rows] == pocs
    assert [x[1] for x in rows] == r.frame_num
    assert all(x[2] == 1 and x[3] == 0 for x, ins in zip(rows, r.inserted) if ins)
    for v in (0, SLICES):
        rc, rows, err = _host(prog, tmp, r.damaged, kw, v)
        assert rc == 1 and "reference pictures are missing" in err, (v, err[-500:])


def test_host_cap_and_batch_room(host_pocs, sg):
    """16 consecutive lost frames are inserted, 17 are not; a gap whose frames do not fit max_frames_per_batch is not concealed either: in both
    cases the stream is refused with the words of the switch being off."""
    prog, tmp = host_pocs
    kw = dict(LONG, frames=20)
    r = c2.lose_pictures(sg.encode(want_recon=False, **kw)[0], list(range(2, 2 + c2.MAX_GAP)))
    rc, rows, err = _host(prog, tmp, r.damaged, kw, SLICES | PICTURES)
    assert rc == 0 and [x[1] for x in rows] == list(range(20)), err[-500:]
    rc, rows, err = _host(prog, tmp, r.damaged, kw, SLICES | PICTURES, frames=18)  # 2 pictures in front, 16 inserted ones and the revealing one: 19
    assert rc == 1 and "reference pictures are missing" in err
    kw = dict(LONG, frames=21)
    units, _, pics = cu.parse(sg.encode(want_recon=False, **kw)[0])
    gone = {s.unit for p in range(2, 3 + c2.MAX_GAP) for s in pics[p]}
    damaged = b"".join(u for i, u in enumerate(units) if i not in gone)
    rc, rows, err = _host(prog, tmp, damaged, kw, SLICES | PICTURES)
    assert rc == 1 and "frame_num 19 after 1: reference pictures are missing" in err


def test_abi_has_the_bits_and_the_counter(H):
    """The bit names and the cap are in the header, h264mi_decoder_concealed_pictures is declared, exported, bound in Python and called in Go, and
    h264mi_decoder_create refuses values outside the bit set before it looks for a device."""
    from h264decode_amd import _lib
    header = open(os.path.join(ROOT, "include", "h264mi.h")).read()
    assert re.search(r"#define H264MI_CONCEAL_SLICES 1\b", header) and re.search(r"#define H264MI_CONCEAL_PICTURES 2\b", header)
    assert re.search(r"#define H264MI_CONCEAL_FIELDS 4\b", header) and re.search(r"#define H264MI_CONCEAL_MAX_GAP 16\b", header)
    assert re.search(r"int32_t h264mi_decoder_concealed_pictures\(", header)
    L = H.lib()
    assert hasattr(L, "h264mi_decoder_concealed_pictures") and "h264mi_decoder_concealed_pictures" in _lib.EXPORTS
    assert L.h264mi_decoder_concealed_pictures(None, None) == -1
    assert (H.CONCEAL_SLICES, H.CONCEAL_PICTURES, H.CONCEAL_FIELDS, H.CONCEAL_MAX_GAP) == (1, 2, 4, 16) and hasattr(H.Decoder, "concealed_pictures")
    go = open(os.path.join(ROOT, "go", "h264", "h264mi.go")).read()
    assert "C.h264mi_decoder_concealed_pictures(" in go and "C.H264MI_CONCEAL_PICTURES" in go and "C.H264MI_CONCEAL_SLICES" in go and "C.H264MI_CONCEAL_FIELDS" in go
    assert "h264mi_decoder_concealed_pictures" in open(os.path.join(ROOT, "examples", "h264mi_decode.c")).read()
    assert names_last(_lib) == "conceal_errors"
    for bad in (2, 4, 6, 8, 9, -1):
        cfg = _lib.Config()
        cfg.struct_size = ctypes.sizeof(cfg)
        cfg.max_streams, cfg.max_width, cfg.max_height, cfg.max_frames_per_batch, cfg.conceal_errors = 1, 64, 64, 4, bad
        h = ctypes.c_void_p()
        assert L.h264mi_decoder_create(ctypes.byref(cfg), ctypes.byref(h)) == -1, bad
        assert b"conceal_errors" in L.h264mi_last_error_string()


def names_last(_lib):
    return [f for f, _ in _lib.Config._fields_][-1]


def test_front_ends_leave_room_for_inserted_frames():
    from h264decode_amd import h264
    assert h264._frames_with_headroom(30, False) == 30 and h264._frames_with_headroom(30, True) == 30
    assert h264._frames_with_headroom(30, h264.CONCEAL_SLICES | h264.CONCEAL_PICTURES) == 30 + h264.CONCEAL_MAX_GAP
    serve = open(os.path.join(ROOT, "tools", "serve.py")).read()
    assert "--conceal-pictures" in serve and "--conceal-fields" in serve


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
                     max_bitstream_bytes=sum(len(s) for s in streams) * 2 + (1 << 20), allow_unpinned_field_cabac=_unpinned(kw), **cfg)


def _check_frames(dec, r, want, want_pocs, first=0, n=None, stream=0):
    """Frames [first, first + n) of the repaired stream are the frames of `stream` in the decoder's last batch."""
    n = len(want) - first if n is None else n
    assert dec.stream_status(stream) == 0
    assert dec.frame_count(stream) == n
    out = dec.read_frames(stream, crop=False)
    bad = [i for i in range(n) if not np.array_equal(out[i], want[first + i])]
    assert not bad, "frames %r differ from the oracle's decode of the repaired stream" % ([first + i for i in bad],)
    infos = [dec.frame_info(stream, f) for f in range(n)]
    assert [fi.pic_order_cnt for fi in infos] == [int(x) for x in want_pocs[first:first + n]]
    assert [fi.frame_num for fi in infos] == r.frame_num[first:first + n]
    assert all(fi.nal_ref_idc == 1 and fi.idr == 0 for fi, ins in zip(infos, r.inserted[first:first + n]) if ins)
    assert [dec.frame_concealed(stream, f) for f in range(n)] == [r.mbs if ins else 0 for ins in r.inserted[first:first + n]]


def _check_concealed(H, oracle_mod, kw, r):
    want, _ = oracle_mod.decode(r.repaired, crop=False)
    want_pocs = list(oracle_mod.last_pocs)
    for x in (None, 0, 512):
        with _x_wgs(x):
            dec = _decoder(H, kw, [r.damaged], conceal_errors=SLICES | PICTURES)
            try:
                dec.decode([r.damaged])
                _check_frames(dec, r, want, want_pocs)
                assert dec.concealed_pictures() == sum(r.inserted)
                assert dec.concealed() == (0, r.mbs * sum(r.inserted))
            finally:
                dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_lost_pictures_are_concealed(name, H, sg, oracle_mod):
    kw, lost = CASES[name]
    r = c2.lose_pictures(sg.encode(**kw)[0], lost)
    if name in MATRIX_CASES:  # the conditions of the matrix, on the oracle alone, before the product is asked
        oracle_mod.decode(r.repaired, crop=False)
        c2.check_lost(r, list(oracle_mod.last_pocs))
    _check_concealed(H, oracle_mod, kw, r)


@pytest.mark.gpu
def test_gpu_cap_of_sixteen_frames(H, sg, oracle_mod):
    """16 consecutive lost frames of a 20-frame stream are concealed; 17 of a 21-frame stream end as with the bit clear."""
    kw = dict(LONG, frames=20)
    r = c2.lose_pictures(sg.encode(**kw)[0], list(range(2, 2 + c2.MAX_GAP)))
    assert sum(r.inserted) == c2.MAX_GAP
    _check_concealed(H, oracle_mod, kw, r)
    kw = dict(LONG, frames=21)
    units, _, pics = cu.parse(sg.encode(**kw)[0])
    gone = {s.unit for p in range(2, 3 + c2.MAX_GAP) for s in pics[p]}
    damaged = b"".join(u for i, u in enumerate(units) if i not in gone)
    off, on = _status(H, kw, damaged, SLICES), _status(H, kw, damaged, SLICES | PICTURES)
    assert off[:2] == (-2, -2) and on == off


def _status(H, kw, stream, conceal, frames=None):
    dec = _decoder(H, kw, [stream], frames=frames, conceal_errors=conceal)
    try:
        code = 0
        try:
            dec.decode([stream])
        except H.H264MIError as e:
            code = e.code
        return code, dec.stream_status(0), dec.frame_count(0), dec.concealed(), dec.concealed_pictures()
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_gap_that_does_not_fit_the_batch(H, sg):
    """The inserted frames and the revealing picture need room in max_frames_per_batch; without it the stream ends as with the bit clear."""
    kw, lost = CASES["one_slice_mono_high_1_2"]
    r = c2.lose_pictures(sg.encode(**kw)[0], lost)
    off, on = _status(H, kw, r.damaged, SLICES, frames=3), _status(H, kw, r.damaged, SLICES | PICTURES, frames=3)  # the IDR picture, 2 inserted frames and the revealing picture: 4
    assert off[:2] == (-2, -2) and on == off
    assert _status(H, kw, r.damaged, SLICES | PICTURES, frames=8)[:3] == (0, 0, 8)


@pytest.mark.gpu
def test_gpu_value_1_and_0_refuse_a_gap_as_before(H, sg):
    kw, lost = CASES["one_slice_main_cabac_3"]
    r = c2.lose_pictures(sg.encode(**kw)[0], lost)
    off, on = _status(H, kw, r.damaged, 0), _status(H, kw, r.damaged, True)
    assert off == (-2, -2, 0, (0, 0), 0) and on == off


@pytest.mark.gpu
def test_gpu_revealing_picture_opens_the_next_batch(H, sg, oracle_mod):
    """The lost picture was the last one of a chunk: the gap shows with the first picture of the next prepare.  Batch by batch, and pipelined as
    execute; prepare; execute; sync."""
    kw, lost = CASES["one_slice_main_cabac_3"]
    r = c2.lose_pictures(sg.encode(**kw)[0], lost)
    want, _ = oracle_mod.decode(r.repaired, crop=False)
    want_pocs = list(oracle_mod.last_pocs)
    aus = c2.access_units(r.damaged)
    assert len(aus) == 7
    chunks = [b"".join(aus[:3]), b"".join(aus[3:])]  # pictures 0..2 | 4..7, picture 3 is lost
    for pipelined in (False, True):
        dec = _decoder(H, kw, [r.damaged], frames=5, conceal_errors=SLICES | PICTURES)
        try:
            if pipelined:
                dec.prepare([chunks[0]])
                dec.execute()
                dec.prepare([chunks[1]])
                dec.execute()
                dec.sync()
            else:
                dec.decode([chunks[0]])
                _check_frames(dec, r, want, want_pocs, 0, 3)
                dec.decode([chunks[1]])
            _check_frames(dec, r, want, want_pocs, 3, 5)
            assert dec.concealed_pictures() == 1 and dec.concealed() == (0, r.mbs)
        finally:
            dec.close()


@pytest.mark.gpu
def test_gpu_one_damaged_stream_among_intact_ones(H, sg, oracle_mod):
    names = ["cabac_wp1_multiref", "cavlc_idc2_offsets", "b_ibbp_cabac_implicit", "cabac_idc0_offsets_cqp"]
    kws = [dict(cu.CONCEAL_MATRIX[n], frames=10) for n in names]
    streams = [sg.encode(**kw)[0] for kw in kws]
    r = c2.lose_pictures(streams[1], [4, 5, 8])
    want = [oracle_mod.decode(r.repaired if i == 1 else s, crop=False)[0] for i, s in enumerate(streams)]
    oracle_mod.decode(r.repaired, crop=False)
    want_pocs = list(oracle_mod.last_pocs)
    feed = [r.damaged if i == 1 else s for i, s in enumerate(streams)]
    dec = H.Decoder(max_streams=4, max_width=176, max_height=144, max_frames_per_batch=10, max_slices_per_frame=4, max_bitstream_bytes=1 << 21, conceal_errors=SLICES | PICTURES)
    try:
        dec.decode(feed)
        for i in range(4):
            assert dec.stream_status(i) == 0 and dec.frame_count(i) == 10
            assert np.array_equal(dec.read_frames(i, crop=False), want[i]), "stream %d" % i
        _check_frames(dec, r, want[1], want_pocs, stream=1)
        assert dec.concealed_pictures() == 3 and dec.concealed() == (0, 3 * r.mbs)
    finally:
        dec.close()


def _feed_until_failure(H, kw, stream, conceal):
    """One access unit per call: (frames decoded before the first refusal, its code, the stream status)."""
    dec = _decoder(H, kw, [stream], conceal_errors=conceal)
    frames = []
    try:
        for au in c2.access_units(stream):
            try:
                dec.decode([au])
            except H.H264MIError as e:
                return frames, e.code, dec.stream_status(0)
            frames += [f.copy() for f in dec.read_frames(0, crop=False)] if dec.frame_count(0) else []
        return frames, 0, dec.stream_status(0)
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_what_the_lost_picture_carried_stays_lost(H, sg, oracle_mod):
    """cavlc_wp2_rplm_mmco without picture 6: a later list modification names a picture that the lost marking operations would have kept.  The
    oracle refuses the repaired stream; the product with value 3 on the damaged stream ends where, and with the frames with which, the product
    with value 1 ends on the repaired stream."""
    kw = cu.CONCEAL_MATRIX["cavlc_wp2_rplm_mmco"]
    r = c2.lose_pictures(sg.encode(**kw)[0], [6])
    with pytest.raises(oracle_mod.OracleError, match="ref_pic_list_modification names a missing picture"):
        oracle_mod.decode(r.repaired, crop=False)
    a, b = _feed_until_failure(H, kw, r.damaged, SLICES | PICTURES), _feed_until_failure(H, kw, r.repaired, SLICES)
    assert a[1:] == b[1:] and a[1] != 0
    assert len(a[0]) == len(b[0]) >= 7 and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))


@pytest.mark.gpu
def test_gpu_clean_streams_with_all_bits(H, sg):
    """Every case of the parity matrix, field pictures and streams with declared frame_num gaps included, decodes exactly and reports nothing."""
    for name in sorted(FULL_MATRIX):
        kw = FULL_MATRIX[name]
        stream, rec, _ = sg.encode(**kw)
        dec = _decoder(H, kw, [stream], conceal_errors=SLICES | PICTURES | FIELDS)
        try:
            dec.decode([stream])
            assert np.array_equal(dec.read_frames(0, crop=False), rec), name
            assert dec.concealed() == (0, 0) and dec.concealed_pictures() == 0, name
            assert all(dec.frame_concealed(0, f) == 0 for f in range(dec.frame_count(0))), name
        finally:
            dec.close()


@pytest.mark.gpu
def test_gpu_c_program_with_conceal_all(H, sg, oracle_mod, tmp_path):
    """examples/h264mi_decode.c --conceal-all on a stream of one slice per picture with a lost picture: the oracle's frames of the repaired
    stream, and the picture total."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    kw, lost = CASES["one_slice_main_cabac_3"]
    r = c2.lose_pictures(sg.encode(**kw)[0], lost)
    want, info = oracle_mod.decode(r.repaired, crop=True)
    src, dst = tmp_path / "in.h264", tmp_path / "out.yuv"
    src.write_bytes(r.damaged)
    p = subprocess.run([os.path.join(ROOT, "examples", "h264mi_decode"), str(src), str(dst), "3", "--conceal-all"], stderr=subprocess.PIPE, check=True)
    got = np.frombuffer(dst.read_bytes(), dtype=np.uint8).reshape(-1, info.width * info.height * 3 // 2)
    assert np.array_equal(got, want)
    assert "concealed: 1 pictures" in p.stderr.decode() and ("concealed: 0 slices, %d macroblocks" % r.mbs) in p.stderr.decode()
