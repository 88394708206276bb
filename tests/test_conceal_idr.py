"""Error concealment of IDR pictures (h264mi_config.conceal_errors with H264MI_CONCEAL_IDR = 16): lost and damaged slices of an IDR frame picture that
still has a reference frame are reconstructed as a zero-motion copy of entry 0 of the initial P list built before the picture's marking.  The
yardstick is the oracle's decode of the REPAIRED stream (tests/concealutil3.py: the IDR picture relabelled as a non-IDR picture that ends in memory
management operation 5); every GPU comparison is bit-exact."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import concealutil as cu
import concealutil2 as c2
import concealutil3 as c3
import dpbtrace
from concealutil3 import COPY_CASES, HEADER_CASES, IDR_MATRIX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICES, PICTURES, FIELDS, IDR = 1, 2, 4, 16  # H264MI_CONCEAL_*
ON = SLICES | IDR

_cache = {}


def _case(name, sg, oracle_mod):
    """Generated once per case and left unchanged: the stream, the oracle's frames and PicOrderCnt list of it."""
    if name not in _cache:
        kw, spec = IDR_MATRIX[name]
        stream = sg.encode(want_recon=False, **kw)[0]
        ref, info = oracle_mod.decode(stream, crop=False)
        _cache[name] = (kw, spec, stream, ref, info, [int(x) for x in oracle_mod.last_pocs])
    return _cache[name]


def _repaired(name, mode, sg, oracle_mod):
    """(Made, the oracle's frames of the repaired stream, its PicOrderCnt list), once per case and mode."""
    key = (name, mode)
    if key not in _cache:
        kw, spec, stream = _case(name, sg, oracle_mod)[:3]
        m = c3.make(stream, spec, mode)
        want, _ = oracle_mod.decode(m.repaired, crop=False)
        _cache[key] = (m, want, [int(x) for x in oracle_mod.last_pocs])
    return _cache[key]


# ---------------------------------------------------------------- CPU: the writer and the rule, independent of the product's device code
@pytest.mark.parametrize("name", sorted(IDR_MATRIX))
def test_repaired_stream_is_a_valid_stream(name, sg, oracle_mod):
    """The case meets its conditions (concealutil3.check_case); the stream in which X is only relabelled decodes exactly like the original; the
    repaired stream decodes without error to the original's frame count and PicOrderCnt list, the frames in front of the first damaged picture
    untouched and that picture changed -- for lost and for damaged slices."""
    kw, spec, stream, ref, info, pocs = _case(name, sg, oracle_mod)
    assert kw["width"] >= 176 and kw["height"] >= 144 and 9 <= kw["frames"] <= 12 and 3 <= kw["idr_period"] <= 6 and 3 <= cu.nslices(kw) <= 4
    for mode in ("lost", "damaged"):
        m = c3.make(stream, spec, mode)  # (asserts check_case)
        assert all(m.pics[p][0].hdr.pic_order_cnt_lsb == 0 and m.pics[p][0].hdr.frame_num == 0 and not m.pics[p][0].hdr.long_term_reference_flag and
                   m.pics[p][0].hdr.slice_type == 7 for p in m.xs)
        assert m.damaged != stream and m.repaired != stream and m.relabelled != stream
        out, info2 = oracle_mod.decode(m.relabelled, crop=False)
        assert info2.n_frames == info.n_frames == kw["frames"] and np.array_equal(out, ref) and [int(x) for x in oracle_mod.last_pocs] == pocs
        out, info2 = oracle_mod.decode(m.repaired, crop=False)
        assert info2.n_frames == info.n_frames and [int(x) for x in oracle_mod.last_pocs] == pocs
        first = min(p for p, c in enumerate(m.per_picture) if c)
        assert np.array_equal(out[:first], ref[:first])
        assert not np.array_equal(out[first], ref[first])
        for x in m.xs:  # from the next IDR picture on that is not damaged itself the frames are the original's again
            nxt = next((p for p in range(x + 1, len(m.pics)) if m.pics[p][0].type == 5), None)
            if nxt is not None and not any(m.per_picture[nxt:]):
                assert np.array_equal(out[nxt:], ref[nxt:])


def test_the_matrix_has_the_required_shapes(sg):
    """A first, a middle and a last slice of an IDR picture, two adjacent slices of one, two damaged IDR pictures in one stream, picks in P pictures of
    a damaged GOP in two cases (concealutil3.check_matrix); both entropy coders, the three POC types, B pictures, slice groups, both start codes."""
    resolved = []
    for name, (kw, spec) in IDR_MATRIX.items():
        _, _, pics = cu.parse(sg.encode(want_recon=False, **kw)[0])
        resolved.append((pics, c3.resolve(pics, spec)))
    c3.check_matrix(resolved)
    kws = [kw for kw, _ in IDR_MATRIX.values()]
    assert 8 <= len(kws) <= 10
    assert {kw["cabac"] for kw in kws} == {0, 1} and {kw.get("poc_type", 0) for kw in kws} == {0, 1, 2} and {kw.get("deblock_idc", 0) for kw in kws} == {0, 1, 2}
    assert any(kw.get("bframes") for kw in kws) and any(kw.get("slice_groups") and kw.get("aso") for kw in kws) and any(kw.get("transform8x8") for kw in kws)
    assert any(kw.get("mmco") and kw.get("rplm") and kw.get("weighted_pred") for kw in kws) and any(kw.get("long_start_code") == 0 for kw in kws)
    assert any(kw.get("mono") for kw in kws) and any(kw["width"] % 16 for kw in kws)


@pytest.mark.parametrize("name", COPY_CASES)
def test_replaced_macroblocks_are_a_copy_of_the_concealment_reference(name, sg, oracle_mod):
    """deblock_idc 1 in the intact slices, only IDR picks in the damaged GOPs, one reference frame and no non-reference pictures: a replaced macroblock
    of X whose left and upper neighbours are replaced too (or outside the picture) equals the co-located samples of the frame decoded last before X."""
    kw, spec, stream = _case(name, sg, oracle_mod)[:3]
    assert kw["deblock_idc"] == 1 and sg.default_params(**kw).num_ref_frames == 1 and not kw.get("bframes") and not kw.get("nonref_period")
    m, out, _ = _repaired(name, "lost", sg, oracle_mod)
    assert set(m.lost) == set(m.xs)
    wmb, hmb = m.pics[0][0].wmb, m.pics[0][0].hmb
    W, Hh = wmb * 16, hmb * 16

    def planes(f):
        return f[:W * Hh].reshape(Hh, W), f[W * Hh:W * Hh * 5 // 4].reshape(Hh // 2, W // 2), f[W * Hh * 5 // 4:].reshape(Hh // 2, W // 2)
    n_full = 0
    for p, mbs in m.lost.items():
        cur, prev = planes(out[p]), planes(out[p - 1])
        s = set(mbs)
        for a in mbs:
            x, y = a % wmb, a // wmb
            if (x == 0 or a - 1 in s) and (y == 0 or a - wmb in s):
                n_full += 1
                assert np.array_equal(cur[0][16 * y:16 * y + 16, 16 * x:16 * x + 16], prev[0][16 * y:16 * y + 16, 16 * x:16 * x + 16]), (p, a)
                for c in (1, 2):
                    assert np.array_equal(cur[c][8 * y:8 * y + 8, 8 * x:8 * x + 8], prev[c][8 * y:8 * y + 8, 8 * x:8 * x + 8]), (p, a, c)
    assert n_full > 20


def test_abi_has_the_bit(H):
    """The define is in the header, bound in Python, Go and the example; h264mi_decoder_create gets past the conceal_errors check with the four new
    values and refuses the other values with bit 16 -- and bit 8, which stays unassigned -- before it looks for a device."""
    from h264decode_amd import _lib
    assert re.search(r"#define H264MI_CONCEAL_IDR 16\b", open(os.path.join(ROOT, "include", "h264mi.h")).read())
    assert H.CONCEAL_IDR == 16
    assert "C.H264MI_CONCEAL_IDR" in open(os.path.join(ROOT, "go", "h264", "h264mi.go")).read()
    assert "--conceal-idr" in open(os.path.join(ROOT, "examples", "h264mi_decode.c")).read()
    assert [f for f, _ in _lib.Config._fields_][-1] == "conceal_errors"
    L = H.lib()

    def create(value):
        cfg = _lib.Config()
        cfg.struct_size = ctypes.sizeof(cfg)
        cfg.max_streams, cfg.max_width, cfg.max_height, cfg.max_frames_per_batch, cfg.conceal_errors = 1, 64, 64, 4, value
        h = ctypes.c_void_p()
        r = L.h264mi_decoder_create(ctypes.byref(cfg), ctypes.byref(h))
        err = L.h264mi_last_error_string() if r != 0 else b""
        if r == 0:
            L.h264mi_decoder_destroy(h)
        return r, err
    for good in (17, 19, 21, 23):
        r, err = create(good)
        assert b"conceal_errors" not in err, (good, err)  # (without a device: refused further down, for the device)
    for bad in (16, 18, 24, 32, 33, 25):
        r, err = create(bad)
        assert r == -1 and b"conceal_errors" in err, (bad, r, err)


@pytest.fixture(scope="module")
def tracer(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("host_dpb_trace_idr")
    return dpbtrace.build(tmp), tmp


def _pic_lines(text):
    """[{field: int}] of the `pic` lines of a trace."""
    return [{k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)} for line in text.splitlines() if line.startswith("pic ")]


def _parameter_sets(stream):
    out = []
    for u in cu.split_units(stream):
        if (u[cu._sc_len(u)] & 31) not in (7, 8):
            break
        out.append(u)
    return b"".join(out)


@pytest.mark.parametrize("name", ["cabac_main", "cavlc_idc1"])
def test_host_finds_the_concealment_reference(name, tracer, sg):
    """The host side against the null device.  With 17 the IDR picture X names the slot of the reference frame decoded last before it and is
    reconstructed one wave behind it; with 1, and with 17 when X is the stream's first picture, it names none.  A lost slice of X passes prepare
    under both values (the loss shows on the device); a slice of X whose header does not parse passes under 17, counted as dropped, and is refused
    under 1 as ever."""
    prog, tmp = tracer
    kw, spec = IDR_MATRIX[name]
    stream = sg.encode(want_recon=False, **kw)[0]
    m = c3.make(stream, spec, "lost")
    x = m.xs[0]
    on, off = _pic_lines(dpbtrace.trace(prog, tmp, kw, ON, [m.damaged])), _pic_lines(dpbtrace.trace(prog, tmp, kw, SLICES, [m.damaged]))
    assert len(on) == len(off) == kw["frames"]
    assert on[x]["conceal_ref"] == on[x - 1]["slot"] and on[x]["wave"] == on[x - 1]["wave"] + 1
    assert on[x]["n_slices"] == len(m.pics[x]) - sum(1 for p, _ in m.picks if p == x)
    assert off[x]["conceal_ref"] == -1 and off[x]["wave"] == 0
    assert on[0]["conceal_ref"] == -1 and all(a == b for a, b in zip(on[:x], off[:x]))
    # X's reference comes from an earlier batch: still named, and X is in wave 0
    aus = c2.access_units(m.damaged)
    two = _pic_lines(dpbtrace.trace(prog, tmp, kw, ON, [b"".join(aus[:x]), b"".join(aus[x:])]))
    assert two[x]["conceal_ref"] == two[x - 1]["slot"] and two[x]["wave"] == 0
    # X as the first picture of a stream
    alone = _pic_lines(dpbtrace.trace(prog, tmp, kw, ON, [_parameter_sets(stream) + b"".join(aus[x:])]))
    assert alone[0]["conceal_ref"] == -1 and alone[0]["wave"] == 0
    # a slice header that does not parse
    h = c3.make(stream, spec, "header")
    text = dpbtrace.trace(prog, tmp, kw, ON, [h.damaged])
    assert "refused" not in text and _pic_lines(text)[x]["dropped"] == sum(1 for p, _ in h.picks if p == x)
    text = dpbtrace.trace(prog, tmp, kw, SLICES, [h.damaged])
    assert "refused prepare=-2 status=-2" in text and not _pic_lines(text)


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
    return H.Decoder(max_streams=len(streams), max_width=W, max_height=Hc, max_frames_per_batch=frames or kw["frames"], max_slices_per_frame=max(cu.nslices(kw), 1),
                     max_bitstream_bytes=sum(len(s) for s in streams) * 2 + (1 << 20), **cfg)


def _check_concealed(H, oracle_mod, sg, name, mode):
    kw = IDR_MATRIX[name][0]
    m, want, want_pocs = _repaired(name, mode, sg, oracle_mod)
    n = kw["frames"]
    dropped = m.n_slices if mode == "header" else 0
    for x in (None, 0, 512):
        with _x_wgs(x):
            dec = _decoder(H, kw, [m.damaged], conceal_errors=ON)
            try:
                dec.decode([m.damaged])
                if mode == "damaged":  # precondition: the entropy kernels reported every damaged slice (otherwise the DAMAGE is at fault, not the feature)
                    assert dec.concealed()[0] == m.n_slices, "damage not detected: %r" % (dec.concealed(),)
                assert dec.stream_status(0) == 0
                assert dec.frame_count(0) == n
                out = dec.read_frames(0, crop=False)
                bad = [i for i in range(n) if not np.array_equal(out[i], want[i])]
                assert not bad, "frames %r differ from the oracle's decode of the repaired stream (H264MI_X_WGS=%r)" % (bad, x)
                infos = [dec.frame_info(0, f) for f in range(n)]
                assert [fi.pic_order_cnt for fi in infos] == want_pocs
                assert all(infos[p].idr == 1 and infos[p].frame_num == 0 for p in m.xs)
                assert [dec.frame_concealed(0, f) for f in range(n)] == m.per_picture
                assert dec.concealed() == (m.n_slices if mode == "damaged" else dropped, sum(m.per_picture))
            finally:
                dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(IDR_MATRIX))
def test_gpu_lost_slices_of_idr_pictures_are_concealed(name, H, sg, oracle_mod):
    _check_concealed(H, oracle_mod, sg, name, "lost")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(IDR_MATRIX))
def test_gpu_damaged_slices_of_idr_pictures_are_concealed(name, H, sg, oracle_mod):
    _check_concealed(H, oracle_mod, sg, name, "damaged")


@pytest.mark.gpu
@pytest.mark.parametrize("name", HEADER_CASES)
def test_gpu_slices_with_unparsable_headers_are_lost_slices(name, H, sg, oracle_mod):
    """A type-5 slice NAL unit whose header does not parse is dropped and counted: in the IDR picture under construction, or -- the first slice of X
    in stream order -- in the picture the next slice starts."""
    _check_concealed(H, oracle_mod, sg, name, "header")


def _frames_by_feed(H, kws, feed_chunks, frames_per_batch, pipelined):
    """Decodes chunk list after chunk list ([per stream bytes or b""]) on one decoder: per stream the frames of all batches, and the totals."""
    dec = H.Decoder(max_streams=len(kws), max_width=176, max_height=144, max_frames_per_batch=frames_per_batch, max_slices_per_frame=4, max_bitstream_bytes=1 << 21,
                    conceal_errors=ON)
    got = [[] for _ in kws]
    try:
        def harvest():
            for i in range(len(kws)):
                assert dec.stream_status(i) == 0
                if dec.frame_count(i):
                    got[i] += [f.copy() for f in dec.read_frames(i, crop=False)]
        if pipelined:  # execute(k); prepare(k + 1); one sync
            dec.prepare(feed_chunks[0])
            for k in range(len(feed_chunks)):
                dec.execute()
                if k + 1 < len(feed_chunks):
                    dec.prepare(feed_chunks[k + 1])
                dec.sync()
                harvest()
        else:
            for chunks in feed_chunks:
                dec.decode(chunks)
                harvest()
        return got, dec.concealed()
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_one_batch_gop_batches_and_single_access_units_agree(H, sg, oracle_mod):
    """Three streams in one decoder, two of them damaged (one of those in two IDR pictures): as one batch, as one GOP per batch -- X's reference comes
    from an earlier batch --, and as single access units, pipelined.  Each way every stream equals the oracle's decode of its repaired stream."""
    names = ["cabac_main", "cavlc_poc1", "high8x8_mmco_rplm_wp"]
    kws = [IDR_MATRIX[n][0] for n in names]
    feed, want, mbs, n_slices = [], [], 0, 0
    for i, n in enumerate(names):
        if i < 2:
            m, w, _ = _repaired(n, "damaged", sg, oracle_mod)
            feed.append(m.damaged), want.append(w)
            mbs, n_slices = mbs + sum(m.per_picture), n_slices + m.n_slices
        else:
            feed.append(_case(n, sg, oracle_mod)[2]), want.append(_case(n, sg, oracle_mod)[3])
    aus = [c2.access_units(s) for s in feed]
    assert [len(a) for a in aus] == [kw["frames"] for kw in kws]
    gops = [[b"".join(a[k:k + 4]) for k in range(0, len(a), 4)] for a in aus]  # idr_period 4 in all three
    assert all(len(g) == 3 for g in gops)
    longest = max(len(a) for a in aus)
    ways = {"one batch": ([feed], 10, False), "a GOP per batch": ([[g[k] for g in gops] for k in range(3)], 4, False),
            "single access units": ([[a[k] if k < len(a) else b"" for a in aus] for k in range(longest)], 1, True)}
    for way, (chunks, per_batch, pipelined) in ways.items():
        got, totals = _frames_by_feed(H, kws, chunks, per_batch, pipelined)
        for i in range(3):
            assert len(got[i]) == kws[i]["frames"], (way, i)
            bad = [f for f in range(len(got[i])) if not np.array_equal(got[i][f], want[i][f])]
            assert not bad, "%s: frames %r of stream %d differ from the oracle's decode of the repaired stream" % (way, bad, i)
        assert totals == (n_slices, mbs), way


def _status(H, kw, stream, conceal, frames=None, **cfg):
    dec = _decoder(H, kw, [stream], frames=frames, conceal_errors=conceal, **cfg)
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
@pytest.mark.parametrize("name", ["cavlc_poc2_idc2", "cabac_main"])
def test_gpu_nothing_changes_with_the_bit_clear(name, H, sg):
    """The IDR-damaged stream with 0 and with 1: the same error code, stream status and counters as ever -- a damaged slice fails the stream in the
    entropy kernel (-8), a header that does not parse when the batch is prepared (-2)."""
    kw, spec = IDR_MATRIX[name]
    stream = sg.encode(want_recon=False, **kw)[0]
    only_x = [e for e in spec if e[0] == "idr"]
    for mode, code in (("damaged", -8), ("header", -2)):
        damaged = c3.make(stream, only_x, mode).damaged
        off, on = _status(H, kw, damaged, 0), _status(H, kw, damaged, SLICES)
        assert off == (code, code, (0, 0)) and on == off, (mode, off, on)


@pytest.mark.gpu
def test_gpu_not_concealable_stays_as_it_is(H, sg):
    """With 17 and 21 as with 1: damage in the stream's first picture, in the first IDR picture after a change of picture size, and in an IDR field
    picture fails the stream with the same error and status."""
    kw = IDR_MATRIX["cavlc_poc2_idc2"][0]
    stream = sg.encode(want_recon=False, **kw)[0]
    for mode, code in (("damaged", -8), ("header", -2)):
        damaged = cu.make(stream, [(0, 1)], mode=mode, repair=False)[0]
        ref = _status(H, kw, damaged, SLICES)
        assert ref[:2] == (code, code)
        for v in (ON, ON | FIELDS):
            assert _status(H, kw, damaged, v) == ref, (mode, v)
    # two recipes of different size back to back: the second one's IDR picture has reference frames in the DPB, decoded under another SPS
    kw2 = dict(kw, width=144, height=112, seed=712)
    both = stream + sg.encode(want_recon=False, **kw2)[0]
    _, _, pics = cu.parse(both)
    assert pics[kw["frames"]][0].type == 5 and pics[kw["frames"]][0].wmb == 9 and pics[0][0].wmb == 11
    damaged = cu.make(both, [(kw["frames"], 1)], mode="damaged", repair=False)[0]
    ref = _status(H, kw, damaged, SLICES, frames=2 * kw["frames"])
    assert ref[:2] == (-8, -8)
    for v in (ON, ON | FIELDS):
        assert _status(H, kw, damaged, v, frames=2 * kw["frames"]) == ref, v
    # an IDR field picture (the first field of the second IDR frame)
    kwf = dict(width=176, height=128, frames=5, idr_period=3, profile_idc=77, cabac=0, field_pics=1, slices=3, num_ref_frames=2, seed=713)
    stream = sg.encode(want_recon=False, **kwf)[0]
    _, _, pics = cu.parse(stream)
    x = [p for p, sl in enumerate(pics) if sl[0].type == 5][1]
    assert pics[x][0].hdr.field_pic
    for mode, code in (("damaged", -8), ("header", -2)):
        damaged = cu.make(stream, [(x, 1)], mode=mode, repair=False)[0]
        ref = _status(H, kwf, damaged, SLICES, frames=10)
        assert ref[:2] == (code, code)
        for v in (ON, ON | FIELDS):
            assert _status(H, kwf, damaged, v, frames=10) == ref, (mode, v)


@pytest.mark.gpu
def test_gpu_clean_streams_with_the_bit_set(H, sg, oracle_mod):
    """Intact streams with several GOPs in one batch -- every IDR picture but the first reconstructed behind its reference -- decode exactly and
    report nothing concealed; several streams side by side too."""
    for name in sorted(IDR_MATRIX):
        kw, _, stream, ref = _case(name, sg, oracle_mod)[:4]
        dec = _decoder(H, kw, [stream], conceal_errors=ON)
        try:
            dec.decode([stream])
            assert np.array_equal(dec.read_frames(0, crop=False), ref), name
            assert dec.concealed() == (0, 0), name
            assert all(dec.frame_concealed(0, f) == 0 for f in range(dec.frame_count(0))), name
        finally:
            dec.close()
    names = ["cabac_main", "cavlc_poc1", "cabac_b_multiref", "mono_cavlc_b_spatial"]
    streams = [_case(n, sg, oracle_mod)[2] for n in names]
    dec = H.Decoder(max_streams=4, max_width=176, max_height=144, max_frames_per_batch=12, max_slices_per_frame=4, max_bitstream_bytes=1 << 21, conceal_errors=ON | PICTURES | FIELDS)
    try:
        dec.decode(streams)
        for i, n in enumerate(names):
            assert np.array_equal(dec.read_frames(i, crop=False), _case(n, sg, oracle_mod)[3]), n
        assert dec.concealed() == (0, 0)
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_c_program_with_conceal_idr(H, sg, oracle_mod, tmp_path):
    """examples/h264mi_decode.c --conceal-idr: the damaged stream decodes to the oracle's pictures of the repaired one, and the program reports the totals."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    name = "high8x8_mmco_rplm_wp"
    m, _, _ = _repaired(name, "damaged", sg, oracle_mod)
    want, info = oracle_mod.decode(m.repaired, crop=True)
    src, dst = tmp_path / "in.h264", tmp_path / "out.yuv"
    src.write_bytes(m.damaged)
    p = subprocess.run([os.path.join(ROOT, "examples", "h264mi_decode"), str(src), str(dst), "4", "--conceal-idr"], stderr=subprocess.PIPE, check=True)
    got = np.frombuffer(dst.read_bytes(), dtype=np.uint8).reshape(-1, info.width * info.height * 3 // 2)
    assert np.array_equal(got, want)
    assert ("concealed: %d slices, %d macroblocks" % (m.n_slices, sum(m.per_picture))) in p.stderr.decode()
