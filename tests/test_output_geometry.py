"""Output geometry: crop origin, crop units and the smallest pictures.

Every expected value here is the standard's formula (7.4.2.1.1, 7-18 .. 7-21) written out in tests/spsutil.py with numpy slicing over the
generator's coded-size reconstruction -- pixels do not depend on cropping --, never the crop code of the product, the oracle or the generator.
The streams get their crop rectangle from spsutil.recrop(), which rewrites the SPS: left and top offsets, all four at once, the four-row unit
of frame_mbs_only_flag = 0 and the one-sample unit of monochrome streams (odd display sizes) are things the generator never writes itself.
All comparisons are exact."""
import io
import os

import numpy as np
import pytest

import spsutil
from conftest import MATRIX

IPP = dict(frames=3, idr_period=0)
# name: (generator recipe at coded size, (left, right, top, bottom) for the SPS)
TABLE = {
    # x0 = 32, y0 = 16, w = 160: every luma and chroma row of K6 takes the 16-byte path from a non-zero origin
    "a_aligned_origin": (dict(IPP, width=192, height=144, profile_idc=77, cabac=1, seed=901), (16, 0, 8, 0)),
    "b_left_1": (dict(IPP, width=176, height=144, profile_idc=66, cabac=0, seed=902), (1, 0, 0, 0)),  # byte path, chroma origin 1
    "c_all_four": (dict(IPP, width=176, height=144, profile_idc=77, cabac=1, seed=903), (3, 5, 7, 2)),
    # luma rows stay aligned; W / 2 = 88: chroma rows alternate between the two paths
    "d_top_1": (dict(IPP, width=176, height=144, profile_idc=100, cabac=1, transform8x8=1, seed=904), (0, 0, 1, 0)),
    "e_interlace_sps": (dict(IPP, width=176, height=128, profile_idc=77, cabac=0, interlace_sps=1, num_ref_frames=2, seed=905), (2, 1, 3, 1)),  # unit of 4 rows
    "f_field_pics": (dict(IPP, width=176, height=128, profile_idc=77, cabac=0, field_pics=1, num_ref_frames=2, seed=906), (0, 2, 2, 1)),
    "g_16x16": (dict(IPP, width=16, height=16, profile_idc=77, cabac=1, seed=907), (7, 0, 7, 0)),  # 2x2 display, chroma 1x1
    "h_mono": (dict(IPP, width=176, height=144, profile_idc=100, mono=1, cabac=1, transform8x8=1, seed=908), (1, 2, 3, 4)),  # 173x137, chroma 87x69
    "i_mono_interlace_sps": (dict(IPP, width=176, height=128, profile_idc=100, mono=1, cabac=0, interlace_sps=1, seed=909), (0, 3, 1, 0)),  # unit of 2 rows
}
ROWS = sorted(TABLE)
# what the formulas give, worked out by hand: (x0, y0, w, h)
RECTS = {"a_aligned_origin": (32, 16, 160, 128), "b_left_1": (2, 0, 174, 144), "c_all_four": (6, 14, 160, 126), "d_top_1": (0, 2, 176, 142),
         "e_interlace_sps": (4, 12, 170, 112), "f_field_pics": (0, 8, 172, 116), "g_16x16": (14, 14, 2, 2), "h_mono": (1, 3, 173, 137),
         "i_mono_interlace_sps": (0, 2, 173, 126)}

# the smallest pictures: every macroblock on all four picture edges at once, degenerate inter window clamps, band plans of one row, fields of one
# macroblock row.  (The generator accepts all six at the sizes asked for.)
SMALL = {
    "16x16_main_cabac": dict(IPP, width=16, height=16, profile_idc=77, cabac=1, seed=921),
    "16x16_baseline_intra_pcm": dict(IPP, width=16, height=16, profile_idc=66, cabac=0, intra_in_p_permille=300, pcm_permille=50, seed=922),
    "16x32_field_pics": dict(IPP, width=16, height=32, profile_idc=77, cabac=0, field_pics=1, num_ref_frames=2, seed=923),
    "32x16_high_8x8_b": dict(width=32, height=16, frames=4, idr_period=0, profile_idc=100, cabac=1, transform8x8=1, bframes=1, num_ref_frames=2, seed=924),
    "16x64_slices4": dict(IPP, width=16, height=64, profile_idc=77, cabac=1, slices=4, seed=925),
    "48x16_qpel_sub8x8": dict(IPP, width=48, height=16, profile_idc=66, cabac=0, motion_x4=37, motion_y4=-23, sub8x8_permille=500, seed=926),
}


class Case:
    def __init__(self, sg, name):
        self.kw, self.crop = TABLE[name]
        self.raw, self.rec, _ = sg.encode(**self.kw)
        self.stream, self.info = spsutil.recrop(self.raw, *self.crop)
        self.rect = spsutil.crop_rect(self.info, *self.crop)
        self.want = spsutil.expected_frames(self.rec, self.info, *self.crop)
        self.pictures = self.kw["frames"] * (2 if self.kw.get("field_pics") else 1)


@pytest.fixture(scope="module")
def cases(sg):
    """Every table row once: generated, rewritten, with its expected output (shared by the tests below and never written to)."""
    out = {name: Case(sg, name) for name in ROWS}
    for c in out.values():
        c.rec.setflags(write=False), c.want.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def small(sg):
    out = {}
    for name, kw in SMALL.items():
        stream, rec, _ = sg.encode(**kw)
        rec.setflags(write=False)
        out[name] = (kw, stream, rec)
    return out


# ------------------------------------------------------------------------------------------------ CPU


def test_table_rectangles_by_hand(cases):
    """spsutil.crop_rect against the rectangles worked out by hand, and the sizes the issue names."""
    for name in ROWS:
        c = cases[name]
        assert c.rect == RECTS[name], name
        assert (c.info["coded_w"], c.info["coded_h"]) == (c.kw["width"], c.kw["height"])
        assert c.want.shape == (3, spsutil.i420_size(*c.rect[2:]))
    assert cases["h_mono"].want.shape[1] == 173 * 137 + 2 * 87 * 69
    assert cases["g_16x16"].want.shape[1] == 6


@pytest.mark.parametrize("name", ["crop_3byte_sc", "interlace_sps_cabac", "mono_cropped_cavlc_qpel", "scaling_matrix_cropped"])
def test_recrop_with_the_generators_own_offsets_is_the_identity(name, sg):
    """... byte for byte: start codes of both lengths, chroma_format_idc, the scaling lists' nextScale loop, both frame_mbs_only values and
    the trailing bits survive the round trip, and the generator writes the standard's units (monochrome: one luma sample)."""
    kw = MATRIX[name] if name in MATRIX else dict(width=180, height=100, frames=2, idr_period=0, profile_idc=100, cabac=1, transform8x8=1, scaling_matrix=1, seed=931)
    stream, _, _ = sg.encode(**kw)
    W, H = (kw["width"] + 15) // 16 * 16, (kw["height"] + 15) // 16 * 16
    ux = 1 if kw.get("mono") else 2
    uy = ux * (2 if kw.get("interlace_sps") else 1)
    assert (W - kw["width"]) % ux == 0 and (H - kw["height"]) % uy == 0 and (W > kw["width"] or H > kw["height"])
    again, info = spsutil.recrop(stream, 0, (W - kw["width"]) // ux, 0, (H - kw["height"]) // uy)
    assert again == stream
    assert info == dict(chroma_format_idc=0 if kw.get("mono") else 1, coded_w=W, coded_h=H, frame_mbs_only=0 if kw.get("interlace_sps") else 1)
    # and a different rectangle really changes the SPS (and nothing else)
    other, _ = spsutil.recrop(stream, 1, 0, 0, 0)
    assert other != stream and [n for _, n in spsutil.split_nals(other)][1:] == [n for _, n in spsutil.split_nals(stream)][1:]


@pytest.mark.parametrize("name", ROWS)
def test_host_parser_reports_offsets_and_display_size(name, cases, H):
    c = cases[name]
    (rbsp,) = spsutil.sps_rbsps(c.stream)
    sps = H.NewSPS(rbsp)
    assert sps.FrameCropping == 1
    assert (sps.FrameCropLeftOffset, sps.FrameCropRightOffset, sps.FrameCropTopOffset, sps.FrameCropBottomOffset) == c.crop
    assert (sps.width, sps.height) == c.rect[2:]
    assert (sps.ChromaFormat, sps.FrameMbsOnly) == (c.info["chroma_format_idc"], c.info["frame_mbs_only"])


def test_crop_range_check_edges(cases, H):
    """What remains must be a non-empty part of the picture, in the units of the stream's own chroma format and frame_mbs_only_flag: the last
    accepted sum of offsets leaves one unit, the next one is H264MI_EBITSTREAM (-2)."""
    def parse(row, crop):
        (rbsp,) = spsutil.sps_rbsps(spsutil.recrop(cases[row].raw, *crop)[0])
        return H.NewSPS(rbsp)
    # (row, horizontal?, largest accepted sum, what then remains)
    edges = [("c_all_four", True, 87, 2), ("h_mono", True, 175, 1),          # 176 wide: units of 2 and of 1
             ("c_all_four", False, 71, 2), ("h_mono", False, 143, 1),        # 144 high, frame_mbs_only_flag = 1: units of 2 and of 1
             ("e_interlace_sps", False, 31, 4), ("i_mono_interlace_sps", False, 63, 2)]  # 128 high, frame_mbs_only_flag = 0: units of 4 and of 2
    for row, horizontal, total, left_over in edges:
        for a in (0, 1, total):  # the sum counts, however it is split
            b = total - a
            sps = parse(row, (a, b, 0, 0) if horizontal else (0, 0, a, b))
            assert (sps.width if horizontal else sps.height) == left_over, (row, horizontal, a)
            with pytest.raises(H.H264MIError) as ei:
                parse(row, (a, b + 1, 0, 0) if horizontal else (0, 0, a, b + 1))
            assert ei.value.code == -2, (row, horizontal, a)


@pytest.mark.parametrize("name", ROWS)
def test_oracle_crops_by_the_formulas(name, cases, oracle_mod):
    c = cases[name]
    out, info = oracle_mod.decode(c.stream, crop=True)
    assert (info.width, info.height, info.coded_width, info.coded_height) == c.rect[2:] + (c.info["coded_w"], c.info["coded_h"])
    assert out.shape == c.want.shape and np.array_equal(out, c.want)
    full, _ = oracle_mod.decode(c.stream, crop=False)
    assert np.array_equal(full, c.rec)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_oracle_decodes_the_smallest_pictures(name, small, oracle_mod):
    kw, stream, rec = small[name]
    out, info = oracle_mod.decode(stream, crop=False)
    assert (info.coded_width, info.coded_height, info.n_frames) == (kw["width"], kw["height"], kw["frames"])
    assert np.array_equal(out, rec)


# ------------------------------------------------------------------------------------------------ GPU


def _decoder(H, w, h, pictures, streams=1, slices=1):
    return H.Decoder(max_streams=streams, max_width=w, max_height=h, max_frames_per_batch=pictures, max_slices_per_frame=slices)


def _packed(dec, want_bytes, stream):
    """pack_batch into a device buffer of exactly the expected size with 64 guard bytes behind it, all 0xA5 before."""
    import torch
    buf = torch.full((want_bytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    n = dec.pack_batch(buf.data_ptr(), want_bytes, stream=stream)
    dec.sync()
    got = buf.cpu().numpy()
    assert n == want_bytes
    assert (got[want_bytes:] == 0xA5).all(), "K6 wrote behind the last frame"
    return got[:want_bytes]


def _check_info(dec, stream, frame, c):
    fi = dec.frame_info(stream, frame)
    assert (fi.width, fi.height, fi.coded_width, fi.coded_height, fi.crop_x, fi.crop_y) == \
        (c.rect[2], c.rect[3], c.info["coded_w"], c.info["coded_h"], c.rect[0], c.rect[1]), (stream, frame)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROWS)
def test_gpu_crop_table(name, cases, H):
    import torch
    from h264decode_amd._lib import check
    c = cases[name]
    n = c.kw["frames"]
    dec = _decoder(H, c.info["coded_w"], c.info["coded_h"], c.pictures)
    try:
        dec.decode([c.stream])
        assert dec.frame_count(0) == n
        for f in range(n):
            _check_info(dec, 0, f, c)
            got = dec.read_frame_tight(0, f, crop=True)
            assert got.shape == c.want[f].shape and np.array_equal(got, c.want[f]), ("read, cropped", f)
            assert np.array_equal(dec.read_frame_tight(0, f, crop=False), c.rec[f]), ("read, coded size", f)
        assert np.array_equal(_packed(dec, c.want.size, 0), c.want.reshape(-1)), "pack_batch"
        one = c.want.shape[1]
        buf = torch.full((one + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        check(dec._L.h264mi_frame_pack_device(dec._h, 0, n - 1, buf.data_ptr(), one))
        dec.sync()
        got = buf.cpu().numpy()
        assert np.array_equal(got[:one], c.want[n - 1]) and (got[one:] == 0xA5).all(), "h264mi_frame_pack_device"
        assert dec._L.h264mi_frame_pack_device(dec._h, 0, n - 1, buf.data_ptr(), one - 1) == -7  # H264MI_ECAPACITY, before anything is launched
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_one_pack_launch_over_mixed_geometry(cases, H):
    """Rows a, c, g and h as four streams of one decoder, packed by ONE K6 launch: the grid is sized for the tallest frame, so the blocks beyond
    the 2x2 frame's six rows must write nothing; frames of odd byte size (173x137: 35707) shift the alignment of every later frame, which
    decides between the 16-byte and the byte path row by row."""
    rows = ["a_aligned_origin", "h_mono", "c_all_four", "g_16x16"]  # (the odd-sized frames in front of aligned ones)
    cs = [cases[r] for r in rows]
    dec = _decoder(H, 192, 144, 3, streams=4)
    try:
        dec.decode([c.stream for c in cs])
        want = np.concatenate([c.want.reshape(-1) for c in cs])
        assert cases["h_mono"].want.shape[1] % 2 == 1
        assert np.array_equal(_packed(dec, want.size, -1), want)
        for i, c in enumerate(cs):  # ... and every stream on its own, from offset 0
            assert np.array_equal(_packed(dec, c.want.size, i), c.want.reshape(-1)), rows[i]
            for f in range(3):
                _check_info(dec, i, f, c)
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_crop_change_without_a_size_change(cases, H):
    """Row b's stream followed by row c's in one chunk of one stream: the coded size stays, a new SPS (same id) arrives with the second IDR picture.
    Every frame is cropped by its own SPS -- in frame_info, in the host read and at its place in the packed batch."""
    b, c = cases["b_left_1"], cases["c_all_four"]
    assert (b.info["coded_w"], b.info["coded_h"]) == (c.info["coded_w"], c.info["coded_h"]) and b.rect != c.rect
    dec = _decoder(H, 176, 144, 6)
    try:
        dec.decode([b.stream + c.stream])
        assert dec.frame_count(0) == 6
        for f in range(6):
            k = b if f < 3 else c
            _check_info(dec, 0, f, k)
            assert np.array_equal(dec.read_frame_tight(0, f, crop=True), k.want[f % 3]), f
            assert np.array_equal(dec.read_frame_tight(0, f, crop=False), k.rec[f % 3]), f
        want = np.concatenate([b.want.reshape(-1), c.want.reshape(-1)])
        assert np.array_equal(_packed(dec, want.size, 0), want)
    finally:
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c_all_four", "h_mono"])
def test_gpu_front_end_delivers_the_display_size(name, cases, H):
    c = cases[name]
    got = []
    n = H.handleConnection(io.BytesIO(c.stream), on_frames=got.append, max_width=c.info["coded_w"], max_height=c.info["coded_h"], frames_per_batch=2, read_size=257)
    assert n == 3
    got = np.concatenate(got)
    assert got.shape == c.want.shape and np.array_equal(got, c.want)
    # ... and the batch server, which sizes every frame by its own frame_info
    seen = []
    srv = H.BatchServer(max_connections=1, max_width=c.info["coded_w"], max_height=c.info["coded_h"], frames_per_batch=2, on_frames=lambda i, f: seen.append(f))
    assert srv.add(io.BytesIO(c.stream)) == 0
    assert srv.run()[0] == 3
    seen = np.concatenate(seen)
    assert seen.shape == c.want.shape and np.array_equal(seen, c.want)


class _x_wgs:
    """H264MI_X_WGS for the decoders created inside (None: unset -- banded kernels; 0: a picture inside one workgroup)."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.old = os.environ.pop("H264MI_X_WGS", None)
        if self.n is not None:
            os.environ["H264MI_X_WGS"] = str(self.n)

    def __exit__(self, *a):
        os.environ.pop("H264MI_X_WGS", None)
        if self.old is not None:
            os.environ["H264MI_X_WGS"] = self.old


@pytest.mark.gpu
@pytest.mark.parametrize("x", [None, 0])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_gpu_smallest_pictures(name, x, small, H, oracle_mod):
    kw, stream, rec = small[name]
    ref, _ = oracle_mod.decode(stream, crop=False)
    assert np.array_equal(ref, rec), "oracle != generator"
    with _x_wgs(x):
        dec = _decoder(H, kw["width"], kw["height"], kw["frames"] * (2 if kw.get("field_pics") else 1), slices=kw.get("slices", 1))
        try:
            dec.decode([stream])
            out = dec.read_frames(0, crop=False)
        finally:
            dec.close()
    assert out.shape == rec.shape and np.array_equal(out, rec)


@pytest.mark.gpu
@pytest.mark.parametrize("x", [None, 0])
def test_gpu_smallest_pictures_in_one_batch(x, small, sg, H):
    """All six beside a 176x144 stream: launches whose pictures differ by a factor of 99 in macroblocks."""
    names = sorted(SMALL)
    big, big_rec, _ = sg.encode(**dict(IPP, width=176, height=144, profile_idc=77, cabac=1, seed=927))
    with _x_wgs(x):
        dec = _decoder(H, 176, 144, 6, streams=7, slices=4)
        try:
            dec.decode([small[n][1] for n in names] + [big])
            for i, n in enumerate(names):
                kw, _, rec = small[n]
                out = dec.read_frames(i, crop=False, size=kw["width"] * kw["height"] * 3 // 2)
                assert out.shape == rec.shape and np.array_equal(out, rec), n
            assert np.array_equal(dec.read_frames(6, crop=False), big_rec)
        finally:
            dec.close()
