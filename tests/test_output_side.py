"""Macroblock side information (K11): motion vectors, references, picture order count distances, macroblock classes, QP, coded-block flags and slice
ordinals of decoded frames as int16 planes per 4x4 luma block, laid out on the device.

The yardstick is tests/sideutil.py -- the contract of include/h264mi.h ("Macroblock side information") in numpy -- applied to the records
h264mi_frame_read_mbrecs / h264mi_frame_read_mbmv1 return, with the reference lists' picture order counts passed in as plain arrays.  The planes are a
function of those alone, so every GPU comparison is an equality.  The CPU tests pin the yardstick against answers worked out by hand, the pure entry
point h264mi_side_size against it, and h264mi_frame_ref_pocs -- through the null device -- against the initial lists of 8.2.4.2 stated here in Python.
Second opinions: the oracle's macroblock trace (QP, vector and reference of block 0), and the Python list rule for the distances."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import concealutil as cu
import hostprog
import sideutil as su
import spsutil
from concealutil import CONCEAL_MATRIX
from conftest import FIELD_MATRIX, MATRIX, pictures_of
from test_output_convert import TABLE

EINVAL, EUNSUPPORTED, ECAPACITY = -1, -3, -7
ALL = su.ALL
BIT = su.BIT
SUBSETS = [BIT["mvx0"] | BIT["mvy0"], BIT["type"] | BIT["qp"] | BIT["nz"] | BIT["slice"], BIT["dpoc1"]]
SENTINEL = 0xA5


# ------------------------------------------------------------------------------------------------ hand-made records
def _rec(t, qp=0, nz=0, slice_in_pic=0, ref0=(0, 0, 0, 0), slot0=(-1, -1, -1, -1), mv=None, ref1=(0, 0, 0, 0), slot1=(-1, -1, -1, -1)):
    r = np.zeros(128, np.uint8)
    r[0], r[2] = t, qp
    r[8:10] = np.array([nz], np.uint16).view(np.uint8)
    r[14:16] = np.array([slice_in_pic & 0xFFFF], np.uint16).view(np.uint8)
    r[16:20] = np.array(ref1, np.int8).view(np.uint8)
    r[32:36] = np.array(ref0, np.int8).view(np.uint8)
    r[36:44] = np.array(slot0, np.int16).view(np.uint8)
    r[44:48] = np.array([7], np.uint32).view(np.uint8)  # slice_idx: an index of the host's table, which the yardstick must not look at
    if mv is not None:
        r[48:112] = np.asarray(mv, np.int16).reshape(32).view(np.uint8)
    r[120:128] = np.array(slot1, np.int16).view(np.uint8)
    return r


def _plane(v, name):
    return v[su.NAMES.index(name)]


def test_yardstick_p8x8_and_intra_known_answers():
    """One 2 x 1 macroblock picture: a P_8x8 macroblock with sixteen distinct vectors and a reference per quadrant, and an intra macroblock whose record
    still carries slot words (they must not show)."""
    mv = [[10 * k + 1, -(10 * k + 2)] for k in range(16)]
    p = _rec(su.MB_P8x8, qp=31, nz=0x8421, slice_in_pic=2, ref0=(0, 1, 2, 0), slot0=(3, 4, 5, 3), mv=mv)
    i = _rec(3, qp=40, nz=0xFFFF, slice_in_pic=2, ref0=(0, 0, 0, 0), slot0=(0, 0, 0, 0), mv=[[99, 99]] * 16, slot1=(0, 0, 0, 0))
    pocs = {2: (20, [18, 14, 26], [])}
    v = su.frame(np.stack([p, i]), None, 2, 1, 0, 0, 32, 16, pocs)
    assert v.shape == (12, 4, 8) and v.dtype == np.int16
    assert _plane(v, "type").tolist() == [[8, 8, 8, 8, 3, 3, 3, 3]] * 4
    assert _plane(v, "qp").tolist() == [[31] * 4 + [40] * 4] * 4 and (_plane(v, "slice") == 2).all()
    assert _plane(v, "nz").tolist() == [[1, 0, 0, 0, 1, 1, 1, 1], [0, 1, 0, 0, 1, 1, 1, 1], [0, 0, 1, 0, 1, 1, 1, 1], [0, 0, 0, 1, 1, 1, 1, 1]]
    assert _plane(v, "mvx0")[:, :4].tolist() == [[1, 11, 21, 31], [41, 51, 61, 71], [81, 91, 101, 111], [121, 131, 141, 151]]
    assert _plane(v, "mvy0")[:, :4].tolist() == [[-2, -12, -22, -32], [-42, -52, -62, -72], [-82, -92, -102, -112], [-122, -132, -142, -152]]
    assert _plane(v, "ref0")[:, :4].tolist() == [[0, 0, 1, 1], [0, 0, 1, 1], [2, 2, 0, 0], [2, 2, 0, 0]]
    assert _plane(v, "dpoc0")[:, :4].tolist() == [[-2, -2, -6, -6], [-2, -2, -6, -6], [6, 6, -2, -2], [6, 6, -2, -2]]
    for name, none in (("mvx0", 0), ("mvy0", 0), ("ref0", -1), ("dpoc0", 0)):  # the intra macroblock
        assert (_plane(v, name)[:, 4:] == none).all(), name
    for name, none in (("mvx1", 0), ("mvy1", 0), ("ref1", -1), ("dpoc1", 0)):  # no list 1 anywhere
        assert (_plane(v, name) == none).all(), name
    # the selected planes come in ascending bit order
    sel = su.frame(np.stack([p, i]), None, 2, 1, 0, 0, 32, 16, pocs, BIT["dpoc0"] | BIT["qp"])
    assert sel.shape == (2, 4, 8) and np.array_equal(sel[0], _plane(v, "qp")) and np.array_equal(sel[1], _plane(v, "dpoc0"))


def test_yardstick_b_quadrants_and_concealed_known_answers():
    """A B macroblock with one quadrant per list pattern -- list 0 only, list 1 only, both, direct (both, derived) -- and a concealed record."""
    mv0 = [[k + 1, 2 * k + 1] for k in range(16)]
    mv1 = [[-(k + 1), 100 + k] for k in range(16)]
    b = _rec(su.MB_B, qp=26, slice_in_pic=0, ref0=(1, 0, 0, 1), slot0=(6, -1, 2, 6), mv=mv0, ref1=(0, 1, 0, 0), slot1=(-1, 9, 8, 8))
    c = _rec(su.MB_PSKIP, qp=28, slice_in_pic=0xFFFF, ref0=(0, 0, 0, 0), slot0=(5, 5, 5, 5))
    pocs = {0: (8, [4, 0], [12, 16]), -1: (8, [6], [])}
    v = su.frame(np.stack([b, c]), np.array([mv1, np.zeros((16, 2))], np.int16), 2, 1, 0, 0, 32, 16, pocs)
    q = lambda name: _plane(v, name)[::2, 0:4:2].reshape(4).tolist()  # the top-left cell of each quadrant
    assert q("ref0") == [1, -1, 0, 1] and q("ref1") == [-1, 1, 0, 0]
    assert q("dpoc0") == [-8, 0, -4, -8] and q("dpoc1") == [0, 8, 4, 4]
    assert q("mvx0") == [1, 0, 9, 11] and q("mvy0") == [1, 0, 17, 21] and q("mvx1") == [0, -3, -9, -11] and q("mvy1") == [0, 102, 108, 110]
    assert _plane(v, "mvx1")[0, :4].tolist() == [0, 0, -3, -4] and _plane(v, "mvx0")[3, :4].tolist() == [13, 14, 15, 16]
    conc = {n: _plane(v, n)[:, 4:] for n in su.NAMES}
    assert (conc["type"] == su.MB_PSKIP).all() and (conc["slice"] == -1).all() and (conc["ref0"] == 0).all() and (conc["dpoc0"] == -2).all()
    assert (conc["mvx0"] == 0).all() and (conc["ref1"] == -1).all() and (conc["dpoc1"] == 0).all() and (conc["qp"] == 28).all()
    # a record nobody delivered: all zero bytes, slot words included
    n = su.frame(np.zeros((1, 128), np.uint8), None, 1, 1, 0, 0, 16, 16, {})
    assert (_plane(n, "type") == 0).all() and (_plane(n, "slice") == -1).all() and (_plane(n, "ref0") == -1).all() and (_plane(n, "ref1") == -1).all()
    # distances are clamped to int16
    far = su.frame(np.stack([_rec(su.MB_P16x16, slot0=(1, 1, 1, 1))]), None, 1, 1, 0, 0, 16, 16, {0: (0, [1 << 20], [])})
    assert (_plane(far, "dpoc0") == 32767).all()


GRID_SHAPES = [(cx, cy, w, h) for cx in (0, 2, 6, 18) for cy in (0, 6) for w, h in ((1, 1), (4, 3), (5, 9), (170, 20))]


def test_yardstick_grid_arithmetic():
    """Cell (j, i) is the coded block ((crop_x >> 2) + i, (crop_y >> 2) + j): a 12 x 2 macroblock picture whose list-0 vector names its block."""
    wmb, hmb = 12, 2
    recs = np.stack([_rec(su.MB_P16x16, slot0=(0, 0, 0, 0), mv=[[4 * (m % wmb) + k % 4, 4 * (m // wmb) + k // 4] for k in range(16)]) for m in range(wmb * hmb)])
    for cx, cy, w, h in GRID_SHAPES:
        v = su.frame(recs, None, wmb, hmb, cx, cy, w, h, {}, BIT["mvx0"] | BIT["mvy0"])
        gw, gh = (w + 3) // 4, (h + 3) // 4
        assert v.shape == (2, gh, gw), (cx, cy, w, h)
        assert np.array_equal(v[0], np.tile(np.arange(gw) + (cx >> 2), (gh, 1))) and np.array_equal(v[1], np.tile((np.arange(gh) + (cy >> 2))[:, None], (1, gw)))
    assert su.size(ALL, 170, 138) == (43, 35, 2 * 43 * 35 * 12) and su.size(1, 1, 1) == (1, 1, 2) and su.size(BIT["ref1"] | 1, 5, 4) == (2, 1, 8)


def test_side_size_equals_the_yardstick(H):
    L = H.lib()
    gw, gh, n = ctypes.c_int32(-9), ctypes.c_int32(-9), ctypes.c_size_t(0)
    for _, _, w, h in GRID_SHAPES + [(0, 0, 16384, 16384), (0, 0, 1920, 1080)]:
        for bits in [ALL, 1, 0x800] + SUBSETS:
            assert L.h264mi_side_size(bits, w, h, ctypes.byref(gw), ctypes.byref(gh), ctypes.byref(n)) == 0
            assert (gw.value, gh.value, n.value) == su.size(bits, w, h) == H.Decoder.side_size(bits, w, h), (bits, w, h)
    assert H.Decoder.side_size(("mvx0", "dpoc1"), 170, 138) == su.size(BIT["mvx0"] | BIT["dpoc1"], 170, 138)
    assert L.h264mi_side_size(ALL, 8, 8, None, None, None) == 0
    for bits, w, h in ((0, 16, 16), (0x1000, 16, 16), (ALL | 0x4000, 16, 16), (-1, 16, 16), (ALL, 0, 16), (ALL, 16, 0), (ALL, 16385, 16), (ALL, 16, 16385), (ALL, -4, 4)):
        n.value = 77
        assert L.h264mi_side_size(bits, w, h, ctypes.byref(gw), ctypes.byref(gh), ctypes.byref(n)) == EINVAL, (bits, w, h)
        assert n.value == 77 and su.size(bits, w, h) is None
    assert tuple(1 << i for i in range(12)) == tuple(BIT[n] for n in su.NAMES) and H.SIDE_NAMES == su.NAMES and H.SIDE_ALL == ALL
    assert (H.MB_NONE, H.MB_IPCM, H.MB_P16x16, H.MB_P8x8, H.MB_PSKIP, H.MB_B, H.MB_BSKIP) == (0, 4, 5, 8, 9, 10, 12)


# ------------------------------------------------------------------------------------------------ the initial lists of 8.2.4.2, in Python
def initial_lists(frames, k, num_ref_frames, kind):
    """(list 0, list 1) of picture k as picture order counts.  frames: per frame in decoding order (poc, frame_num, nal_ref_idc, idr), frame pictures
    only, no list modification, no marking operations, no long-term pictures: the references are the last num_ref_frames reference frames since the last
    IDR picture (sliding window, 8.2.5.3).  P: descending PicNum (8.2.4.2.1) -- frame_num never wraps in these streams, asserted.  B: by picture order
    count distance (8.2.4.2.3); list 1 with its first two entries switched when it is longer than one entry and equal to list 0."""
    refs = []
    for poc, fn, ref_idc, idr in frames[:k]:
        if idr:
            refs = []
        if ref_idc:
            refs.append((poc, fn))
            refs = refs[-max(num_ref_frames, 1):]
    if frames[k][3]:
        refs = []
    cur = frames[k][0]
    if kind == "I":
        return [], []
    if kind == "P":
        assert all(fn < frames[k][1] for _, fn in refs), "frame_num wrapped: PicNum is not frame_num"
        return [p for p, _ in sorted(refs, key=lambda r: -r[1])], []
    before, after = sorted((p for p, _ in refs if p < cur), reverse=True), sorted(p for p, _ in refs if p > cur)
    l0, l1 = before + after, after + before
    if len(l1) > 1 and l1 == l0:
        l1[0], l1[1] = l1[1], l1[0]
    return l0, l1


def _headers(H, stream):
    """The slice headers of the stream, in stream order, with the SPS in force."""
    vs, out = H.VideoStream(), []
    for nu in H.read_nal_units(stream):
        if nu.Type == 7:
            vs.SPS = H.NewSPS(nu.RBSP())
        elif nu.Type == 8:
            vs.PPS = H.NewPPS(vs.SPS, nu.RBSP())
        elif nu.Type in (1, 5):
            out.append((H.NewSliceContext(vs, nu, nu.RBSP()).Slice.Header, vs.SPS))
    return out


def _parse_ref_pocs(text):
    """[(poc, frame_num, nal_ref_idc, idr, status, {slice: (cur, l0, l1)})] from the lines of tools/host_ref_pocs."""
    frames = []
    for ln in text.splitlines():
        p = ln.split()
        if p[0] == "F":
            frames.append([int(v) for v in p[1:6]] + [{}])
        elif p[0] == "S":
            bar = p.index("|")
            n0, n1 = int(p[3]), int(p[bar + 1])
            l0, l1 = [int(v) for v in p[4:bar]], [int(v) for v in p[bar + 2:]]
            assert len(l0) == n0 and len(l1) == n1
            frames[-1][5][int(p[1])] = (int(p[2]), l0, l1)
        elif p[0] == "C":
            frames[-1][5][-1] = (int(p[1]), [int(v) for v in p[3:]], [])
            assert len(p) - 3 == int(p[2])
    return frames


@pytest.fixture(scope="module")
def ref_pocs_prog(tmp_path_factory):
    return hostprog.build("host_ref_pocs.sh", tmp_path_factory.mktemp("host_ref_pocs"))


def _host_ref_pocs(prog, tmp_path, stream, kw, conceal=0):
    path = os.path.join(str(tmp_path), "s.h264")
    open(path, "wb").write(stream)
    r = subprocess.run([prog, path, str(kw["width"]), str(kw["height"]), str(pictures_of(kw)), "16", str(conceal)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return _parse_ref_pocs(r.stdout)


def _check_active_counts(H, stream, frames):
    """n of every slice and list is the slice header's active count (0 for the lists a slice type does not have)."""
    hdrs = _headers(H, stream)
    at = 0
    for fr in frames:
        for s in sorted(k for k in fr[5] if k >= 0):
            hd, _ = hdrs[at]
            at += 1
            st = hd.slice_type % 5
            cur, l0, l1 = fr[5][s]
            assert len(l0) == (hd.num_ref_idx_l0_active_minus1 + 1 if st != 2 else 0), (fr[:4], s)
            assert len(l1) == (hd.num_ref_idx_l1_active_minus1 + 1 if st == 1 else 0), (fr[:4], s)
    assert at == len(hdrs)
    return hdrs[0][1].max_num_ref_frames


PLAIN_LISTS = ["multiref_cabac", "multiref_cavlc", "b_ibp_cabac", "b_ibbp_cavlc", "b_pyramid_cabac", "poc1_nonref", "slices_idc_cycle"]


def _kind(l0, l1):
    return "B" if l1 else ("P" if l0 else "I")


@pytest.mark.parametrize("name", PLAIN_LISTS)
def test_ref_pocs_equal_the_initial_lists(name, H, sg, ref_pocs_prog, tmp_path):
    kw = MATRIX[name]
    stream = sg.encode(want_recon=False, **kw)[0]
    frames = _host_ref_pocs(ref_pocs_prog, tmp_path, stream, kw)
    assert len(frames) == kw["frames"] and all(fr[4] == 0 for fr in frames)
    nrf = _check_active_counts(H, stream, frames)
    plain = [tuple(fr[:4]) for fr in frames]
    kinds = set()
    for k, fr in enumerate(frames):
        assert sorted(fr[5]) == [-1] + list(range(kw.get("slices", 1))), (k, sorted(fr[5]))
        assert fr[5][-1] == (fr[0], [], []), "no concealment: no concealment reference"
        for s, (cur, l0, l1) in fr[5].items():
            if s < 0:
                continue
            assert cur == fr[0], (k, s)
            w0, w1 = initial_lists(plain, k, nrf, _kind(l0, l1))
            assert len(w0) >= len(l0) and len(w1) >= len(l1), (k, s, w0, w1, l0, l1)
            assert l0 == w0[:len(l0)] and l1 == w1[:len(l1)], (k, s, l0, w0, l1, w1)
            kinds.add(_kind(l0, l1))
    assert kinds == ({"I", "P", "B"} if kw.get("bframes") else {"I", "P"})
    if name.startswith("multiref"):
        assert any(len(fr[5][0][1]) > 1 for fr in frames), "a list of several entries"


@pytest.mark.parametrize("name", ["rplm_cabac", "mmco_idr_lt", "poc_bottom_first_mmco5"])
def test_ref_pocs_of_modified_lists_name_earlier_reference_frames(name, H, sg, ref_pocs_prog, tmp_path):
    kw = MATRIX[name]
    stream = sg.encode(want_recon=False, **kw)[0]
    frames = _host_ref_pocs(ref_pocs_prog, tmp_path, stream, kw)
    assert len(frames) == kw["frames"] and all(fr[4] == 0 for fr in frames)
    _check_active_counts(H, stream, frames)
    hdrs = [h for h, _ in _headers(H, stream)]
    assert len(hdrs) == len(frames)  # one slice per picture
    earlier, n_op5 = [], 0
    for k, fr in enumerate(frames):
        if fr[3]:
            earlier = []
        cur, l0, l1 = fr[5][0]
        for p in l0 + l1:
            assert p in earlier, (k, p, earlier)
        op5 = bool(hdrs[k].nal_ref_idc and hdrs[k].adaptive_ref_pic_marking_mode_flag and
                   5 in list(hdrs[k].memory_management_control_operation[:hdrs[k].n_memory_management_control_operations]))
        if op5:  # the count before operation 5 rewrites it: above every reference's (P pictures in output order), and not what is reported afterwards
            n_op5 += 1
            assert l0 and cur > max(l0) and cur != fr[0] and fr[0] <= 1, (k, cur, fr[0], l0)
            earlier = []
        else:
            assert cur == fr[0], (k, cur, fr[0])
        if fr[2]:
            earlier.append(fr[0])  # (after operation 5: the rewritten count, which is what later lists were built with)
    if name == "poc_bottom_first_mmco5":
        assert n_op5 >= 1
    if name == "rplm_cabac":  # some list is not the initial one
        plain = [tuple(fr[:4]) for fr in frames]
        nrf = _headers(H, stream)[0][1].max_num_ref_frames
        assert any(fr[5][0][1] != initial_lists(plain, k, nrf, "P")[0][:len(fr[5][0][1])] for k, fr in enumerate(frames) if fr[5][0][1])


def test_ref_pocs_concealment_pseudo_slice_on_the_host(H, sg, ref_pocs_prog, tmp_path):
    """With conceal_errors every non-IDR frame picture that has a reference reports it as the one entry of slice -1: entry 0 of the initial P list."""
    kw = MATRIX["multiref_cabac"]
    stream = sg.encode(want_recon=False, **kw)[0]
    frames = _host_ref_pocs(ref_pocs_prog, tmp_path, stream, kw, conceal=1)
    plain = [tuple(fr[:4]) for fr in frames]
    for k, fr in enumerate(frames):
        want = initial_lists(plain, k, 3, "P")[0][:1] if not fr[3] else []
        assert fr[5][-1] == (fr[0], want, []), (k, fr[5][-1], want)
    assert sum(len(fr[5][-1][1]) for fr in frames) == kw["frames"] - 1


# ------------------------------------------------------------------------------------------------ GPU
def _decoder(H, kw, streams=1, w=None, h=None, frames=None, **cfg):
    W, Hc = ((w or kw["width"]) + 15) // 16 * 16, ((h or kw["height"]) + 15) // 16 * 16
    return H.Decoder(max_streams=streams, max_width=W, max_height=Hc, max_frames_per_batch=frames or pictures_of(kw), max_slices_per_frame=16, **cfg)


def _slice_pocs(dec, stream, frame):
    out = {}
    for s in range(-1, 64):
        try:
            cur, l0 = dec.ref_pocs(stream, frame, s, 0)
        except Exception:
            break
        out[s] = (cur, l0, dec.ref_pocs(stream, frame, s, 1)[1])
    return out


def _picture_order(dec, stream, frame):
    """`frame` of h264mi_frame_read_mbrecs counts PICTURES of the stream in the batch: a frame coded as two fields is two of them."""
    return sum(2 if dec.frame_fields(stream, f).field_coded else 1 for f in range(frame))


def _want(dec, stream, frame, bits=ALL):
    """The yardstick's planes of one frame picture of the last executed batch (synchronises)."""
    fi = dec.frame_info(stream, frame)
    wmb, hmb = fi.coded_width // 16, fi.coded_height // 16
    order = _picture_order(dec, stream, frame)
    v = su.frame(dec.read_mbrecs(stream, order, wmb * hmb), dec.read_mbmv1(stream, order, wmb * hmb), wmb, hmb, fi.crop_x, fi.crop_y, fi.width, fi.height,
                 _slice_pocs(dec, stream, frame), bits)
    v.setflags(write=False)
    return v


def _select(v, bits):
    return v[[i for i in range(12) if bits & (1 << i)]]


def _launch(dec, bits, stream=-1, items=None, nbytes=None, pad=64):
    """One K11 launch into a device buffer full of sentinel bytes: (bytes written, the buffer on the host).  Everything behind `bytes` still holds the sentinel."""
    import torch
    buf = torch.full((nbytes + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    got = dec.side_batch(buf.data_ptr(), nbytes, bits, stream) if items is None else dec.side_items(buf.data_ptr(), nbytes, bits, items)
    dec.sync()
    host = buf.cpu().numpy()
    assert (host[got:] == SENTINEL).all(), "K11 wrote behind the bytes it reports"
    return got, host[:got]


def _flat(wants):
    return np.concatenate([w.reshape(-1) for w in wants]).view(np.uint8) if wants else np.zeros(0, np.uint8)


def _first_diff(got, want):
    d = np.flatnonzero(got.view(np.int16) != want.view(np.int16))
    return None if d.size == 0 else (int(d[0]), int(got.view(np.int16)[d[0]]), int(want.view(np.int16)[d[0]]))


RECIPES = ["sub8x8_heavy", "frac_motion_sub8x8", "multiref_cabac", "weighted_pred", "pcm_qpjitter_cabac", "high8x8_cabac", "slice_qp_delta", "fmo_dispersed_aso",
           "b_ibbp_cabac", "b_temporal_cabac", "b_wp_implicit", "b_high8x8_slices", "b_gop_intra_pcm", "poc_bottom_first_mmco5", "mono_cropped_cavlc_qpel",
           "crop_3byte_sc", "field_mixed_paff"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", RECIPES)
def test_gpu_planes_equal_the_yardstick(name, H, sg):
    kw = dict(MATRIX, **FIELD_MATRIX)[name]
    stream = sg.encode(want_recon=False, **kw)[0]
    dec = _decoder(H, kw)
    try:
        dec.decode([stream])
        n = dec.frame_count(0)
        assert n == kw["frames"]
        coded = [dec.frame_fields(0, f).field_coded for f in range(n)]
        served = [f for f in range(n) if not coded[f]]
        if name == "field_mixed_paff":
            assert served and len(served) < n
            for f in (f for f in range(n) if coded[f]):  # a frame of two field pictures: refused, nothing written
                one = su.size(ALL, kw["width"], kw["height"])[2]
                import torch
                buf = torch.full((one,), SENTINEL, dtype=torch.uint8, device="cuda")
                with pytest.raises(H.H264MIError) as ei:
                    dec.side_items(buf.data_ptr(), one, ALL, [(0, served[0]), (0, f)])
                assert ei.value.code == EUNSUPPORTED and "field" in str(ei.value)
                dec.sync()
                assert (buf.cpu().numpy() == SENTINEL).all()
                with pytest.raises(H.H264MIError) as ei:
                    dec.ref_pocs(0, f, 0, 0)
                assert ei.value.code == EUNSUPPORTED
            with pytest.raises(H.H264MIError) as ei:
                dec.side_batch(buf.data_ptr(), one, ALL, 0)
            assert ei.value.code == EUNSUPPORTED
        else:
            assert len(served) == n
        wants = [_want(dec, 0, f) for f in served]
        items = [(0, f) for f in served]
        gw, gh, one = su.size(ALL, kw["width"], kw["height"])
        assert wants[0].shape == (12, gh, gw)
        if name in ("mono_cropped_cavlc_qpel", "crop_3byte_sc"):
            assert gw % 4, "the element path"
        for bits in [ALL] + SUBSETS:
            want = _flat([_select(w, bits) for w in wants])
            got, host = _launch(dec, bits, items=items, nbytes=want.size)
            assert got == want.size == len(served) * su.size(bits, kw["width"], kw["height"])[2]
            assert np.array_equal(host, want), (name, bits, _first_diff(host, want))
        if name != "field_mixed_paff":  # the batch call is the item call over every frame
            got, host = _launch(dec, ALL, stream=0, nbytes=len(served) * one)
            assert np.array_equal(host, _flat(wants))
        # what the recipe is here for
        t = np.concatenate([_plane(w, "type").reshape(-1) for w in wants])
        if name == "sub8x8_heavy":
            assert (t == H.MB_P8x8).any() and (t == H.MB_PSKIP).any()
            per_block = [w for w in wants if (np.diff(_plane(w, "mvx0"), axis=1) != 0)[_plane(w, "type")[:, 1:] == H.MB_P8x8].any()]
            assert per_block, "vectors differ between the 4x4 blocks of a macroblock"
        if name == "pcm_qpjitter_cabac":
            pcm = t == H.MB_IPCM
            qp = np.concatenate([_plane(w, "qp").reshape(-1) for w in wants])
            nz = np.concatenate([_plane(w, "nz").reshape(-1) for w in wants])
            assert pcm.any() and (qp[pcm] == 0).all() and (nz[pcm] == 1).all() and len(set(qp[~pcm].tolist())) > 3
        if name == "high8x8_cabac":
            nz = np.concatenate([_plane(w, "nz").reshape(-1, gw) for w in wants])
            t8 = np.concatenate([_plane(w, "type").reshape(-1, gw) for w in wants]) == H.MB_I8x8
            assert t8.any() and (nz[0::2, 0::2][t8[0::2, 0::2]] == nz[1::2, 1::2][t8[1::2, 1::2]]).all() and nz[t8].any()
        if name in ("slice_qp_delta", "fmo_dispersed_aso", "b_high8x8_slices"):
            sl = np.concatenate([_plane(w, "slice").reshape(-1) for w in wants])
            assert sorted(set(sl.tolist())) == list(range(cu.nslices(kw)))
        if name == "fmo_dispersed_aso":  # dispersed: horizontally adjacent macroblocks belong to different slice groups, hence slices
            sl = _plane(wants[1], "slice")
            assert (sl[:, 3:-1:4] != sl[:, 4::4]).all()
        if kw.get("bframes"):
            r0 = np.concatenate([_plane(w, "ref0").reshape(-1) for w in wants])
            r1 = np.concatenate([_plane(w, "ref1").reshape(-1) for w in wants])
            d1 = np.concatenate([_plane(w, "dpoc1").reshape(-1) for w in wants])
            assert ((r0 >= 0) & (r1 >= 0)).any() and ((r0 < 0) & (r1 >= 0)).any() and ((r0 >= 0) & (r1 < 0)).any() and (d1 > 0).any()
            if kw.get("bskip_permille"):
                assert (t == H.MB_BSKIP).any() or (t == H.MB_BDIRECT).any()
        if name == "multiref_cabac":
            assert (np.concatenate([_plane(w, "ref0").reshape(-1) for w in wants]) > 0).any()
    finally:
        dec.close()


GEOMETRY = {name: (dict(TABLE[name][0], seed=2501 + i), TABLE[name][1]) for i, name in enumerate(sorted(TABLE))}
GEOMETRY["left_6"] = (dict(frames=3, idr_period=0, width=176, height=144, profile_idc=77, cabac=1, sub8x8_permille=400, seed=2511), (3, 2, 0, 0))    # block offset 1, 166 wide
GEOMETRY["left_18"] = (dict(frames=3, idr_period=0, width=176, height=144, profile_idc=66, cabac=0, sub8x8_permille=400, seed=2512), (9, 1, 1, 3))  # block offset 4, 156 wide


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_gpu_geometry(name, H, sg):
    kw, crop = GEOMETRY[name]
    raw = sg.encode(want_recon=False, **kw)[0]
    stream, info = spsutil.recrop(raw, *crop) if any(crop) else (raw, dict(coded_w=kw["width"], coded_h=kw["height"], chroma_format_idc=0 if kw.get("mono") else 1, frame_mbs_only=1))
    dec = _decoder(H, kw, w=info["coded_w"], h=info["coded_h"])
    try:
        dec.decode([stream])
        n = dec.frame_count(0)
        assert n == kw["frames"]
        fi = dec.frame_info(0, 0)
        if any(crop):
            assert (fi.crop_x, fi.crop_y, fi.width, fi.height) == spsutil.crop_rect(info, *crop)
        if name == "left_6":
            assert (fi.crop_x >> 2, fi.width) == (1, 166) and ((fi.crop_x >> 2) + (fi.width + 3) // 4) % 4 != 0
        if name == "left_18":
            assert (fi.crop_x >> 2, fi.width) == (4, 156) and ((fi.crop_x >> 2) + (fi.width + 3) // 4) % 4 != 0
        one = su.size(ALL, fi.width, fi.height)[2]
        if kw.get("field_pics"):  # every frame of this row is two field pictures: refused, nothing written
            import torch
            buf = torch.full((n * one,), SENTINEL, dtype=torch.uint8, device="cuda")
            with pytest.raises(H.H264MIError) as ei:
                dec.side_batch(buf.data_ptr(), n * one, ALL)
            assert ei.value.code == EUNSUPPORTED
            dec.sync()
            assert (buf.cpu().numpy() == SENTINEL).all()
            return
        wants = [_want(dec, 0, f) for f in range(n)]
        for bits in (ALL, SUBSETS[0]):
            want = _flat([_select(w, bits) for w in wants])
            got, host = _launch(dec, bits, nbytes=want.size)
            assert got == want.size and np.array_equal(host, want), (name, bits, _first_diff(host, want))
        # an odd destination for the items behind the first: frame 1 alone, two bytes into the buffer's 8-byte grid
        import torch
        buf = torch.full((one + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert dec.side_items(buf.data_ptr() + 2, one, ALL, [(0, 1)]) == one
        dec.sync()
        host = buf.cpu().numpy()
        assert (host[:2] == SENTINEL).all() and (host[2 + one:] == SENTINEL).all() and np.array_equal(host[2:2 + one], _flat([wants[1]]))
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_mixed_launch(H, sg):
    """Three streams of unlike size and slice type in one decoder: the batch call is the concatenation, stream-major; an items call takes a permuted
    order and a repeated frame."""
    names = ["cavlc_I", "crop_3byte_sc", "b_ibp_cabac"]
    kws = [MATRIX[n] for n in names]
    streams = [sg.encode(want_recon=False, **kw)[0] for kw in kws]
    dec = H.Decoder(max_streams=3, max_width=192, max_height=144, max_frames_per_batch=max(kw["frames"] for kw in kws), max_slices_per_frame=4)
    try:
        dec.decode(streams)
        frames = [(s, f) for s in range(3) for f in range(dec.frame_count(s))]
        assert len(frames) == sum(kw["frames"] for kw in kws)
        wants = {sf: _want(dec, *sf) for sf in frames}
        assert len({w.shape for w in wants.values()}) == 3
        for bits in (ALL, SUBSETS[2] | BIT["mvy1"]):
            want = _flat([_select(wants[sf], bits) for sf in frames])
            got, host = _launch(dec, bits, nbytes=want.size)
            assert got == want.size and np.array_equal(host, want), (bits, _first_diff(host, want))
        one = [sf for sf in frames if sf[0] == 2]
        want = _flat([wants[sf] for sf in one])
        got, host = _launch(dec, ALL, stream=2, nbytes=want.size)
        assert np.array_equal(host, want)
        items = [frames[-1], frames[0], frames[4], frames[-1], frames[2], frames[4]]
        want = _flat([wants[sf] for sf in items])
        got, host = _launch(dec, ALL, items=items, nbytes=want.size)
        assert got == want.size and np.array_equal(host, want), _first_diff(host, want)
    finally:
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["frac_motion_cabac", "multiref_cabac", "b_ibbp_cabac"])
def test_gpu_block0_equals_the_oracle_trace(name, H, sg, oracle_mod):
    """Second opinion: the oracle's macroblock trace (decoding order, raster macroblock order) against the cell of every macroblock's block 0."""
    kw = MATRIX[name]
    stream = sg.encode(want_recon=False, **kw)[0]
    _, info, tr = oracle_mod.decode(stream, crop=False, trace=True)
    wmb, hmb = kw["width"] // 16, kw["height"] // 16
    tr = tr.reshape(kw["frames"], hmb, wmb, 8)
    dec = _decoder(H, kw)
    try:
        dec.decode([stream])
        bits = BIT["qp"] | BIT["mvx0"] | BIT["mvy0"] | BIT["ref0"]
        one = su.size(bits, kw["width"], kw["height"])[2]
        got, host = _launch(dec, bits, nbytes=kw["frames"] * one)
        v = host.view(np.int16).reshape(kw["frames"], 4, 4 * hmb, 4 * wmb)[:, :, ::4, ::4]
        ref = tr[..., 7].copy()
        ref[ref <= -50] += 100  # macroblocks of B slices are marked by -100
        n_b = int((tr[..., 7] <= -50).sum())
        assert (n_b > 0) == bool(kw.get("bframes"))
        for k, (label, want) in enumerate((("qp", tr[..., 2]), ("mvx0", tr[..., 5]), ("mvy0", tr[..., 6]), ("ref0", ref))):
            bad = np.argwhere(v[:, k] != want)
            assert bad.size == 0, (name, label, bad[:4].tolist(), v[:, k][tuple(bad[0])], want[tuple(bad[0])])
        assert (v[:, 1] != 0).any() and (ref >= 0).any() and (ref < 0).any()
    finally:
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PLAIN_LISTS)
def test_gpu_dpoc_equals_the_python_list_rule(name, H, sg):
    kw = MATRIX[name]
    stream = sg.encode(want_recon=False, **kw)[0]
    nrf = _headers(H, stream)[0][1].max_num_ref_frames
    dec = _decoder(H, kw)
    try:
        dec.decode([stream])
        n = dec.frame_count(0)
        plain = []
        for f in range(n):
            fi = dec.frame_info(0, f)
            plain.append((fi.pic_order_cnt, fi.frame_num, fi.nal_ref_idc, fi.idr))
        bits = BIT["slice"] | BIT["ref0"] | BIT["dpoc0"] | BIT["ref1"] | BIT["dpoc1"]
        gw, gh, one = su.size(bits, kw["width"], kw["height"])
        got, host = _launch(dec, bits, nbytes=n * one)
        v = host.view(np.int16).reshape(n, 5, gh, gw)
        seen = 0
        for f in range(n):
            sl, r0, d0, r1, d1 = v[f]
            assert (sl >= 0).all()
            kinds = {s: _kind(*dec.ref_pocs(0, f, s, 0)[1:], dec.ref_pocs(0, f, s, 1)[1]) for s in set(sl.reshape(-1).tolist())}
            for s, kind in kinds.items():
                lists = initial_lists(plain, f, nrf, kind)
                for r, d, lst in ((r0, d0, lists[0]), (r1, d1, lists[1])):
                    m = sl == s
                    want = np.zeros_like(d)
                    for e in set(r[m & (r >= 0)].tolist()):
                        want[m & (r == e)] = lst[e] - plain[f][0]
                    assert np.array_equal(d[m], want[m]), (name, f, s, kind)
                    seen += int((want[m] != 0).sum())
        assert seen > 0
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_concealed_macroblocks(H, sg):
    name = "cabac_wp1_multiref"
    kw = CONCEAL_MATRIX[name]
    stream = sg.encode(want_recon=False, **kw)[0]
    damaged, repaired, per_picture, n_slices = cu.make(stream, mode="lost")
    lost, _ = cu.lost_mbs(stream)
    dec = _decoder(H, kw, conceal_errors=True)
    try:
        dec.decode([damaged])
        n = dec.frame_count(0)
        assert [dec.frame_concealed(0, f) for f in range(n)] == per_picture and sum(per_picture) > 0
        wmb, hmb = (kw["width"] + 15) // 16, (kw["height"] + 15) // 16
        gw, gh, one = su.size(ALL, kw["width"], kw["height"])
        wants = [_want(dec, 0, f) for f in range(n)]
        got, host = _launch(dec, ALL, nbytes=n * one)
        assert np.array_equal(host, _flat(wants)), _first_diff(host, _flat(wants))
        v = host.view(np.int16).reshape(n, 12, gh, gw)
        for f in range(n):
            mask = np.zeros((hmb, wmb), bool)
            for a in lost.get(f, []):
                mask[a // wmb, a % wmb] = True
            assert int(mask.sum()) == per_picture[f]
            cells = np.repeat(np.repeat(mask, 4, axis=0), 4, axis=1)[:gh, :gw]
            pl = {nme: v[f, i] for i, nme in enumerate(su.NAMES)}
            assert ((pl["slice"] == -1) == cells).all(), f
            if not per_picture[f]:
                continue
            cur, pocs = dec.ref_pocs(0, f, -1, 0)
            assert len(pocs) == 1 and pocs[0] != cur
            assert (pl["type"][cells] == H.MB_PSKIP).all() and (pl["ref0"][cells] == 0).all() and (pl["dpoc0"][cells] == pocs[0] - cur).all()
            assert (pl["mvx0"][cells] == 0).all() and (pl["mvy0"][cells] == 0).all() and (pl["ref1"][cells] == -1).all()
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_contract_edges(H, sg):
    import torch
    kw = MATRIX["cabac_IPP"]
    stream = sg.encode(want_recon=False, **kw)[0]
    L = H.lib()
    dec = _decoder(H, kw)
    try:
        n, nb = ctypes.c_size_t(77), ctypes.c_size_t(78)
        buf = torch.full((1 << 20,), SENTINEL, dtype=torch.uint8, device="cuda")
        # before any execute: whatever the pack call gives
        r_pack = L.h264mi_batch_pack_device(dec._h, -1, buf.data_ptr(), 1 << 20, ctypes.byref(nb))
        assert L.h264mi_batch_side_device(dec._h, -1, ALL, buf.data_ptr(), 1 << 20, ctypes.byref(n)) == r_pack and n.value == nb.value == 0
        dec.decode([stream])
        frames = dec.frame_count(0)
        one = su.size(ALL, kw["width"], kw["height"])[2]
        item = H._lib.SideItem
        arr = (item * 2)(item(0, 1), item(0, 0))
        # one byte short: the size is reported, nothing is written
        n.value = 0
        assert L.h264mi_batch_side_device(dec._h, -1, ALL, buf.data_ptr(), frames * one - 1, ctypes.byref(n)) == ECAPACITY and n.value == frames * one
        n.value = 0
        assert L.h264mi_items_side_device(dec._h, ALL, arr, 2, buf.data_ptr(), 2 * one - 1, ctypes.byref(n)) == ECAPACITY and n.value == 2 * one
        # n = 0 succeeds
        n.value = 5
        assert L.h264mi_items_side_device(dec._h, ALL, None, 0, buf.data_ptr(), 0, ctypes.byref(n)) == 0 and n.value == 0
        assert L.h264mi_items_side_device(dec._h, ALL, arr, 0, buf.data_ptr(), 0, None) == 0
        # planes, streams, items, pointers
        for bits in (0, 0x1000, -1, ALL | 0x10000):
            assert L.h264mi_batch_side_device(dec._h, -1, bits, buf.data_ptr(), 1 << 20, ctypes.byref(n)) == EINVAL, bits
            assert L.h264mi_items_side_device(dec._h, bits, arr, 2, buf.data_ptr(), 1 << 20, ctypes.byref(n)) == EINVAL, bits
            assert L.h264mi_items_side_device(dec._h, bits, arr, 0, buf.data_ptr(), 1 << 20, ctypes.byref(n)) == EINVAL, bits
        assert dec.deinterlace(0, "field") == frames  # the derived pseudo-stream exists, and has no macroblocks
        assert L.h264mi_batch_side_device(dec._h, H.STREAM_DERIVED, ALL, buf.data_ptr(), 1 << 20, ctypes.byref(n)) == EINVAL
        for bad in ((H.STREAM_DERIVED, 0), (0, frames), (0, -1), (1, 0), (-1, 0)):
            arr2 = (item * 2)(item(0, 0), item(*bad))
            assert L.h264mi_items_side_device(dec._h, ALL, arr2, 2, buf.data_ptr(), 1 << 20, ctypes.byref(n)) == EINVAL, bad
        cur, cnt = ctypes.c_int32(0), ctypes.c_int32(0)
        assert L.h264mi_frame_ref_pocs(dec._h, H.STREAM_DERIVED, 0, 0, 0, ctypes.byref(cur), None, 0, ctypes.byref(cnt)) == EINVAL
        assert L.h264mi_frame_ref_pocs(dec._h, 0, 1, 0, 2, ctypes.byref(cur), None, 0, ctypes.byref(cnt)) == EINVAL
        assert L.h264mi_frame_ref_pocs(dec._h, 0, 1, 1, 0, ctypes.byref(cur), None, 0, ctypes.byref(cnt)) == EINVAL  # one slice per picture
        assert L.h264mi_frame_ref_pocs(dec._h, 0, 1, 0, 0, ctypes.byref(cur), None, 0, ctypes.byref(cnt)) == ECAPACITY and cnt.value >= 1
        assert L.h264mi_frame_ref_pocs(dec._h, 0, 0, 0, 0, None, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == 0  # the IDR picture
        for stream_id in (-2, 1):
            assert L.h264mi_batch_side_device(dec._h, stream_id, ALL, buf.data_ptr(), 1 << 20, ctypes.byref(n)) == EINVAL
        assert L.h264mi_batch_side_device(dec._h, -1, ALL, None, 1 << 20, ctypes.byref(n)) == EINVAL
        assert L.h264mi_batch_side_device(None, -1, ALL, buf.data_ptr(), 1 << 20, ctypes.byref(n)) == EINVAL
        assert L.h264mi_items_side_device(dec._h, ALL, None, 1, buf.data_ptr(), 1 << 20, ctypes.byref(n)) == EINVAL
        assert L.h264mi_items_side_device(dec._h, ALL, arr, -1, buf.data_ptr(), 1 << 20, ctypes.byref(n)) == EINVAL
        assert L.h264mi_batch_side_device(dec._h, -1, ALL, buf.data_ptr() + 1, 1 << 20, ctypes.byref(n)) == EINVAL  # int16 planes at an odd address
        dec.sync()
        assert (buf.cpu().numpy() == SENTINEL).all(), "a refused call wrote something"
        # ... and the call that fits exactly
        wants = [_want(dec, 0, f) for f in range(frames)]
        got, host = _launch(dec, ALL, nbytes=frames * one, pad=0)
        assert got == frames * one and np.array_equal(host, _flat(wants))
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_fence_of_the_record_sets(H, sg):
    """K11 reads the macroblock records of the pass executed last; the pass three executes on rewrites that set on a stream of its own.  The launch is
    recorded, the next execute takes it, and the planes of the FIRST batch -- launched before three further executes, no synchronisation in between --
    equal the yardstick; the pixels of all four batches are what the generator reconstructed."""
    import torch
    pending = H.load_hooks().h264mi_internal_side_pending

    def is_pending(dec):
        v = ctypes.c_int32(-1)
        assert pending(dec._h, ctypes.byref(v)) == 0
        return v.value
    kws = [dict(MATRIX["sub8x8_heavy"], seed=2601 + i, frames=4) for i in range(4)]
    enc = [sg.encode(**kw) for kw in kws]
    streams, recs = [e[0] for e in enc], [e[1] for e in enc]
    kw = kws[0]
    gw, gh, one = su.size(ALL, kw["width"], kw["height"])
    pix = spsutil.i420_size(kw["width"], kw["height"])
    ref_dec = _decoder(H, kw)
    try:
        ref_dec.decode([streams[0]])
        wants = [_want(ref_dec, 0, f) for f in range(4)]
    finally:
        ref_dec.close()
    dec = _decoder(H, kw)
    try:
        side = torch.full((4 * one + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        packs = [torch.full((4 * pix,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(4)]
        assert is_pending(dec) == 0
        dec.prepare([streams[0]])
        dec.execute()
        assert is_pending(dec) == 0, "no K11 call: no event, execute does what it always did"
        assert dec.side_batch(side.data_ptr(), 4 * one, ALL) == 4 * one
        assert is_pending(dec) == 1, "the K11 launch is recorded for the next execute's entropy stream"
        assert dec.pack_batch(packs[0].data_ptr(), 4 * pix) == 4 * pix
        for k in (1, 2, 3):
            dec.prepare([streams[k]])
            dec.execute()
            assert is_pending(dec) == 0, "taken by the execute that follows"
            assert dec.pack_batch(packs[k].data_ptr(), 4 * pix) == 4 * pix
        dec.sync()
        host = side.cpu().numpy()
        assert (host[4 * one:] == SENTINEL).all()
        assert np.array_equal(host[:4 * one], _flat(wants)), _first_diff(host[:4 * one], _flat(wants))
        for k in range(4):
            assert np.array_equal(packs[k].cpu().numpy().reshape(4, pix), recs[k]), "pixels of batch %d" % k
        # the records K11 would read now are the last batch's
        assert not np.array_equal(_flat([_want(dec, 0, f) for f in range(4)]), _flat(wants))
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_python_side_info(H, sg):
    kws = [MATRIX["b_ibp_cabac"], MATRIX["crop_3byte_sc"]]
    streams = [sg.encode(want_recon=False, **kw)[0] for kw in kws]
    dec = H.Decoder(max_streams=2, max_width=192, max_height=144, max_frames_per_batch=9, max_slices_per_frame=4)
    try:
        dec.decode(streams)
        frames = [(s, f) for s in range(2) for f in range(dec.frame_count(s))]
        wants = {sf: _want(dec, *sf) for sf in frames}
        views = dec.side_info()
        assert len(views) == len(frames)
        for sf, v in zip(frames, views):
            assert v.dtype.is_floating_point is False and tuple(v.shape) == wants[sf].shape and v.is_cuda
            assert np.array_equal(v.cpu().numpy(), wants[sf]), sf
        names = ("mvx0", "mvy0", "ref0", "dpoc0")
        views = dec.side_info(stream=1, planes=names)
        assert len(views) == kws[1]["frames"]
        for f, v in enumerate(views):
            assert np.array_equal(v.cpu().numpy(), _select(wants[(1, f)], sum(BIT[n] for n in names)))
        views = dec.side_info(planes=("type",), items=[(0, 3), (1, 0), (0, 3)])
        assert [tuple(v.shape) for v in views] == [(1, 36, 44), (1, 25, 45), (1, 36, 44)]
        assert np.array_equal(views[2].cpu().numpy(), wants[(0, 3)][:1]) and np.array_equal(views[1].cpu().numpy(), wants[(1, 0)][:1])
        assert dec.side_info(items=[]) == []
        with pytest.raises(H.H264MIError):
            dec.side_info(planes=("mvx2",))
    finally:
        dec.close()
