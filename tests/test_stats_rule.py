"""Frame statistics (K12), the rule on the CPU: the yardstick tests/statsutil.py held to answers worked out by hand, the invariants of the contract
("Frame statistics" of include/h264mi.h), and the pure entry point h264mi_stats_size held to the yardstick.  The samples on the device:
tests/test_output_stats.py; the host state: tests/test_host_stats.py."""
import ctypes

import numpy as np
import pytest

import statsutil as su
from h264decode_amd import STATS_CELL_SAD, STATS_CELL_SUM, STATS_PREV_HISTORY, STATS_PREV_NONE  # (the package's names of the contract's constants)

EINVAL = -1


def _i420(y, cb, cr):
    return np.concatenate([np.asarray(p, np.uint8).reshape(-1) for p in (y, cb, cr)])


def test_known_answers_3x3():
    """3 x 3 luma, 2 x 2 chroma (odd sizes round up); one cell of size 8, partial in both directions."""
    S = _i420([[1, 2, 3], [4, 5, 6], [7, 8, 9]], [10, 20, 30, 40], [50, 60, 70, 80])
    P = _i420([[1, 2, 3], [4, 0, 6], [7, 8, 19]], [10, 20, 30, 45], [49, 60, 70, 80])
    assert S.size == 9 + 4 + 4
    r = su.record(S, P, 3, 3, 5)
    want = dict(sum_y=45, sum_y2=285, sum_cb=100, sum_cr=260, sad_y=5 + 10, sse_y=25 + 100, sad_cb=5, sad_cr=1, min_y=1, max_y=9, changed_y=1, has_prev=1, w=3, h=3)
    assert {k: r[k] for k in want} == want
    assert su.record(S, P, 3, 3, 4)["changed_y"] == 2 and su.record(S, P, 3, 3, 10)["changed_y"] == 0 and su.record(S, P, 3, 3, 9)["changed_y"] == 1
    assert r["hist_y"].tolist() == [0] + [1] * 9 + [0] * 246
    n = su.record(S, None, 3, 3, 0)
    assert (n["has_prev"], n["sad_y"], n["sse_y"], n["sad_cb"], n["sad_cr"], n["changed_y"]) == (0,) * 6 and n["sum_y2"] == 285
    cs, cd = su.grid(S, P, 3, 3, 8)
    assert cs.tolist() == [[45]] and cd.tolist() == [[15]] and su.grid(S, None, 3, 3, 64)[1].tolist() == [[0]]
    assert su.item_bytes(3, 3) == 1120 and su.item_bytes(3, 3, 8, 3) == 1120 + 16 and su.item_bytes(3, 3, 8, 1) == 1120 + 16
    it = su.item(S, P, 3, 3, 8, 3, 5)
    assert it.size == 1136 and it[1120:].tolist() == [45, 0, 0, 0, 15, 0, 0, 0] + [0] * 8
    assert it[:8].tolist() == [45, 0, 0, 0, 0, 0, 0, 0] and it[64:72].tolist() == [1, 0, 0, 0, 9, 0, 0, 0], "little-endian, sum_y first, min_y at byte 64"
    p = su.parse(it, 3)
    assert {k: p[k] for k in want} == want and (p["gw"], p["gh"]) == (1, 1) and p["cell_sum"].tolist() == [[45]]
    su.check_invariants(p, 3)


def test_known_answers_17x9():
    """S[y][x] = 10 y + x on 17 x 9; chroma 9 x 5: Cb = 100, Cr[y][x] = x.  P = S + 2 in column 16, S - 3 in row 8 left of it; Cb + 1.
    Sums in closed form: sum of y over 0 .. 8 is 36 (squares 204), of x over 0 .. 16 is 136 (squares 1496), over 0 .. 7 is 28, over 8 .. 15 is 92."""
    w, h = 17, 9
    y = np.add.outer(10 * np.arange(h), np.arange(w))
    py = y.copy()
    py[:, 16] += 2
    py[8, :16] -= 3
    cr = np.tile(np.arange(9), (5, 1))
    S, P = _i420(y, np.full((5, 9), 100), cr), _i420(py, np.full((5, 9), 101), cr)
    r = su.record(S, P, w, h, 2)
    want = dict(sum_y=17 * 10 * 36 + 9 * 136, sum_y2=100 * 17 * 204 + 20 * 36 * 136 + 9 * 1496, sum_cb=4500, sum_cr=5 * 36, sad_y=9 * 2 + 16 * 3,
                sse_y=9 * 4 + 16 * 9, sad_cb=45, sad_cr=0, min_y=0, max_y=96, changed_y=16, has_prev=1, w=17, h=9)
    assert want["sum_y"] == 7344 and want["sum_y2"] == 458184 and want["sad_y"] == 66 and want["sse_y"] == 180
    assert {k: r[k] for k in want} == want
    assert su.record(S, P, w, h, 1)["changed_y"] == 25 and su.record(S, P, w, h, 3)["changed_y"] == 0
    hist = r["hist_y"]
    assert (hist[0], hist[10], hist[16], hist[96], hist[97]) == (1, 2, 2, 1, 0) and hist.sum() == 153
    cs, cd = su.grid(S, P, w, h, 8)  # 3 x 2 cells: columns 0 .. 7, 8 .. 15, 16; rows 0 .. 7, 8
    assert cs.tolist() == [[80 * 28 + 8 * 28, 80 * 28 + 8 * 92, 10 * 28 + 8 * 16], [8 * 80 + 28, 8 * 80 + 92, 96]] == [[2464, 2976, 408], [668, 732, 96]]
    assert cd.tolist() == [[0, 0, 16], [24, 24, 2]]
    cs, cd = su.grid(S, P, w, h, 16)  # 2 x 1
    assert cs.tolist() == [[7344 - 504, 504]] and cd.tolist() == [[48, 18]]
    assert su.grid(S, P, w, h, 32)[0].tolist() == [[7344]] and su.grid(S, P, w, h, 64)[1].tolist() == [[66]]
    assert su.item_bytes(w, h, 8, 3) == 1120 + 48 and su.item_bytes(w, h, 8, 2) == 1120 + 32 and su.item_bytes(w, h, 16, 3) == 1120 + 16
    for cell in su.CELLS:
        for planes in (1, 2, 3):
            su.check_invariants(su.parse(su.item(S, P, w, h, cell, planes, 2), planes), planes)
    only_sad = su.parse(su.item(S, P, w, h, 8, 2, 2), 2)
    assert "cell_sum" not in only_sad and only_sad["cell_sad"].tolist() == [[0, 0, 16], [24, 24, 2]], "the selected planes follow the record in ascending bit order"


def test_invariants_on_random_frames():
    rnd = np.random.RandomState(1201)
    for w, h in ((1, 1), (2, 2), (9, 7), (16, 16), (65, 33), (130, 70)):
        n = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
        S, P = rnd.randint(0, 256, n).astype(np.uint8), rnd.randint(0, 256, n).astype(np.uint8)
        for cell, planes in ((0, 0), (8, 3), (16, 1), (32, 2), (64, 3)):
            for prev in (P, None, S):
                r = su.parse(su.item(S, prev, w, h, cell, planes, 31), planes)
                su.check_invariants(r, planes)
                assert (r["gw"], r["gh"]) == su.grid_size(w, h, cell)
                if prev is S:  # P = S: every difference field is 0, and there IS a predecessor
                    assert r["has_prev"] == 1 and all(r[k] == 0 for k in ("sad_y", "sse_y", "sad_cb", "sad_cr", "changed_y"))
                    assert planes & 2 == 0 or not r["cell_sad"].any()
                if prev is P and w * h >= 63:  # (uniform samples: about a quarter of the differences are <= 31)
                    assert r["sse_y"] >= r["sad_y"] > 0 and 0 < r["changed_y"] < w * h
    flat = np.full(16 * 16 * 3 // 2, 200, np.uint8)  # the largest sample values: a flat frame of 200 against one of 0
    r = su.record(flat, np.zeros_like(flat), 16, 16, 199)
    assert (r["sad_y"], r["sse_y"], r["changed_y"], r["min_y"], r["max_y"]) == (256 * 200, 256 * 40000, 256, 200, 200) and r["hist_y"][200] == 256
    assert su.record(flat, np.zeros_like(flat), 16, 16, 200)["changed_y"] == 0, "|S - P| > thresh is strict"


SIZES = (1, 7, 8, 9, 63, 64, 65, 16384)


def _size(L, H, cell, planes, w, h, thresh=0, flags=0):
    gw, gh, n = ctypes.c_int32(-9), ctypes.c_int32(-9), ctypes.c_size_t(12345)
    spec = H._lib.StatsSpec(cell, planes, thresh, flags)
    return L.h264mi_stats_size(ctypes.byref(spec), w, h, ctypes.byref(gw), ctypes.byref(gh), ctypes.byref(n)), (gw.value, gh.value, n.value)


def test_stats_size_equals_the_yardstick(H):
    """h264mi_stats_size -- no decoder, no device -- over every cell size and plane set at the sizes around a cell's edge and the largest."""
    L = H.lib()
    for cell, planes in [(0, 0)] + [(c, p) for c in su.CELLS for p in (1, 2, 3)]:
        for w in SIZES:
            for h in SIZES:
                code, got = _size(L, H, cell, planes, w, h)
                assert code == 0 and got == su.grid_size(w, h, cell) + (su.item_bytes(w, h, cell, planes),), (cell, planes, w, h)
                assert got[2] % 16 == 0 and H.Decoder.stats_size(w, h, cell, planes) == got
    assert _size(L, H, 8, 3, 16384, 16384)[1] == (2048, 2048, 1120 + 2 * 4 * 2048 * 2048)
    assert _size(L, H, 64, 1, 65, 1)[1] == (2, 1, 1120 + 16)
    spec = H._lib.StatsSpec(16, 3, 255, 0)  # any output pointer may be NULL
    n = ctypes.c_size_t(0)
    assert L.h264mi_stats_size(ctypes.byref(spec), 33, 17, None, None, None) == 0
    assert L.h264mi_stats_size(ctypes.byref(spec), 33, 17, None, None, ctypes.byref(n)) == 0 and n.value == 1120 + 2 * 4 * 3 * 2
    assert H.Decoder.stats_size(33, 17, 16, ("cell_sum", "cell_sad")) == (3, 2, 1168) and H.stats_planes(("cell_sad",)) == 2


def test_stats_size_refusals(H):
    L = H.lib()
    bad = [(4, 1), (12, 1), (128, 1), (-8, 1), (1, 1), (0, 1), (0, 3), (8, 0), (64, 0), (16, 4), (16, 7), (16, -1), (0, -1)]  # (cell, planes)
    for cell, planes in bad:
        assert not su.spec_ok(cell, planes) and su.item_bytes(16, 16, cell, planes) is None
        code, got = _size(L, H, cell, planes, 16, 16)
        assert code == EINVAL and got == (-9, -9, 12345), (cell, planes)
    for thresh, flags in ((-1, 0), (256, 0), (0, 1), (0, -1)):
        assert not su.spec_ok(16, 3, thresh, flags)
        assert _size(L, H, 16, 3, 16, 16, thresh, flags) == (EINVAL, (-9, -9, 12345)), (thresh, flags)
    assert _size(L, H, 16, 3, 16, 16, 255)[0] == 0 and _size(L, H, 0, 0, 16, 16, 0)[0] == 0
    for w, h in ((0, 16), (16, 0), (-1, 16), (16385, 16), (16, 16385)):
        assert su.item_bytes(w, h) is None and su.item_bytes(w, h, 8, 3) is None
        assert _size(L, H, 0, 0, w, h) == (EINVAL, (-9, -9, 12345)) and _size(L, H, 8, 3, w, h)[0] == EINVAL, (w, h)
    assert L.h264mi_stats_size(None, 16, 16, None, None, None) == EINVAL
    with pytest.raises(H.H264MIError):
        H.Decoder.stats_size(16, 16, 8, 0)
    with pytest.raises(H.H264MIError):
        H.stats_planes(("cell_max",))


def test_constants_match_the_header(H):
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "h264mi.h")).read()
    for name, value in (("H264MI_STATS_CELL_SUM", su.CELL_SUM), ("H264MI_STATS_CELL_SAD", su.CELL_SAD), ("H264MI_STATS_PREV_NONE", "(%d)" % su.PREV_NONE),
                        ("H264MI_STATS_PREV_HISTORY", "(%d)" % su.PREV_HISTORY), ("H264MI_STATS_HISTORY", 1)):
        assert "#define %s %s" % (name, value) in hdr, name
    assert (H.STATS_CELL_SUM, H.STATS_CELL_SAD, H.STATS_PREV_NONE, H.STATS_PREV_HISTORY, H.STATS_HISTORY) == (1, 2, -1, -2, 1)
    assert (STATS_CELL_SUM, STATS_CELL_SAD, STATS_PREV_NONE, STATS_PREV_HISTORY) == (su.CELL_SUM, su.CELL_SAD, su.PREV_NONE, su.PREV_HISTORY)
    assert ctypes.sizeof(H._lib.FrameStats) == su.RECORD_BYTES == 1120 and H._lib.FrameStats.hist_y.offset == 96 and H._lib.FrameStats.min_y.offset == 64
    assert tuple(n for n, _ in H._lib.FrameStats._fields_) == su.U64 + su.U32 + ("hist_y",) == H.STATS_U64 + H.STATS_U32 + ("hist_y",)
    assert "Frame statistics (K12)" in hdr and hdr.index("Frame statistics (K12)") > hdr.index("Macroblock side information (K11)")
