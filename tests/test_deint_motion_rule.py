"""Motion-adaptive deinterlacing, the rule on the CPU: the yardstick tests/deintmotionutil.py against answers worked out by hand and against its two
identities, and the library's pure entry point h264mi_deint_motion_pixel against the yardstick.  No GPU."""
import ctypes

import numpy as np

import cscutil
import deintmotionutil as dmu
import deintutil as du
import spsutil

EINVAL = -1
FIELD, EDGE = du.FIELD, du.EDGE


def _col(s, p, mode=FIELD, parity=0):
    prev = None if p is None else np.array(p, np.uint8).reshape(-1, 1)
    return dmu.plane(np.array(s, np.uint8).reshape(-1, 1), prev, mode, parity, True).reshape(-1).tolist()


def test_known_answers_of_single_columns():
    """A 1 x 5 column, parity 0: rows 1 and 3 are missing, FIELD gives them (10 + 40 + 1) >> 1 = 25 and (40 + 80 + 1) >> 1 = 60."""
    s = [10, 100, 40, 7, 80]
    assert _col(s, None) == [10, 25, 40, 60, 80] == du.plane(np.array(s, np.uint8).reshape(-1, 1), FIELD, 0, True).reshape(-1).tolist()
    # static: nothing moved, the weave goes out at full vertical resolution
    assert _col(s, s) == s
    # moving: row 1: m = max(190, 200, 100) = 200, [100 - 200, 100 + 200] holds 25; row 3: m = max(200, 80, 248), [7 - 248, 7 + 248] holds 60
    assert _col(s, [200, 0, 240, 255, 0]) == [10, 25, 40, 60, 80]
    # a clamp in each direction: row 1: m = max(|10 - 12|, 0, 0) = 2, 25 is pulled UP to 100 - 2; row 3: m = max(0, |80 - 77|, 0) = 3, 60 DOWN to 7 + 3
    assert _col(s, [12, 100, 40, 7, 77]) == [10, 98, 40, 10, 80]
    # the move of the missing row itself counts: row 1: m = |100 - 60| = 40, 25 -> 60 (row 3 is still: 7); and parity 1: rows 0, 2, 4 are missing, up = dn at both ends
    assert _col(s, [10, 60, 40, 7, 80]) == [10, 60, 40, 7, 80]
    assert _col(s, None, parity=1) == [100, 100, (100 + 7 + 1) >> 1, 7, 7] == [100, 100, 54, 7, 7]
    # m = max(1, 1, 0) = 1: 100 -> 10 + 1 | max(1, 2, 0) = 2: 54 -> 40 + 2 | max(2, 2, 0) = 2: 7 -> 80 - 2
    assert _col(s, [10, 99, 40, 9, 80], parity=1) == [11, 100, 42, 7, 78]
    assert _col([77], [3], parity=1) == [77] and _col([77], [3], EDGE, 0) == [77]  # one row: kept either way
    assert dmu.pixel((10, 100, 40), (12, 100, 40), 25) == 98 and dmu.pixel((40, 7, 80), (40, 7, 77), 60) == 10 and dmu.pixel((1, 2, 3), None, 200) == 200


def test_the_two_identities():
    """No predecessor: mode M's frame, bit for bit.  The frame as its own predecessor: the source frame, bit for bit."""
    rnd = np.random.RandomState(2410)
    for w, h in ((1, 1), (2, 2), (5, 3), (16, 16), (33, 18), (34, 7)):
        f = rnd.randint(0, 256, spsutil.i420_size(w, h)).astype(np.uint8)
        g = rnd.randint(0, 256, spsutil.i420_size(w, h)).astype(np.uint8)
        for mode in (FIELD, EDGE):
            for parity in (0, 1):
                assert np.array_equal(dmu.frame(f, None, w, h, mode, parity), du.frame(f, w, h, mode, parity)), (w, h, mode, parity)
                assert np.array_equal(dmu.frame(f, f, w, h, mode, parity), f), (w, h, mode, parity)
                out, miss = dmu.frame(f, g, w, h, mode, parity), dmu.missing_rows(w, h, parity)
                assert out.shape == f.shape and out.dtype == np.uint8
                assert np.array_equal(out[~miss], f[~miss]), "kept rows are copied"
                sp = du.frame(f, w, h, mode, parity).astype(int)
                lo, hi = np.minimum(sp, f.astype(int)), np.maximum(sp, f.astype(int))
                assert ((out >= lo) & (out <= hi)).all(), "between the spatial value and the weave"
    assert dmu.missing_rows(2, 3, 0).tolist() == [0, 0, 1, 1, 0, 0] + [0, 1] + [0, 1] and dmu.missing_rows(1, 1, 1).tolist() == [0, 0, 0]


def test_motion_pixel_equals_the_yardstick(H):
    """h264mi_deint_motion_pixel -- the rule of one sample as the library states it -- over all rows of a few random columns, both modes and parities."""
    rnd = np.random.RandomState(2411)
    L = H.lib()
    n = 0
    for hp in (1, 2, 5, 8):
        for _ in range(3):
            s = rnd.randint(0, 256, (hp, 3)).astype(np.uint8)
            p = np.clip(s.astype(int) + rnd.randint(-6, 7, (hp, 3)) * (rnd.randint(0, 3, (hp, 3)) == 0), 0, 255).astype(np.uint8)  # mostly still, some moves
            for mode in (FIELD, EDGE):
                for parity in (0, 1):
                    sp, out = du.plane(s, mode, parity, True), dmu.plane(s, p, mode, parity, True)
                    for y in range(hp):
                        kept, up, dn = du.rows(mode, parity, hp, y)
                        for x in range(3):
                            if kept:
                                assert out[y][x] == s[y][x]
                                continue
                            a, b = (s[up][x], s[y][x], s[dn][x]), (p[up][x], p[y][x], p[dn][x])
                            assert H.deint_motion_pixel(a, b, sp[y][x]) == dmu.pixel(a, b, sp[y][x]) == out[y][x], (hp, mode, parity, y, x)
                            assert H.deint_motion_pixel(a, None, sp[y][x]) == sp[y][x]
                            n += 1
    assert n == 270  # missing rows of 1, 2, 5 and 8 rows under both parities: 0 + 2 + 5 + 8, x 2 modes x 3 columns x 3 draws
    # the ends of the range, and the refused calls
    assert H.deint_motion_pixel((0, 255, 0), (255, 0, 255), 0) == 0 and H.deint_motion_pixel((0, 255, 0), (0, 255, 0), 0) == 255
    assert H.deint_motion_pixel((255, 0, 255), (255, 1, 255), 255) == 1
    a3 = ctypes.c_uint8 * 3
    out = ctypes.c_int32(-9)
    assert L.h264mi_deint_motion_pixel(None, a3(1, 2, 3), 5, ctypes.byref(out)) == EINVAL
    assert L.h264mi_deint_motion_pixel(a3(1, 2, 3), a3(1, 2, 3), 5, None) == EINVAL
    for sp in (-1, 256):
        assert L.h264mi_deint_motion_pixel(a3(1, 2, 3), a3(1, 2, 3), sp, ctypes.byref(out)) == EINVAL
    assert out.value == -9
    assert (H.DEINT_PREV_NONE, H.DEINT_PREV_HISTORY, H.DEINT_HISTORY) == (dmu.PREV_NONE, dmu.PREV_HISTORY, dmu.HISTORY) == (-1, -2, 1)
    assert cscutil.planes(np.zeros(spsutil.i420_size(3, 3), np.uint8), 3, 3)[1].shape == (2, 2)  # (the plane sizes the yardstick relies on)
