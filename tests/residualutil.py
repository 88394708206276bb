"""Residual decoding (8.5) written once more, in numpy on int64, straight from the clauses: the yardstick of tests/test_residual_cells.py.

Independent of streamgen/sg_recon.c, oracle/h264o_recon.c, k_residual.h, mi_tables.h and the entropy kernels: no code and no table of theirs.  The zig-zag
scans are generated from their rule (anti-diagonals, alternating direction), the field scans and Table 8-15 are typed from the standard's description.  The
input is the generator's residual trace (streamgen.last_residual_trace()): the prediction sample of every sample, and per macroblock its kind, flags, QP_Y
and the levels as the entropy writer wrote them, in scan order; per picture the two chroma offsets and the eight scaling lists as sent.  The output is the
picture before deblocking, a class word per block, and a CELL for every decision 8.5 took on the way.

What the clauses say, as this file reads them (the project has no copy of the standard):
- 8.5.6 / 8.5.7: a list of levels is mapped to positions by the inverse zig-zag scan in frame macroblocks and by the inverse field scan in field
  macroblocks (every macroblock of a field picture).  A SCALING LIST is mapped by the inverse zig-zag scan always, also in a field picture: the clause
  names the field scan for transform coefficient levels only.
- 8.5.8: qPI = Clip3(0, 51, QP_Y + chroma_qp_index_offset) for Cb, with second_chroma_qp_index_offset for Cr; QPc by Table 8-15 (qPI below 30: itself).
- 8.5.9: LevelScale(m, i, j) = weightScale(i, j) * normAdjust(m, i, j); the list is Intra-Y / Cb / Cr or Inter-Y / Cb / Cr, and Intra-Y / Inter-Y 8x8.
- 8.5.10: Intra16x16 DC: f = A c A, dcY = (f * LevelScale(QP % 6, 0, 0)) << (QP / 6 - 6) from QP 36 on, (f * LS + 2^(5 - QP / 6)) >> (6 - QP / 6) below.
- 8.5.11: chroma DC: f = [[1, 1], [1, -1]] c [[1, 1], [1, -1]], dcC = ((f * LevelScale(QPc % 6, 0, 0)) << (QPc / 6)) >> 5: no rounding term.
- 8.5.12: d = (c * LS) << (qP / 6 - 4) from qP 24 on, (c * LS + 2^(3 - qP / 6)) >> (4 - qP / 6) below; d00 is the DC value where one was derived
  separately; rows first, then columns, with (x >> 1); r = (x + 32) >> 6.  8.5.13: the same with 6 for 4, 36 for 24, the 8-point butterflies with (x >> 1)
  and (x >> 2).  ">>" is arithmetic: it rounds towards minus infinity.
- 8.5.14: u = Clip1(pred + r).  A block without coded levels has r = 0; I_PCM samples are the picture; a monochrome picture has chroma planes of 128.

A cell names one decision; reachable_cells() enumerates them from the rules above, not from what the recipes happen to reach.

group4: k_inter.hip puts the macroblocks 4 g .. 4 g + 3 of a PICTURE (consecutive addresses, aligned to four, lanes beyond the picture idle) into one
wavefront and takes its DC-only chroma path when no inter macroblock of the four has chroma class 2.  The group is therefore the aligned run of four
consecutive addresses; "others" are the macroblocks of the run that are not inter macroblocks with chroma residual.  The run at the end of a picture that
is shorter than four is counted by its length ("short", 1 .. 3) instead."""
from collections import Counter

import numpy as np

RS_SKIPPED, RS_INTER, RS_I4, RS_I8, RS_I16, RS_PCM = range(6)   # the trace's macroblock kinds


# ---- 8.5.6 / 8.5.7: the scans, as (x, y) per scan index ----
def _zigzag(n):
    """anti-diagonals x + y = s from the upper left corner; odd ones run down to the left, even ones up to the right"""
    out = []
    for s in range(2 * n - 1):
        cells = [(x, s - x) for x in range(n) if 0 <= s - x < n]
        out += cells[::-1] if s & 1 else cells
    return out


def _pairs(text):
    return [(int(t[0]), int(t[1])) for t in text.split()]


# Table 8-12, field scan: the first column down, then (1,0); the rest of column 1; columns 2 and 3 down
_FIELD4 = _pairs("00 01 10 02 03 11 12 13 20 21 22 23 30 31 32 33")
# Table 8-13, field scan, as xy
_FIELD8 = _pairs("00 01 02 10 11 03 04 12 20 13 05 06 07 14 21 30 22 15 16 17 23 31 40 32 24 25 26 27 33 41 50 42 "
                 "34 35 36 37 43 51 60 52 44 45 46 47 53 61 62 54 55 56 57 63 70 71 64 65 66 67 72 73 74 75 76 77")
_ZIGZAG4, _ZIGZAG8 = _zigzag(4), _zigzag(8)
assert sorted(_FIELD4) == sorted(_ZIGZAG4) and sorted(_FIELD8) == sorted(_ZIGZAG8) and _ZIGZAG4[:6] == [(0, 0), (1, 0), (0, 1), (0, 2), (1, 1), (2, 0)]


def _scan_for(n, field):
    """the scan of transform coefficient LEVELS of a block of n x n in a frame (0) or field (1) macroblock"""
    return (_FIELD4 if field else _ZIGZAG4) if n == 4 else (_FIELD8 if field else _ZIGZAG8)


def _inverse_scan(values, n, scan, first=0):
    """values[k] goes to the position of scan index first + k; the result is indexed [row][column]"""
    c = np.zeros((n, n), dtype=np.int64)
    for k, v in enumerate(values):
        if v:
            x, y = scan[first + k]
            c[y, x] = v
    return c


# ---- 8.5.8: Table 8-15 ----
_QPC_FROM_30 = (29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39)


def _clip3(lo, hi, v):
    return lo if v < lo else (hi if v > hi else v)


def _qpc(plane, qp_y, offsets):
    """QPc of plane 1 (Cb) / 2 (Cr): (QPc, qPI, the sum before the clip)"""
    raw = qp_y + offsets[plane - 1]
    qpi = _clip3(0, 51, raw)
    return (qpi if qpi < 30 else _QPC_FROM_30[qpi - 30]), qpi, raw


# ---- 8.5.9 ----
_NORM4 = ((10, 16, 13), (11, 18, 14), (13, 20, 16), (14, 23, 18), (16, 25, 20), (18, 29, 23))
_NORM8 = ((20, 18, 32, 19, 25, 24), (22, 19, 35, 21, 28, 26), (26, 23, 42, 24, 33, 31), (28, 25, 45, 26, 35, 33), (32, 28, 51, 30, 40, 38), (36, 32, 58, 34, 46, 43))
_ls_cache = {}


def _level_scale(lst, m):
    """LevelScale4x4 / 8x8 (m, i, j) as an array [row][column] from a scaling list in the order of its syntax elements"""
    key = (bytes(bytearray(int(v) for v in lst)), m)
    if key not in _ls_cache:
        n = 4 if len(lst) == 16 else 8
        weight = _inverse_scan([int(v) for v in lst], n, _ZIGZAG4 if n == 4 else _ZIGZAG8)   # a scaling list: zig-zag always
        norm = np.zeros((n, n), dtype=np.int64)
        for i in range(n):
            for j in range(n):
                if n == 4:
                    k = 0 if i % 2 == 0 and j % 2 == 0 else (1 if i % 2 == 1 and j % 2 == 1 else 2)
                    norm[i, j] = _NORM4[m][k]
                else:
                    if i % 4 == 0 and j % 4 == 0:
                        k = 0
                    elif i % 2 == 1 and j % 2 == 1:
                        k = 1
                    elif i % 4 == 2 and j % 4 == 2:
                        k = 2
                    elif (i % 4 == 0 and j % 2 == 1) or (i % 2 == 1 and j % 4 == 0):
                        k = 3
                    elif (i % 4 == 0 and j % 4 == 2) or (i % 4 == 2 and j % 4 == 0):
                        k = 4
                    else:
                        k = 5
                    norm[i, j] = _NORM8[m][k]
        _ls_cache[key] = weight * norm
    return _ls_cache[key]


# ---- the arithmetic the wrong-rule test patches ----
def _round_term(shift):
    return 1 << (shift - 1)


def _shr(x, n):
    return x >> n


_PIVOT_4x4, _PIVOT_8x8, _PIVOT_DC16 = 4, 6, 6     # qP / 6 from which the scaling shifts left


class _Rec:
    """what one picture's reconstruction counted"""

    def __init__(self):
        self.cells = Counter()
        self.max_d = {}

    def hit(self, *cell):
        self.cells[cell] += 1


def _scale(prod, per, pivot, rec, cls):
    """the two branches of 8.5.10, 8.5.12.1 and 8.5.13 on the products c * LevelScale"""
    if per >= pivot:
        d = prod << (per - pivot)
    else:
        if (prod < 0).any():
            rec.hit("round", cls, "neg")
        if (prod > 0).any():
            rec.hit("round", cls, "pos")
        d = (prod + _round_term(pivot - per)) >> (pivot - per)
    return d


def _note_d(rec, cls, d):
    m = int(np.abs(d).max())
    if m > rec.max_d.get(cls, 0):
        rec.max_d[cls] = m
    if m >= T[cls]:
        rec.hit("value", "big", cls)


def _half(x, n, rec, tag):
    if ((x < 0) & ((x & ((1 << n) - 1)) != 0)).any():
        rec.hit("value", "odd_neg", tag, n)
    return _shr(x, n)


def _final(h, rec, tag):
    if ((h < 0) & ((h & 63) == 32)).any():
        rec.hit("value", "tie_neg", tag)
    return (h + 32) >> 6


def _transform4(d, rec):
    """8.5.12.2: d[row][column]"""
    d0, d1, d2, d3 = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    e0, e1, e2, e3 = d0 + d2, d0 - d2, _half(d1, 1, rec, "4x4") - d3, d1 + _half(d3, 1, rec, "4x4")
    f = np.stack([e0 + e3, e1 + e2, e1 - e2, e0 - e3], axis=1)
    if int(np.abs(f).max()) >= 1 << 15:
        rec.hit("value", "rowpass15")
    f0, f1, f2, f3 = f[0], f[1], f[2], f[3]
    g0, g1, g2, g3 = f0 + f2, f0 - f2, _half(f1, 1, rec, "4x4") - f3, f1 + _half(f3, 1, rec, "4x4")
    return _final(np.stack([g0 + g3, g1 + g2, g1 - g2, g0 - g3], axis=0), rec, "4x4")


def _butterfly8(d, rec):
    """the 8-point transform of 8.5.13 on d[0] .. d[7] (arrays)"""
    a0, a2 = d[0] + d[4], d[0] - d[4]
    a4, a6 = _half(d[2], 1, rec, "8x8") - d[6], d[2] + _half(d[6], 1, rec, "8x8")
    a1 = -d[3] + d[5] - d[7] - _half(d[7], 1, rec, "8x8")
    a3 = d[1] + d[7] - d[3] - _half(d[3], 1, rec, "8x8")
    a5 = -d[1] + d[7] + d[5] + _half(d[5], 1, rec, "8x8")
    a7 = d[3] + d[5] + d[1] + _half(d[1], 1, rec, "8x8")
    b0, b2, b4, b6 = a0 + a6, a2 + a4, a2 - a4, a0 - a6
    b1, b3 = a1 + _half(a7, 2, rec, "8x8"), a3 + _half(a5, 2, rec, "8x8")
    b5, b7 = _half(a3, 2, rec, "8x8") - a5, a7 - _half(a1, 2, rec, "8x8")
    return [b0 + b7, b2 + b5, b4 + b3, b6 + b1, b6 - b1, b4 - b3, b2 - b5, b0 - b7]


def _transform8(d, rec):
    g = np.stack(_butterfly8([d[:, k] for k in range(8)], rec), axis=1)
    if int(np.abs(g).max()) >= 1 << 15:
        rec.hit("value", "rowpass15")
    m = np.stack(_butterfly8([g[k] for k in range(8)], rec), axis=0)
    return _final(m, rec, "8x8")


_A4 = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], dtype=np.int64)
_A2 = np.array([[1, 1], [1, -1]], dtype=np.int64)

# the largest power of two that the generator alone reaches with a dequantised coefficient of each class under its range guard (the measured maxima stand
# in tests/golden/residual_counters.txt; test_recipes_together_reach_every_cell asserts T <= maximum < 2 T)
T = {"luma4": 1 << 14, "dc16": 1 << 14, "luma8": 1 << 14, "cdc": 1 << 14, "cac": 1 << 14}

# class word of a block: bits 0-2 class, 3 intra prediction, 4 a coded level, 5-10 qP, 11 field, 12-13 plane, 14 coded matrix
CLASSES = ("luma4", "i16", "luma8", "cdc", "cac", "none", "pcm")


def class_word(cls, intra, coded, qp, field, plane, matrix):
    return CLASSES.index(cls) | intra << 3 | coded << 4 | qp << 5 | field << 11 | plane << 12 | matrix << 14


def describe(word):
    return dict(cls=CLASSES[word & 7], intra=word >> 3 & 1, coded=word >> 4 & 1, qp=word >> 5 & 63, field=word >> 11 & 1, plane=word >> 12 & 3, coded_matrix=word >> 14 & 1)


def _blk4_xy(idx):
    """6.4.3: upper left luma sample of luma4x4BlkIdx"""
    return (idx >> 2 & 1) * 8 + (idx & 1) * 4, (idx >> 3) * 8 + (idx >> 1 & 1) * 4


class Picture:
    pass


def reconstruct_picture(t):
    """8.5 on one entry of streamgen.last_residual_trace().  Returns a Picture: planes (Y, Cb, Cr as uint8, before deblocking), words {(macroblock
    address, plane, block): class word} (luma blocks by luma4x4BlkIdx, or luma8x8BlkIdx * 4 with the 8x8 transform; chroma by chroma4x4BlkIdx), qpc
    [rows, columns, 2], qp [rows, columns], nz [4 rows, 4 columns per macroblock: a 4x4 luma block with a level; with the 8x8 transform its 8x8 block],
    cells (a Counter) and max_d (per class the largest dequantised magnitude)."""
    rec = _Rec()
    field, mono = int(t["field"] != 0), int(t["mono"])
    fname = "field" if field else "frame"
    mbs = t["rsmbs"]
    hmb, wmb = mbs.shape
    res = [np.zeros(p.shape, dtype=np.int64) for p in t["pred"]]
    out = [p.astype(np.int64) for p in t["pred"]]
    offsets = (t["chroma_qp_index_offset"], t["second_chroma_qp_index_offset"])
    lists4, lists8 = t["lists4"], t["lists8"]
    coded_list = [bool((lists4[i] != 16).any()) for i in range(6)] + [bool((lists8[i] != 16).any()) for i in range(2)]
    words, qpc_plane, nz = {}, np.zeros((hmb, wmb, 2), dtype=np.int64), np.zeros((hmb * 4, wmb * 4), dtype=np.uint8)
    s4, s8 = _scan_for(4, field), _scan_for(8, field)
    group = []   # per macroblock address: 2 / 1 = an inter macroblock with that chroma class, 0 = another

    def block_cells(cls, qp, lname, lidx, intra):
        rec.hit("scale", cls, qp)
        rec.hit("matrix", "coded" if coded_list[lidx] else "flat", "intra" if intra else "inter", lname, fname)

    def scan_cells(kind, values, first=0):
        for k, v in enumerate(values):
            if v:
                rec.hit("scan", fname, kind, first + k)

    for my in range(hmb):
        for mx in range(wmb):
            mb, addr = mbs[my, mx], my * wmb + mx
            kind, qp, cbp, t8 = int(mb["kind"]), int(mb["qp"]), int(mb["cbp"]), int(mb["t8x8"])
            intra = int(kind >= RS_I4)
            luma, chroma_class = cbp & 15, cbp >> 4
            x0, y0 = mx * 16, my * 16
            for c in (1, 2):
                qpc_plane[my, mx, c - 1] = _qpc(c, 0 if kind == RS_PCM else qp, offsets)[0]
            group.append(chroma_class if kind == RS_INTER else 0)
            if kind == RS_PCM:
                pcm = mb["pcm"].astype(np.int64)
                out[0][y0:y0 + 16, x0:x0 + 16] = pcm[:256].reshape(16, 16)
                for v in (0, 255):
                    if (pcm[:256 if mono else 384] == v).any():
                        rec.hit("value", "pcm", v)
                if not mono:
                    out[1][y0 // 2:y0 // 2 + 8, x0 // 2:x0 // 2 + 8] = pcm[256:320].reshape(8, 8)
                    out[2][y0 // 2:y0 // 2 + 8, x0 // 2:x0 // 2 + 8] = pcm[320:].reshape(8, 8)
                nz[my * 4:my * 4 + 4, mx * 4:mx * 4 + 4] = 1
                for b in range(16):
                    words[(addr, 0, b)] = class_word("pcm", 1, 1, 0, field, 0, 0)
                continue
            if kind == RS_SKIPPED or (cbp == 0 and kind != RS_I16):
                if qp != int(mb["slice_qp"]):
                    rec.hit("value", "carried_qp", "skipped" if kind == RS_SKIPPED else "cbp0")
            if kind != RS_SKIPPED:
                rec.hit("cbp", "i16" if kind == RS_I16 else ("intra" if intra else "inter"), luma, chroma_class)
            # ---- luma ----
            per, rem = qp // 6, qp % 6
            if kind == RS_I16:
                ls = _level_scale(lists4[0], rem)
                dc_levels = [int(v) for v in mb["dc16"]]
                dcy = np.zeros((4, 4), dtype=np.int64)
                if any(dc_levels):
                    scan_cells("dc16", dc_levels)
                    block_cells("dc16", qp, "y4", 0, 1)
                    f = _A4 @ _inverse_scan(dc_levels, 4, s4) @ _A4
                    dcy = _scale(f * ls[0, 0], per, _PIVOT_DC16, rec, "dc16")
                    _note_d(rec, "dc16", dcy)
                for idx in range(16):
                    bx, by = _blk4_xy(idx)
                    ac = [int(v) for v in mb["luma"][idx][1:]]
                    assert mb["luma"][idx][0] == 0 and (luma or not any(ac)), "the trace's levels contradict its coded_block_pattern"
                    d = np.zeros((4, 4), dtype=np.int64)
                    if any(ac):
                        scan_cells("luma4", ac, 1)
                        block_cells("luma4", qp, "y4", 0, 1)
                        d = _scale(_inverse_scan(ac, 4, s4, 1) * ls, per, _PIVOT_4x4, rec, "luma4")
                        _note_d(rec, "luma4", d)
                        nz[my * 4 + by // 4, mx * 4 + bx // 4] = 1
                    d[0, 0] = dcy[by // 4, bx // 4]
                    coded = int(d.any())
                    if coded:
                        res[0][y0 + by:y0 + by + 4, x0 + bx:x0 + bx + 4] = _transform4(d, rec)
                    words[(addr, 0, idx)] = class_word("i16", 1, coded, qp, field, 0, int(coded_list[0]))
            elif t8:
                lidx = 6 if intra else 7
                ls = _level_scale(lists8[lidx - 6], rem)
                lev8 = mb["luma"].reshape(4, 64)
                for b8 in range(4):
                    lev = [int(v) for v in lev8[b8]]
                    bx, by = (b8 & 1) * 8, (b8 >> 1) * 8
                    assert (luma >> b8 & 1) or not any(lev), "the trace's levels contradict its coded_block_pattern"
                    coded, rows = int(any(lev)), 0
                    if coded:
                        scan_cells("luma8", lev)
                        block_cells("luma8", qp, "y8", lidx, intra)
                        c = _inverse_scan(lev, 8, s8)
                        rows = sum(1 << k for k in range(4) if c[2 * k:2 * k + 2].any())
                        d = _scale(c * ls, per, _PIVOT_8x8, rec, "luma8")
                        _note_d(rec, "luma8", d)
                        res[0][y0 + by:y0 + by + 8, x0 + bx:x0 + bx + 8] = _transform8(d, rec)
                        nz[my * 4 + by // 4:my * 4 + by // 4 + 2, mx * 4 + bx // 4:mx * 4 + bx // 4 + 2] = 1
                    rec.hit("rows8", "intra" if intra else "inter", rows)
                    words[(addr, 0, b8 * 4)] = class_word("luma8", intra, coded, qp, field, 0, int(coded_list[lidx]))
            else:
                lidx = 0 if intra else 3
                ls = _level_scale(lists4[lidx], rem)
                for idx in range(16):
                    lev = [int(v) for v in mb["luma"][idx]]
                    bx, by = _blk4_xy(idx)
                    assert (luma >> (idx >> 2) & 1) or not any(lev), "the trace's levels contradict its coded_block_pattern"
                    coded = int(any(lev))
                    if coded:
                        scan_cells("luma4", lev)
                        block_cells("luma4", qp, "y4", lidx, intra)
                        d = _scale(_inverse_scan(lev, 4, s4) * ls, per, _PIVOT_4x4, rec, "luma4")
                        _note_d(rec, "luma4", d)
                        res[0][y0 + by:y0 + by + 4, x0 + bx:x0 + bx + 4] = _transform4(d, rec)
                        nz[my * 4 + by // 4, mx * 4 + bx // 4] = 1
                    words[(addr, 0, idx)] = class_word("luma4" if kind != RS_SKIPPED else "none", intra, coded, qp, field, 0, int(coded_list[lidx]))
            # ---- chroma ----
            if mono:
                continue
            dc_planes, ac_planes = 0, 0
            for c in (1, 2):
                qc, qpi, raw = _qpc(c, qp, offsets)
                pname, lidx = ("cb", "cr")[c - 1], (0 if intra else 3) + c
                cdc = [int(v) for v in mb["cdc"][c - 1]]
                cac = [[int(v) for v in mb["cac"][c - 1][b]] for b in range(4)]
                assert (chroma_class or not any(cdc)) and (chroma_class == 2 or not any(any(a) for a in cac)), "the trace's levels contradict its coded_block_pattern"
                if chroma_class:
                    rec.hit("qpc", pname, qpi)
                    if raw < 0:
                        rec.hit("qpc", pname, "clip0")
                    if raw > 51:
                        rec.hit("qpc", pname, "clip51")
                ls = _level_scale(lists4[lidx], qc % 6)
                dcc = np.zeros((2, 2), dtype=np.int64)
                if any(cdc):
                    dc_planes |= c
                    for k, v in enumerate(cdc):
                        if v:
                            rec.hit("scan", pname, "cdc", k)
                    block_cells("cdc", qc, pname + "4", lidx, intra)
                    f = _A2 @ np.array(cdc, dtype=np.int64).reshape(2, 2) @ _A2
                    dcc = ((f * ls[0, 0]) << (qc // 6)) >> 5
                    _note_d(rec, "cdc", dcc)
                if any(any(a) for a in cac):
                    ac_planes |= c
                elif chroma_class == 2 and any(cdc):
                    rec.hit("chroma", "ac_empty_dc_not")
                for b in range(4):
                    bx, by = (b & 1) * 4, (b >> 1) * 4
                    d = np.zeros((4, 4), dtype=np.int64)
                    if any(cac[b]):
                        scan_cells("cac", cac[b], 1)
                        block_cells("cac", qc, pname + "4", lidx, intra)
                        d = _scale(_inverse_scan(cac[b], 4, s4, 1) * ls, qc // 6, _PIVOT_4x4, rec, "cac")
                        _note_d(rec, "cac", d)
                    d[0, 0] = dcc[b >> 1, b & 1]
                    coded = int(d.any())
                    if coded:
                        res[c][y0 // 2 + by:y0 // 2 + by + 4, x0 // 2 + bx:x0 // 2 + bx + 4] = _transform4(d, rec)
                    words[(addr, c, b)] = class_word("cac" if chroma_class == 2 else ("cdc" if chroma_class == 1 else "none"), intra, coded, qc, field, c, int(coded_list[lidx]))
            if chroma_class == 1:
                rec.hit("chroma", "dc", ("none", "cb", "cr", "both")[dc_planes])
            if chroma_class == 2:
                rec.hit("chroma", "ac", ("none", "cb", "cr", "both")[ac_planes])
    # ---- 8.5.14, and the clips per class ----
    planes = []
    for c in range(3):
        u = out[c] + res[c]
        planes.append(np.clip(u, 0, 255).astype(np.uint8))
        out[c] = u
    if mono:
        planes[1][:], planes[2][:] = 128, 128
    for (addr, c, b), w in words.items():
        d = describe(w)
        if not d["coded"] or d["cls"] in ("pcm", "none"):
            continue
        mx, my = addr % wmb, addr // wmb
        if c == 0:
            n = 8 if d["cls"] == "luma8" else 4
            bx, by = ((b >> 2 & 1) * 8, (b >> 3) * 8) if n == 8 else _blk4_xy(b)
            u = out[0][my * 16 + by:my * 16 + by + n, mx * 16 + bx:mx * 16 + bx + n]
        else:
            u = out[c][my * 8 + (b >> 1) * 4:my * 8 + (b >> 1) * 4 + 4, mx * 8 + (b & 1) * 4:mx * 8 + (b & 1) * 4 + 4]
        if (u < 0).any():
            rec.hit("value", "clip0", d["cls"], "intra" if d["intra"] else "inter")
        if (u > 255).any():
            rec.hit("value", "clip255", d["cls"], "intra" if d["intra"] else "inter")
    for g in range(0, len(group), 4):
        run = group[g:g + 4]
        if len(run) < 4:
            rec.hit("group4", "short", len(run))
        else:
            n2, n1 = run.count(2), run.count(1)
            rec.hit("group4", min(n2, 2), min(n1, 2), min(4 - n2 - n1, 1))
    p = Picture()
    p.planes, p.words, p.qpc, p.qp, p.nz, p.cells, p.max_d = planes, words, qpc_plane, mbs["qp"].astype(np.int64), nz, rec.cells, rec.max_d
    p.wmb, p.hmb, p.field, p.frame = wmb, hmb, t["field"], t["frame"]
    return p


def reconstruct_stream(trace):
    return [reconstruct_picture(t) for t in trace]


def first_difference(pic, planes):
    """None, or where the yardstick's picture first differs from `planes` (Y, Cb, Cr): (macroblock address, plane, block, the block's class word described,
    the yardstick's sample, the other one)"""
    for c in range(3):
        bad = np.argwhere(pic.planes[c] != planes[c])
        if len(bad):
            y, x = (int(v) for v in bad[0])
            n = 16 if c == 0 else 8
            addr, ix, iy = (y // n) * pic.wmb + x // n, x % n, y % n
            if c == 0:
                b = next((k for k in range(16) if (addr, 0, k) in pic.words and _blk4_xy(k)[0] <= ix < _blk4_xy(k)[0] + (8 if describe(pic.words[(addr, 0, k)])["cls"] == "luma8" else 4)
                          and _blk4_xy(k)[1] <= iy < _blk4_xy(k)[1] + (8 if describe(pic.words[(addr, 0, k)])["cls"] == "luma8" else 4)), 0)
            else:
                b = (iy // 4) * 2 + ix // 4
            w = pic.words.get((addr, c, b))
            return addr, c, b, describe(w) if w is not None else None, int(pic.planes[c][y, x]), int(planes[c][y, x])
    return None


def macroblock_words(pic, addr):
    """the class words of a macroblock's blocks, described: what a GPU test reports beside the first wrong macroblock"""
    return {(c, b): describe(w) for (a, c, b), w in sorted(pic.words.items()) if a == addr}


# ---- the cells ----
SCALE_CLASSES = {"luma4": 52, "dc16": 52, "luma8": 52, "cdc": 40, "cac": 40}
ROUND_CLASSES = {"luma4": 24, "dc16": 36, "luma8": 36, "cac": 24}      # class -> the qP from which there is no rounding term (cdc has none at all)
BLOCK_CLASSES = (("luma4", "intra"), ("luma4", "inter"), ("i16", "intra"), ("luma8", "intra"), ("luma8", "inter"), ("cdc", "intra"), ("cdc", "inter"),
                 ("cac", "intra"), ("cac", "inter"))
_reach = None


def reachable_cells():
    global _reach
    if _reach is not None:
        return _reach
    r = set()
    for plane in ("cb", "cr"):
        r |= {("qpc", plane, q) for q in range(52)} | {("qpc", plane, "clip0"), ("qpc", plane, "clip51")}
    for cls, n in SCALE_CLASSES.items():
        r |= {("scale", cls, q) for q in range(n)}
    r |= {("round", cls, s) for cls in ROUND_CLASSES for s in ("neg", "pos")}
    for f in ("frame", "field"):
        r |= {("scan", f, "luma4", k) for k in range(16)} | {("scan", f, "luma8", k) for k in range(64)} | {("scan", f, "dc16", k) for k in range(16)}
        r |= {("scan", f, "cac", k) for k in range(1, 16)}
    r |= {("scan", plane, "cdc", k) for plane in ("cb", "cr") for k in range(4)}
    r |= {("matrix", m, i, l, f) for m in ("flat", "coded") for i in ("intra", "inter") for l in ("y4", "cb4", "cr4", "y8") for f in ("frame", "field")}
    r |= {("cbp", i, luma, c) for i in ("intra", "inter") for luma in range(16) for c in range(3)} | {("cbp", "i16", luma, c) for luma in (0, 15) for c in range(3)}
    r |= {("rows8", i, s) for i in ("intra", "inter") for s in range(16)}
    r |= {("chroma", "dc", p) for p in ("cb", "cr", "both")} | {("chroma", "ac", p) for p in ("cb", "cr", "both")} | {("chroma", "ac_empty_dc_not")}
    r |= {("group4", a, b, c) for a in range(3) for b in range(3) for c in range(2) if _group_sums_to_four(a, b, c)} | {("group4", "short", n) for n in (1, 2, 3)}
    for cls, pred in BLOCK_CLASSES:
        r |= {("value", "clip0", cls, pred), ("value", "clip255", cls, pred)}
    r |= {("value", "tie_neg", "4x4"), ("value", "tie_neg", "8x8"), ("value", "odd_neg", "4x4", 1), ("value", "odd_neg", "8x8", 1), ("value", "odd_neg", "8x8", 2)}
    r |= {("value", "big", cls) for cls in SCALE_CLASSES} | {("value", "rowpass15"), ("value", "pcm", 0), ("value", "pcm", 255)}
    r |= {("value", "carried_qp", "skipped"), ("value", "carried_qp", "cbp0")}
    _reach = r
    return r


def _group_sums_to_four(a, b, c):
    """counts a, b in {0, 1, 2 = two or more} and c in {0, 1 = one or more}: can they be the counts of four macroblocks?"""
    lo = a + b + c
    hi = (4 if a == 2 else a) + (4 if b == 2 else b) + (4 if c == 1 else 0)
    return lo <= 4 <= hi


FAMILIES = ("qpc", "scale", "round", "scan", "matrix", "cbp", "rows8", "chroma", "group4", "value")
NO_EXEMPTION = ("qpc", "scale", "round", "scan", "matrix")
# reachable cells that no recipe reaches, each by name with its reason.  At most one in twenty of a family, none in the families of NO_EXEMPTION.
EXEMPT = {
    ("value", "rowpass15"): "the generator's range guard keeps every intermediate of both transforms within +-32700: no stream of its making holds one",
}


def beyond_reach(cells):
    return sorted((c for c in cells if c not in reachable_cells()), key=repr)


def cell_line(name, cells):
    """a recipe's cells as one line of tests/golden/residual_counters.txt: per family the number of distinct cells and of decisions counted"""
    per = {}
    for c, n in cells.items():
        d = per.setdefault(c[0], [0, 0])
        d[0] += 1
        d[1] += n
    return "  %-28s %s" % (name, " ".join("%s=%d/%d" % (f, per[f][0], per[f][1]) for f in FAMILIES if f in per))


def max_line(max_d):
    return "  T: " + " ".join("%s=%d(max %d)" % (c, T[c], max_d.get(c, 0)) for c in sorted(T))


# ---- recipes of tests/test_residual_cells.py ----
# Pictures of 48x32 .. 96x80; frame recipes have at most 8 frames, field recipes at most 5; four geometries of 3 frames.  The seeds were chosen on the CPU
# until the generator alone reached every cell but the exempt ones.
_R = dict(trace_residual=1, residual_stim=1)
_P = dict(_R, idr_period=0, skip_permille=100, sub8x8_permille=300, intra_in_p_permille=80)
I_RECIPES = {
    "i_cavlc_base": dict(_R, width=64, height=48, frames=6, idr_period=1, profile_idc=66, cabac=0, seed=1),
    "i_cabac_high8_cqo_m12_pcm": dict(_R, width=80, height=64, frames=6, idr_period=1, profile_idc=100, cabac=1, transform8x8=1, chroma_qp_offset=-12, pcm_permille=40,
                                      deblock_idc=1, seed=2),
    "i_cavlc_high8_sm2_syntax": dict(_R, width=64, height=48, frames=6, idr_period=1, profile_idc=100, cabac=0, transform8x8=1, scaling_matrix=2, chroma_qp_offset=12,
                                     syntax_stim=1, seed=3),
}
P_RECIPES = {
    "p_cabac_contrast_qp4_pcm": dict(trace_residual=1, width=64, height=48, frames=4, idr_period=2, profile_idc=77, cabac=1, contrast=1, qp=4, pcm_permille=100, noise=0,
                                     motion_x4=5, motion_y4=-3, seed=4),
    "p_cabac_main_intra": dict(_P, width=96, height=80, frames=8, profile_idc=77, cabac=1, num_ref_frames=2, intra_in_p_permille=300, deblock_idc=1, seed=5),
    "p_cavlc_base_skip_3slices": dict(_P, width=80, height=64, frames=8, profile_idc=66, cabac=0, skip_permille=400, slices=3, chroma_qp_offset=12, seed=6),
    "p_cabac_high8_sm3_syntax": dict(_P, width=64, height=48, frames=8, idr_period=2, profile_idc=100, cabac=1, transform8x8=1, scaling_matrix=3, num_ref_frames=2,
                                     chroma_qp_offset=-12, syntax_stim=1, seed=7),
    "p_cavlc_high8": dict(_P, width=80, height=64, frames=8, profile_idc=100, cabac=0, transform8x8=1, num_ref_frames=2, seed=8),
    "p_cabac_contrast_qp51": dict(trace_residual=1, idr_period=0, width=64, height=48, frames=5, profile_idc=77, cabac=1, contrast=1, qp=51, motion_x4=3, motion_y4=-5,
                                  sub8x8_permille=300, seed=9),
    "p_cabac_main_syntax_cqo_p12": dict(_P, width=80, height=64, frames=8, profile_idc=77, cabac=1, chroma_qp_offset=12, syntax_stim=1, seed=26),
}
B_RECIPES = {
    "b_cabac_high8_sm2": dict(_P, width=80, height=64, frames=7, profile_idc=100, cabac=1, transform8x8=1, scaling_matrix=2, bframes=2, num_ref_frames=3,
                              bskip_permille=120, deblock_idc=1, seed=11),
    "b_cavlc_main": dict(_P, width=64, height=64, frames=7, profile_idc=77, cabac=0, bframes=1, num_ref_frames=2, bskip_permille=150, chroma_qp_offset=-12, seed=4),
}
FIELD_RECIPES = {
    "field_cavlc_high8_sm2": dict(_P, width=64, height=64, frames=5, profile_idc=100, cabac=0, transform8x8=1, scaling_matrix=2, field_pics=1, num_ref_frames=2,
                                  intra_in_p_permille=250, deblock_idc=1, seed=13),
    "paff_cavlc_high8": dict(_P, width=64, height=64, frames=5, profile_idc=100, cabac=0, transform8x8=1, field_pics=3, num_ref_frames=2, intra_in_p_permille=250, seed=14),
    "field_cabac_high8": dict(_P, width=64, height=64, frames=4, profile_idc=100, cabac=1, transform8x8=1, field_pics=1, num_ref_frames=2, intra_in_p_permille=250,
                              chroma_qp_offset=12, seed=15),
}
MONO_RECIPES = {
    "mono_cabac_high8": dict(_P, width=64, height=48, frames=6, profile_idc=100, cabac=1, transform8x8=1, mono=1, num_ref_frames=2, seed=16),
}
_G = dict(_P, frames=3, profile_idc=77, cabac=1, num_ref_frames=2, seed=41)
GEOMETRY = {
    "geo_16x16": dict(_G, width=16, height=16), "geo_176x16": dict(_G, width=176, height=16), "geo_16x144": dict(_G, width=16, height=144),
    "geo_32x32": dict(_G, width=32, height=32),
}
RECIPES = dict(I_RECIPES, **P_RECIPES, **B_RECIPES, **FIELD_RECIPES, **MONO_RECIPES, **GEOMETRY)


def is_b(kw):
    return bool(kw.get("bframes"))


def is_field(kw):
    return bool(kw.get("field_pics"))


def main_eligible(kw):
    """a P recipe that k_entropy_m takes when it is decoded alone: CABAC, Main tools only, frame pictures with P slices"""
    return (kw["cabac"] == 1 and kw["profile_idc"] == 77 and not kw.get("transform8x8") and not is_b(kw) and not is_field(kw) and kw.get("idr_period", 1) != 1)
