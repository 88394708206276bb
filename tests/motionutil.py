"""Motion vector and reference index derivation (8.4.1) written once more, in plain Python, straight from 8.4.1.1 (P_Skip), 8.4.1.2.1 - 8.4.1.2.3 (the
co-located block, spatial and temporal direct prediction; frame pictures), 8.4.1.3 with 8.4.1.3.1 / 8.4.1.3.2 (the predictor and its neighbours) and
6.4.11.7 / 6.4.12 (neighbouring partitions, neighbouring locations): the yardstick of tests/test_motion_cells.py.

Independent of streamgen/sg_enc.c (get_nmv / mv_pred / b_direct), oracle/h264o_entropy.c and the entropy kernels (predict_mv, predict_mv16, direct_pred):
no code, no table and no structure of theirs.  A neighbour is found per LUMA LOCATION: the location relative to the macroblock's corner names a macroblock
by Table 6-3 (A, B, C, D, the current one, or nothing), the macroblock's availability is a matter of picture edge, slice and decoding order, and inside the
current macroblock the partition that covers the location is available when it comes EARLIER in the order (mbPartIdx, subMbPartIdx) than the partition being
derived -- never by a mask of finished blocks.  The input is the generator's motion trace (streamgen.last_motion_trace()): the syntax as written (mb_type,
sub_mb_type, ref_idx, signed mvd) and the slices' reference lists; the output is a vector per list and 4x4 block and an index per list and quadrant, to be
held against the trace's final vectors, the oracle's and the GPU's, and a CELL for every derivation that says which rule decided it.

What the rules say, as this file reads them (the project has no copy of the standard):
- 8.4.1.3.2: the neighbours of a partition at (x, y) of width w are the partitions that cover A = (x - 1, y), B = (x, y - 1), C = (x + w, y - 1); when C is
  not available, D = (x - 1, y - 1) takes its place.  A neighbour that is not available, is intra or does not use the list has refIdx -1 and a zero vector.
- 8.4.1.3: 16x8: the upper partition takes B's vector when refIdxB equals its own index, the lower one A's; 8x16: the left one A's, the right one C's.
  Otherwise the median (8.4.1.3.1): when B and C are both not available and A is, B and C become A; when exactly one of the three indices equals the
  partition's, that neighbour's vector; otherwise the median per component.
- 8.4.1.1: P_Skip: index 0; the vector is zero when macroblock A or B is not available, or A has index 0 and a zero vector, or B has; otherwise the
  predictor of the 16x16 partition.
- 8.4.1.2.2: spatial direct: per list the index is MinPositive(A, MinPositive(B, C)) of the MACROBLOCK's neighbours (the macroblock as one 16x16
  partition, also for a direct quadrant of B_8x8); both negative: both 0 with zero vectors.  A list with a negative index is not used.  colZeroFlag =
  RefPicList1[0] is a short-term picture and refIdxCol is 0 and both components of mvCol lie in -1 .. 1.  The vector of a list is zero when its index
  is 0 and colZeroFlag is set, otherwise the 16x16 predictor for that index.
- 8.4.1.2.1: the co-located macroblock is the one at the same address in RefPicList1[0]; the co-located 4x4 block is the same block, or with
  direct_8x8_inference_flag the corner block of its quadrant (raster blocks 0, 3, 12, 15).  Intra: mvCol 0, refIdxCol -1; list 0 used: its vector and index;
  otherwise list 1's.
- 8.4.1.2.3: temporal direct: refIdxL0 = 0 for an intra co-located block, otherwise the lowest index of RefPicList0 that holds the picture the co-located
  block predicted from; refIdxL1 = 0.  RefPicList0[refIdxL0] long-term, or the same PicOrderCnt as RefPicList1[0]: mvL0 = mvCol, mvL1 = 0.  Otherwise
  tb = Clip3(-128, 127, cur - poc0), td = Clip3(-128, 127, poc1 - poc0), tx = (16384 + Abs(td / 2)) / td, DistScaleFactor = Clip3(-1024, 1023,
  (tb * tx + 32) >> 6), mvL0 = (DistScaleFactor * mvCol + 128) >> 8, mvL1 = mvL0 - mvCol ("/" truncates towards zero, ">>" is arithmetic)."""
from collections import Counter

import numpy as np

KIND_INTRA, KIND_16x16, KIND_16x8, KIND_8x16, KIND_8x8, KIND_PSKIP, KIND_BDIRECT, KIND_BSKIP = range(8)   # the trace's macroblock kinds
SLICE_P, SLICE_B, SLICE_I = 0, 1, 2
L0, L1, BI = 1, 2, 3                 # which lists a partition predicts from, as a bit set

# Table 7-13 (P) and 7-14 (B): mb_type -> (shape, lists of partition 0, lists of partition 1)
P_MB = {0: ("16x16", L0, 0), 1: ("16x8", L0, L0), 2: ("8x16", L0, L0), 3: ("8x8", 0, 0), 4: ("8x8", 0, 0)}
B_MB = {0: ("direct", 0, 0), 1: ("16x16", L0, 0), 2: ("16x16", L1, 0), 3: ("16x16", BI, 0), 22: ("8x8", 0, 0)}
for _i, (_a, _b) in enumerate(((L0, L0), (L1, L1), (L0, L1), (L1, L0), (L0, BI), (L1, BI), (BI, L0), (BI, L1), (BI, BI))):
    B_MB[4 + 2 * _i], B_MB[5 + 2 * _i] = ("16x8", _a, _b), ("8x16", _a, _b)
# Table 7-17 (P) and 7-18 (B): sub_mb_type -> (width, height of a sub-macroblock partition in 4x4 blocks, lists); B 0 = direct
P_SUB = {0: (2, 2, L0), 1: (2, 1, L0), 2: (1, 2, L0), 3: (1, 1, L0)}
B_SUB = {0: None, 1: (2, 2, L0), 2: (2, 2, L1), 3: (2, 2, BI), 4: (2, 1, L0), 5: (1, 2, L0), 6: (2, 1, L1), 7: (1, 2, L1), 8: (2, 1, BI), 9: (1, 2, BI),
         10: (1, 1, L0), 11: (1, 1, L1), 12: (1, 1, BI)}


def _idiv(a, b):
    """the "/" of the standard: integer division with truncation towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _clip3(lo, hi, v):
    return lo if v < lo else (hi if v > hi else v)


def _median(a, b, c):
    return a + b + c - min(a, b, c) - max(a, b, c)


class Part:
    """a macroblock partition or sub-macroblock partition: place and size in 4x4 blocks, place in the order, shape for the directional rules, its lists"""
    def __init__(self, order, bx, by, w, h, shape, lists, pos):
        self.order, self.bx, self.by, self.w, self.h, self.shape, self.lists, self.pos = order, bx, by, w, h, shape, lists, pos


# the 41 partition positions: 1 (16x16) + 2 (16x8) + 2 (8x16) + 4 (8x8) + 8 (8x4) + 8 (4x8) + 16 (4x4)
def _position(bx, by, w, h):
    if (w, h) == (4, 4):
        return 0
    if (w, h) == (4, 2):
        return 1 + by // 2
    if (w, h) == (2, 4):
        return 3 + bx // 2
    q = (by // 2) * 2 + bx // 2
    if (w, h) == (2, 2):
        return 5 + q
    if (w, h) == (2, 1):
        return 9 + 2 * q + by % 2
    if (w, h) == (1, 2):
        return 17 + 2 * q + bx % 2
    return 25 + 4 * q + 2 * (by % 2) + bx % 2


def partitions(slice_type, raw, sub):
    """the partitions of a coded inter macroblock in decoding order, and the set of direct quadrants"""
    shape, la, lb = (P_MB if slice_type == SLICE_P else B_MB)[raw]
    if shape == "16x16":
        return [Part((0, 0), 0, 0, 4, 4, "med", la, _position(0, 0, 4, 4))], set()
    if shape == "16x8":
        return [Part((0, 0), 0, 0, 4, 2, "16x8u", la, _position(0, 0, 4, 2)), Part((1, 0), 0, 2, 4, 2, "16x8l", lb, _position(0, 2, 4, 2))], set()
    if shape == "8x16":
        return [Part((0, 0), 0, 0, 2, 4, "8x16l", la, _position(0, 0, 2, 4)), Part((1, 0), 2, 0, 2, 4, "8x16r", lb, _position(2, 0, 2, 4))], set()
    if shape == "direct":
        return [], {0, 1, 2, 3}
    parts, direct = [], set()
    for q in range(4):
        s = (P_SUB if slice_type == SLICE_P else B_SUB)[int(sub[q])]
        if s is None:
            direct.add(q)
            continue
        w, h, lists = s
        x0, y0 = (q % 2) * 2, (q // 2) * 2
        k = 0
        for y in range(y0, y0 + 2, h):
            for x in range(x0, x0 + 2, w):
                parts.append(Part((q, k), x, y, w, h, "med", lists, _position(x, y, w, h)))
                k += 1
    return parts, direct


class Picture:
    """the motion of one picture as the yardstick derived it (what later pictures take co-located blocks from)"""
    def __init__(self, t):
        self.t = t
        self.hmb, self.wmb = t["mbs"].shape
        n = self.hmb * self.wmb
        self.mv = np.zeros((n, 2, 16, 2), dtype=np.int64)
        self.ref = np.full((n, 2, 4), -1, dtype=np.int64)
        self.intra = np.zeros(n, dtype=bool)
        self.done = np.zeros(n, dtype=bool)
        self.slice_of = t["mbs"]["slice"].reshape(-1).astype(np.int64)
        self.absmvd = np.zeros((n, 2, 16, 2), dtype=np.int64)      # |mvd| as written, on every block of its partition (0: none written)
        self.cells = Counter()

    def fields(self):
        return self.mv.reshape(self.hmb, self.wmb, 2, 16, 2), self.ref.reshape(self.hmb, self.wmb, 2, 4)


class _Mb:
    """the macroblock being derived: its address, its slice, and for each 4x4 block the place of its partition in the order (None: nothing there yet)"""
    def __init__(self, pic, addr, sl_no, sl):
        self.pic, self.addr, self.sl_no, self.sl = pic, addr, sl_no, sl
        self.mx, self.my = addr % pic.wmb, addr // pic.wmb
        self.order = [None] * 16
        self.direct_blocks = set()

    def mb_available(self, dx, dy):
        """6.4.4 / 6.4.8: the macroblock at (mx + dx, my + dy) is available when it is inside the picture, belongs to this slice and was decoded before"""
        x, y = self.mx + dx, self.my + dy
        if not (0 <= x < self.pic.wmb and 0 <= y < self.pic.hmb):
            return None
        a = y * self.pic.wmb + x
        if not self.pic.done[a] or self.pic.slice_of[a] != self.sl_no:
            return None
        return a

    def neighbour(self, lst, xn, yn, cur_order):
        """6.4.12 with Table 6-3, then the partition covering the location: (available, refIdx, (mvx, mvy), where, what) for list lst at the luma location
        (xn, yn) relative to this macroblock's corner.  where: "in_done" / "in_later" inside this macroblock, "A" / "B" / "C" / "D" / "outside"; what: "nolist" for
        an available inter partition that does not use the list, "direct" for a direct quadrant of this macroblock that uses it, else None."""
        if yn > 15 or (xn > 15 and yn >= 0):
            return False, -1, (0, 0), "outside", None
        if 0 <= xn <= 15 and yn >= 0:
            b = (yn // 4) * 4 + xn // 4
            if self.order[b] is None or not self.order[b] < cur_order:
                return False, -1, (0, 0), "in_later", None
            a, where = self.addr, "in_done"
        else:
            letter, dx, dy = ("D", -1, -1) if xn < 0 and yn < 0 else (("A", -1, 0) if xn < 0 else (("C", 1, -1) if xn > 15 else ("B", 0, -1)))
            a = self.mb_available(dx, dy)
            if a is None:
                return False, -1, (0, 0), "outside", None
            b, where = ((yn + 16) % 16 // 4) * 4 + (xn + 16) % 16 // 4, letter
        if self.pic.intra[a]:
            return True, -1, (0, 0), where, None
        q = (b // 8) * 2 + (b % 4) // 2
        r = int(self.pic.ref[a, lst, q])
        if r < 0:
            return True, -1, (0, 0), where, "nolist"
        what = "direct" if where == "in_done" and b in self.direct_blocks else None
        return True, r, (int(self.pic.mv[a, lst, b, 0]), int(self.pic.mv[a, lst, b, 1])), where, what

    def abc(self, lst, bx, by, w, cur_order):
        """8.4.1.3.2: the three neighbours of the partition at block (bx, by), w blocks wide; D stands in for a C that is not available"""
        x, y = 4 * bx, 4 * by
        a = self.neighbour(lst, x - 1, y, cur_order)
        b = self.neighbour(lst, x, y - 1, cur_order)
        c = self.neighbour(lst, x + 4 * w, y - 1, cur_order)
        cwhere, csrc = c[3], "C"
        if not c[0]:
            c = self.neighbour(lst, x - 1, y - 1, cur_order)
            csrc = "D" if c[0] else "none"
        return a, b, c, cwhere, csrc

    def predict(self, lst, bx, by, w, shape, ref_idx, cur_order, pos=None, count=True):
        """8.4.1.3: mvpLX of the partition"""
        a, b, c, cwhere, csrc = self.abc(lst, bx, by, w, cur_order)
        st = "B" if self.sl["type"] == SLICE_B else "P"
        if count:   # the geometry of a predictor that goes into the stream: where its C lies, whether D stood in, what its three neighbours are
            self.pic.cells[("geo", pos, cwhere)] += 1
            if csrc == "D":
                self.pic.cells[("geo_d", pos)] += 1
            for n in (a, b, c):
                if n[4] == "nolist":
                    self.pic.cells[("nolist", n[3])] += 1
                elif n[4] == "direct":
                    self.pic.cells[("direct_nb", "spatial" if self.sl["direct_spatial"] else "temporal")] += 1

        def note(rule):
            if count:
                self.pic.cells[("pred", st, lst, shape, rule)] += 1
                self.pic.cells[("csrc", st, lst, csrc)] += 1
        hit = {"16x8u": b, "16x8l": a, "8x16l": a, "8x16r": c}.get(shape)
        if hit is not None and hit[1] == ref_idx:
            note("dir")
            return hit[2]
        only_a = not b[0] and not c[0] and a[0]
        if only_a:
            b = c = a
        same = [n for n in (a, b, c) if n[1] == ref_idx]
        if only_a:
            note("onlyA")
        if len(same) == 1:
            if not only_a:
                note("one" + "ABC"[[n[1] == ref_idx for n in (a, b, c)].index(True)])
            return same[0][2]
        if not only_a:
            note("med%d" % len(same))
        return _median(a[2][0], b[2][0], c[2][0]), _median(a[2][1], b[2][1], c[2][1])

    def fill(self, lst, bx, by, w, h, ref_idx, mv, order):
        for y in range(by, by + h):
            for x in range(bx, bx + w):
                self.pic.mv[self.addr, lst, 4 * y + x] = mv
                self.pic.ref[self.addr, lst, (y // 2) * 2 + x // 2] = ref_idx
                self.order[4 * y + x] = order


def _col_block(cells, earlier, sl, addr, b, inference):
    """8.4.1.2.1 (frame pictures): (mvCol, refIdxCol, identity of the picture the co-located block predicted from or None, "intra" / "l0" / "l1only") of
    4x4 block b (raster) of macroblock addr"""
    col = earlier[int(sl["col_index"])]
    assert col is not None and col.t["pic"] == sl["pic"][1][0], "RefPicList1[0] is not a traced picture"
    bc = (0, 3, 12, 15)[(b // 8) * 2 + (b % 4) // 2] if inference else b
    if inference and bc != b and not col.intra[addr]:
        first = (0, 2, 8, 10)[(b // 8) * 2 + (b % 4) // 2]
        ll = 0 if col.ref[addr, 0, (b // 8) * 2 + (b % 4) // 2] >= 0 else 1
        if b == first and tuple(col.mv[addr, ll, bc]) != tuple(col.mv[addr, ll, first]):
            cells[("col", "corner_differs")] += 1
    if col.intra[addr]:
        return (0, 0), -1, None, "intra"
    q = (bc // 8) * 2 + (bc % 4) // 2
    lst, kind = (0, "l0") if col.ref[addr, 0, q] >= 0 else (1, "l1only")
    r = int(col.ref[addr, lst, q])
    assert r >= 0, "an inter macroblock whose co-located block uses neither list"
    csl = col.t["slices"][int(col.slice_of[addr])]
    return (int(col.mv[addr, lst, bc, 0]), int(col.mv[addr, lst, bc, 1])), r, int(csl["pic"][lst][r]), kind


def _direct(mb, earlier, quadrants, inference, whole):
    """8.4.1.2.2 / 8.4.1.2.3 for the direct quadrants of the macroblock"""
    pic, sl, cells = mb.pic, mb.sl, mb.pic.cells
    order = {q: (q, 0) for q in quadrants}
    blocks_of = {q: [((q // 2) * 2 + dy) * 4 + (q % 2) * 2 + dx for dy in (0, 1) for dx in (0, 1)] for q in quadrants}
    if not inference:
        for q in quadrants:
            cols = {_col_block(cells, earlier, sl, mb.addr, b, False)[0] for b in blocks_of[q]}
            if len(cols) == 4:
                cells[("col", "four_unlike")] += 1
    if sl["direct_spatial"]:
        refs, mvp = [], []
        for lst in (0, 1):
            a, b, c, _, _ = mb.abc(lst, 0, 0, 4, (0, 0))
            r, src = -1, "none"
            for n, name in ((a, "A"), (b, "B"), (c, "C")):          # MinPositive over the three
                if n[1] >= 0 and (r < 0 or n[1] < r):
                    r, src = n[1], name
            refs.append(r)
            cells[("sd_ref", lst, src)] += 1
        zero_pred = refs[0] < 0 and refs[1] < 0
        if zero_pred:
            refs = [0, 0]
            cells[("sd_bothneg",)] += 1
        for lst in (0, 1):
            mvp.append(mb.predict(lst, 0, 0, 4, "med", refs[lst], (0, 0), count=False) if refs[lst] >= 0 and not zero_pred else (0, 0))
        short = not sl["long_term"][1][0]
        for q in sorted(quadrants):
            for b in blocks_of[q]:
                mvcol, refcol, _, kind = _col_block(cells, earlier, sl, mb.addr, b, inference)
                colzero = short and refcol == 0 and -1 <= mvcol[0] <= 1 and -1 <= mvcol[1] <= 1
                cells[("col", kind)] += 1
                cells[("sd_col", "short" if short else "long")] += 1
                if kind != "intra":
                    cells[("sd_refcol", "zero" if refcol == 0 else "pos")] += 1
                    for comp in (0, 1):
                        if short and refcol == 0 and -2 <= mvcol[comp] <= 2 and -1 <= mvcol[1 - comp] <= 1:
                            cells[("sd_mvcol", comp, mvcol[comp])] += 1
                for lst in (0, 1):
                    if refs[lst] < 0:
                        out, mv = "neg", (0, 0)
                    elif zero_pred:
                        out, mv = "bothneg", (0, 0)
                    elif refs[lst] == 0 and colzero:
                        out, mv = "zeroed", (0, 0)
                    else:
                        out, mv = ("kept0" if refs[lst] == 0 else ("keptpos_flag" if colzero else "keptpos")), mvp[lst]
                    cells[("sd_out", lst, out)] += 1
                    mb.fill(lst, b % 4, b // 4, 1, 1, refs[lst], mv if refs[lst] >= 0 else (0, 0), order[q])
    else:
        cells[("td", "mb16" if whole else "quadrant")] += 1
        for q in sorted(quadrants):
            for b in blocks_of[q]:
                mvcol, refcol, target, kind = _col_block(cells, earlier, sl, mb.addr, b, inference)
                cells[("col", kind)] += 1
                if refcol < 0:
                    r0 = 0
                else:
                    found = [i for i in range(int(sl["nref"][0])) if int(sl["pic"][0][i]) == target]
                    assert found, ("temporal direct: the co-located block's reference picture is not in RefPicList0", mb.addr, b)
                    r0 = found[0]
                cells[("td_ref", "zero" if r0 == 0 else "pos")] += 1
                poc0, poc1, cur = int(sl["poc"][0][r0]), int(sl["poc"][1][0]), int(sl["cur_poc"])
                if sl["long_term"][0][r0] or poc1 - poc0 == 0:
                    mv0, mv1 = mvcol, (0, 0)
                    cells[("td", "long" if sl["long_term"][0][r0] else "same_poc")] += 1
                else:
                    tb, td = _clip3(-128, 127, cur - poc0), _clip3(-128, 127, poc1 - poc0)
                    tx = _idiv(16384 + abs(_idiv(td, 2)), td)
                    dsf = _clip3(-1024, 1023, (tb * tx + 32) >> 6)
                    mv0 = tuple((dsf * v + 128) >> 8 for v in mvcol)
                    mv1 = tuple(m - v for m, v in zip(mv0, mvcol))
                    if any(v < 0 and (dsf * v + 128) % 256 for v in mvcol):
                        cells[("td", "neg_remainder")] += 1
                mb.fill(0, b % 4, b // 4, 1, 1, r0, mv0, order[q])
                mb.fill(1, b % 4, b // 4, 1, 1, 0, mv1, order[q])
    for q in quadrants:
        mb.direct_blocks.update(blocks_of[q])


def derive_picture(t, earlier, inference=True):
    """8.4.1 on one picture of streamgen.last_motion_trace(): every macroblock in decoding order (slice by slice as sent, ascending addresses inside a
    slice).  earlier: the Picture objects of the pictures before it in the trace (None for one that was not derived).  Returns a Picture: .fields() = (vectors
    [rows, columns, list, block, 2], indices [rows, columns, list, quadrant]), .cells = a Counter of the cells of every derivation."""
    assert t["field"] == 0, "frame pictures only"
    pic = Picture(t)
    mbs = t["mbs"].reshape(-1)
    for sl_no, sl in enumerate(t["slices"]):
        st = int(sl["type"])
        addrs = [a for a in range(len(mbs)) if mbs[a]["slice"] == sl_no]
        assert len(addrs) == sl["count"] and (not addrs or addrs[0] == sl["first_mb"]), ("slice table and macroblock table disagree", sl_no)
        for addr in addrs:
            m = mbs[addr]
            mb = _Mb(pic, addr, sl_no, sl)
            kind, raw = int(m["kind"]), int(m["raw"])
            if kind == KIND_INTRA:
                pic.intra[addr] = True
            elif kind == KIND_PSKIP:
                assert st == SLICE_P
                a_mb, b_mb = mb.mb_available(-1, 0), mb.mb_available(0, -1)
                a, b, _, _, _ = mb.abc(0, 0, 0, 4, (0, 0))
                if a_mb is None:
                    why, mv = "A_missing", (0, 0)
                elif b_mb is None:
                    why, mv = "B_missing", (0, 0)
                elif a[1] == 0 and a[2] == (0, 0):
                    why, mv = "A_still", (0, 0)
                elif b[1] == 0 and b[2] == (0, 0):
                    why, mv = "B_still", (0, 0)
                else:
                    mv = mb.predict(0, 0, 0, 4, "med", 0, (0, 0), pos=0)
                    why = "predicted_zero" if mv == (0, 0) else "predicted_nonzero"
                pic.cells[("pskip", why)] += 1
                mb.fill(0, 0, 0, 4, 4, 0, mv, (0, 0))
            elif kind in (KIND_BDIRECT, KIND_BSKIP):
                assert st == SLICE_B and raw == (0 if kind == KIND_BDIRECT else -1)
                if kind == KIND_BDIRECT:
                    pic.cells[("mb_type", "B", 0)] += 1
                _direct(mb, earlier, {0, 1, 2, 3}, inference, True)
            else:
                assert st in (SLICE_P, SLICE_B)
                pic.cells[("mb_type", "PB"[st], raw)] += 1
                parts, direct = partitions(st, raw, m["sub"])
                assert {KIND_16x16: 1, KIND_16x8: 2, KIND_8x16: 2}.get(kind, 0) == (len(parts) if kind != KIND_8x8 else 0), ("kind and mb_type disagree", addr)
                if kind == KIND_8x8:
                    assert direct == {q for q in range(4) if m["direct8"] >> q & 1}
                    for q in range(4):
                        pic.cells[("sub_mb_type", "PB"[st], int(m["sub"][q]))] += 1
                if direct:
                    _direct(mb, earlier, direct, inference, False)
                for lst in ((0,) if st == SLICE_P else (0, 1)):
                    for p in parts:
                        q = (p.by // 2) * 2 + p.bx // 2
                        if not p.lists >> lst & 1:
                            # the partition does not use the list: refIdx -1, a zero vector, and it is there for those after it
                            for y in range(p.by, p.by + p.h):
                                for x in range(p.bx, p.bx + p.w):
                                    mb.order[4 * y + x] = p.order
                            continue
                        r = 0 if (st == SLICE_P and raw == 4) else int(m["ref_idx"][lst][q])
                        assert 0 <= r < sl["nref"][lst], ("ref_idx out of the list", addr, lst, q, r)
                        mvp = mb.predict(lst, p.bx, p.by, p.w, p.shape, r, p.order, pos=p.pos)
                        mvd = m["mvd"][lst][4 * p.by + p.bx]
                        mb.fill(lst, p.bx, p.by, p.w, p.h, r, (mvp[0] + int(mvd[0]), mvp[1] + int(mvd[1])), p.order)
                        for y in range(p.by, p.by + p.h):
                            for x in range(p.bx, p.bx + p.w):
                                pic.absmvd[addr, lst, 4 * y + x] = (abs(int(mvd[0])), abs(int(mvd[1])))
                    # (list 1 starts over: what counts is the place of a partition in the order, and every partition has its place by now)
            pic.done[addr] = True
    return pic


SYNTAX_MASKS = ("ref_inc", "skip_inc_p", "skip_inc_b", "btype_inc")
SYNTAX_COUNTS = ("ref_ge3", "ref_direct_nb", "ref_te1", "ref_ue", "mvd_suffix") + tuple("mvd_band_%s_%d" % (c, b) for c in "xy" for b in range(3))


def count_syntax(pic, cabac):
    """The motion syntax of a derived picture, counted again from the trace as 7.3.5 / 9.3.3.1.1 read (the names of streamgen.last_motion()): per ref_idx
    written the ctxIdxInc of its first bin -- condTermFlagN is 1 when neighbour partition N (A to the left, B above) is available, not intra, not skipped,
    not predicted in direct mode, uses the list and has an index above 0; ctxIdxInc = condTermFlagA + 2 condTermFlagB --, indices of at least 3, a direct
    or B-skipped neighbour, te() with one bit (two active entries) or as ue(); per mvd component the sum of |mvd| of A and B (0 for a neighbour that is not
    available, intra, skipped, direct or does not use the list) in its band below 3, 3 .. 32, above 32, and |mvd| of 9 and above; per macroblock of a P / B
    slice the ctxIdxInc of mb_skip_flag (neighbours that are available and not skipped) and, for a B macroblock that is not skipped, of the first bin of
    mb_type (neighbours that are available and neither B_Skip nor B_Direct_16x16).  Masks are bit sets of increments, the rest are counts."""
    out = dict.fromkeys(SYNTAX_MASKS + SYNTAX_COUNTS, 0)
    mbs, done = pic.t["mbs"].reshape(-1), set()
    for sl_no, sl in enumerate(pic.t["slices"]):
        st = int(sl["type"])
        for addr in [a for a in range(len(mbs)) if mbs[a]["slice"] == sl_no]:
            m, mx, my = mbs[addr], addr % pic.wmb, addr // pic.wmb
            kind = int(m["kind"])

            def there(dx, dy):
                x, y = mx + dx, my + dy
                a = y * pic.wmb + x
                return a if 0 <= x < pic.wmb and 0 <= y < pic.hmb and a in done and mbs[a]["slice"] == sl_no else None

            def part_at(bx, by):     # (macroblock, block) of the partition that covers the block, which may lie one to the left of or above this macroblock
                if bx < 0:
                    return there(-1, 0), 4 * by + 3
                if by < 0:
                    return there(0, -1), 12 + bx
                return addr, 4 * by + bx

            def direct_at(a, b):
                return bool(int(mbs[a]["direct8"]) >> ((b // 8) * 2 + (b % 4) // 2) & 1)

            if st != SLICE_I and cabac:
                a_mb, b_mb = there(-1, 0), there(0, -1)
                skipped = (KIND_PSKIP, KIND_BSKIP)
                out["skip_inc_b" if st == SLICE_B else "skip_inc_p"] |= 1 << sum(1 for n in (a_mb, b_mb) if n is not None and int(mbs[n]["kind"]) not in skipped)
                if st == SLICE_B and kind != KIND_BSKIP:
                    out["btype_inc"] |= 1 << sum(1 for n in (a_mb, b_mb) if n is not None and int(mbs[n]["kind"]) not in (KIND_BSKIP, KIND_BDIRECT))
            if kind in (KIND_16x16, KIND_16x8, KIND_8x16, KIND_8x8):
                raw = int(m["raw"])
                parts, direct = partitions(st, raw, m["sub"])
                for lst in ((0,) if st == SLICE_P else (0, 1)):
                    nref = int(sl["nref"][lst])
                    seen = set()
                    for p in parts:       # ref_idx: one per macroblock partition (per quadrant of an 8x8 macroblock) that uses the list
                        q = (p.by // 2) * 2 + p.bx // 2
                        if not p.lists >> lst & 1 or q in seen or nref < 2 or (st == SLICE_P and raw == 4):
                            continue
                        seen.add(q)
                        r = int(m["ref_idx"][lst][q])
                        out["ref_ge3"] += r >= 3
                        if not cabac:
                            out["ref_ue" if nref - 1 > 1 else "ref_te1"] += 1
                            continue
                        inc, dnb = 0, False
                        for weight, (na, nb) in ((1, part_at(p.bx - 1, p.by)), (2, part_at(p.bx, p.by - 1))):
                            if na is None or pic.intra[na]:
                                continue
                            if direct_at(na, nb):
                                dnb = True
                                continue
                            if int(mbs[na]["kind"]) not in (KIND_PSKIP, KIND_BSKIP, KIND_BDIRECT) and pic.ref[na, lst, (nb // 8) * 2 + (nb % 4) // 2] > 0:
                                inc += weight
                        out["ref_inc"] |= 1 << inc
                        out["ref_direct_nb"] += dnb and st == SLICE_B
                    for p in parts:       # mvd: one per (sub-macroblock) partition that uses the list
                        if not p.lists >> lst & 1 or not cabac:
                            continue
                        for comp, c in enumerate("xy"):
                            total = sum(int(pic.absmvd[na, lst, nb, comp]) for na, nb in (part_at(p.bx - 1, p.by), part_at(p.bx, p.by - 1)) if na is not None)
                            out["mvd_band_%s_%d" % (c, (total > 2) + (total > 32))] += 1
                            out["mvd_suffix"] += abs(int(m["mvd"][lst][4 * p.by + p.bx][comp])) >= 9
            done.add(addr)
    return out


def derive_stream(trace, inference=True):
    """every picture of a trace, in coding order; returns the list of Picture objects"""
    out = []
    for t in trace:
        out.append(derive_picture(t, list(out), inference))
    return out


def first_difference(pics, trace):
    """None, or (picture, macroblock address, list, "mv" / "ref", block or quadrant, yardstick value, trace value) of the first place where the yardstick's
    field and the trace's final vectors / indices differ"""
    for i, (p, t) in enumerate(zip(pics, trace)):
        mbs = t["mbs"].reshape(-1)
        for a in range(len(mbs)):
            for lst in (0, 1):
                for q in range(4):
                    if p.ref[a, lst, q] != mbs[a]["ref"][lst][q]:
                        return i, a, lst, "ref", q, int(p.ref[a, lst, q]), int(mbs[a]["ref"][lst][q])
                for b in range(16):
                    want = tuple(int(v) for v in mbs[a]["mv"][lst][b]) if mbs[a]["ref"][lst][(b // 8) * 2 + (b % 4) // 2] >= 0 else (0, 0)
                    if tuple(int(v) for v in p.mv[a, lst, b]) != want:
                        return i, a, lst, "mv", b, tuple(int(v) for v in p.mv[a, lst, b]), want
    return None


def planes_of(pic):
    """the yardstick's field of a picture as the planes of Decoder.side_info: {"mvx0", "mvy0", "ref0", "mvx1", "mvy1", "ref1"} -> int array [4 * rows,
    4 * columns], one cell per 4x4 block (vectors 0 and index -1 where the list is not used), and "kind" -> the trace's macroblock kind per block"""
    mv, ref = pic.fields()
    hmb, wmb = pic.hmb, pic.wmb
    out = {}
    for lst in (0, 1):
        r = np.repeat(np.repeat(ref[:, :, lst].reshape(hmb, wmb, 2, 2).transpose(0, 2, 1, 3).reshape(2 * hmb, 2 * wmb), 2, axis=0), 2, axis=1)
        for c, name in ((0, "mvx"), (1, "mvy")):
            v = mv[:, :, lst, :, c].reshape(hmb, wmb, 4, 4).transpose(0, 2, 1, 3).reshape(4 * hmb, 4 * wmb)
            out["%s%d" % (name, lst)] = np.where(r >= 0, v, 0)
        out["ref%d" % lst] = r
    out["kind"] = np.repeat(np.repeat(pic.t["mbs"]["kind"].astype(np.int64), 4, axis=0), 4, axis=1)
    out["slice_type"] = np.repeat(np.repeat(pic.t["slices"]["type"][pic.t["mbs"]["slice"]].astype(np.int64), 4, axis=0), 4, axis=1)
    return out


# ---- the cells that can be reached at all, enumerated from the rules (never from what a stream gave) ----
_SHAPE_RULES = {
    # which rule can decide a partition of each shape.  A directional hit takes the neighbour whose index matches out of the median: the upper 16x8
    # partition never ends on "B alone", nor can all three match; the lower one's B (the upper partition) is always there, so A is never alone; ...
    "med": ("onlyA", "oneA", "oneB", "oneC", "med0", "med2", "med3"),
    "16x8u": ("dir", "onlyA", "oneA", "oneC", "med0", "med2"),
    "16x8l": ("dir", "oneB", "oneC", "med0", "med2"),
    "8x16l": ("dir", "onlyA", "oneB", "oneC", "med0", "med2"),
    "8x16r": ("dir", "onlyA", "oneA", "oneB", "med0", "med2"),
}


def _all_positions():
    """(position, bx, by, w, h, place in the order) of the 41 partition positions"""
    out = [(0, 0, 0, 4, 4, (0, 0)), (1, 0, 0, 4, 2, (0, 0)), (2, 0, 2, 4, 2, (1, 0)), (3, 0, 0, 2, 4, (0, 0)), (4, 2, 0, 2, 4, (1, 0))]
    for q in range(4):
        x0, y0 = (q % 2) * 2, (q // 2) * 2
        for w, h in ((2, 2), (2, 1), (1, 2), (1, 1)):
            k = 0
            for y in range(y0, y0 + 2, h):
                for x in range(x0, x0 + 2, w):
                    out.append((_position(x, y, w, h), x, y, w, h, (q, k)))
                    k += 1
    assert sorted(o[0] for o in out) == list(range(41))
    return out


def reachable_cells():
    """the cells of the families this file counts, as far as the availability rules let them occur (picture edges, slice edges, slice groups, the order
    inside a macroblock)"""
    cells = set()
    for st, lists in (("P", (0,)), ("B", (0, 1))):
        for lst in lists:
            cells |= {("pred", st, lst, shape, rule) for shape, rules in _SHAPE_RULES.items() for rule in rules}
            cells |= {("csrc", st, lst, c) for c in ("C", "D", "none")}
    for pos, bx, by, w, h, order in _all_positions():
        x, y = 4 * (bx + w), 4 * by - 1
        if y < 0:
            cells |= {("geo", pos, "C" if x > 15 else "B"), ("geo", pos, "outside")}     # a neighbouring macroblock, there or not
            # D stands in when that macroblock is missing and D's is there: above right missing is the picture's right edge; the macroblock above missing
            # takes D's (the same one, or for a partition at the left edge the one above left) with it, except across slice groups
            if x > 15 or bx == 0:
                cells.add(("geo_d", pos))
        elif x > 15:
            cells |= {("geo", pos, "outside"), ("geo_d", pos)}                           # to the right of the macroblock: never there
        else:
            # inside the macroblock: the partition there comes earlier or later, by quadrant first and by sub-macroblock partition second
            q, qc = (by // 2) * 2 + bx // 2, (y // 8) * 2 + x // 8
            earlier = qc < q or (qc == q and order[1] > 0 and y // 4 < by)
            cells.add(("geo", pos, "in_done" if earlier else "in_later"))
            if not earlier:
                cells.add(("geo_d", pos))                                                # D lies inside the macroblock then, and earlier
    cells |= {("pskip", w) for w in ("A_missing", "B_missing", "A_still", "B_still", "predicted_nonzero", "predicted_zero")}
    cells |= {("sd_ref", lst, src) for lst in (0, 1) for src in ("A", "B", "C", "none")} | {("sd_bothneg",)}
    cells |= {("sd_col", "short"), ("sd_col", "long"), ("sd_refcol", "zero"), ("sd_refcol", "pos")}
    cells |= {("sd_mvcol", comp, v) for comp in (0, 1) for v in (-2, -1, 0, 1, 2)}
    cells |= {("sd_out", lst, o) for lst in (0, 1) for o in ("neg", "zeroed", "kept0", "keptpos_flag")}
    cells |= {("col", k) for k in ("intra", "l0", "l1only", "corner_differs", "four_unlike")}
    cells |= {("td_ref", "zero"), ("td_ref", "pos"), ("td", "neg_remainder"), ("td", "long"), ("td", "mb16"), ("td", "quadrant"), ("direct_nb", "temporal"),
              ("direct_nb", "spatial")}
    cells |= {("mb_type", "P", v) for v in range(5)} | {("mb_type", "B", v) for v in range(1, 23)} | {("mb_type", "B", 0)}
    cells |= {("sub_mb_type", "P", v) for v in range(4)} | {("sub_mb_type", "B", v) for v in range(13)}
    cells |= {("nolist", w) for w in ("in_done", "A", "B", "C", "D")}
    return cells


FAMILY = {"pred": "predictor", "csrc": "predictor", "geo": "geometry", "nolist": "geometry", "pskip": "P_Skip", "sd_ref": "spatial", "sd_bothneg": "spatial",
          "sd_col": "spatial", "sd_refcol": "spatial", "sd_mvcol": "spatial", "sd_out": "spatial", "col": "co-located", "td_ref": "temporal", "td": "temporal",
          "direct_nb": "temporal", "geo_d": "geometry", "mb_type": "syntax", "sub_mb_type": "syntax"}
NO_EXEMPTION = ("P_Skip", "co-located", "temporal")
# reachable cells that no recipe reaches, each by name with its reason.  At most one in twenty of a family, none in the families of NO_EXEMPTION.
EXEMPT = {
}


def counted(cells):
    """the cells of a Counter that belong to the enumerated families (cells counted for the record only -- ("sd_out", ..., "keptpos"),
    ("sd_out", ..., "bothneg"), ("td", "same_poc") -- are left out)"""
    reach = reachable_cells()
    return {c for c in cells if c in reach}


def beyond_reach(cells):
    """cells of the enumerated kinds that were counted although the enumeration says they cannot occur"""
    reach = reachable_cells()
    kinds = {"pred", "csrc", "geo", "geo_d", "pskip", "sd_ref", "col", "td_ref", "mb_type", "sub_mb_type", "nolist"}
    return sorted(c for c in cells if c[0] in kinds and c not in reach)


def cell_line(name, cells):
    """a recipe's cells as one line of tests/golden/motion_counters.txt: per family the number of distinct cells and of derivations counted"""
    per = {}
    for c, n in cells.items():
        f = FAMILY.get(c[0])
        if f and c in reachable_cells():
            d = per.setdefault(f, [0, 0])
            d[0] += 1
            d[1] += n
    return "  %-30s %s" % (name, " ".join("%s=%d/%d" % (f.replace(" ", "_"), per[f][0], per[f][1]) for f in sorted(per)))


# ---- recipes of tests/test_motion_cells.py ----
# Frame pictures of 48x32 .. 96x80 with at most 8 frames, and the five geometries of test_entropy_p16_gpu.py with 4 frames.
_P = dict(idr_period=0, skip_permille=120, sub8x8_permille=550, intra_in_p_permille=60, trace_motion=1, motion_stim=1)
_B = dict(_P, bframes=2, num_ref_frames=3, bskip_permille=140, profile_idc=77)
P_RECIPES = {
    "p_cabac_1ref": dict(_P, width=64, height=48, frames=6, profile_idc=77, cabac=1, num_ref_frames=1, seed=1),
    "p_cabac_3ref": dict(_P, width=96, height=80, frames=8, profile_idc=77, cabac=1, num_ref_frames=3, seed=200),
    "p_cabac_3ref_3slices_midrow": dict(_P, width=80, height=64, frames=6, profile_idc=77, cabac=1, num_ref_frames=3, slices=3, intra_stim=1, seed=3),
    "p_cabac_intra_neighbours": dict(_P, width=80, height=64, frames=6, profile_idc=77, cabac=1, num_ref_frames=3, intra_in_p_permille=350, seed=4),
    "p_cabac_sub_heavy": dict(_P, width=64, height=64, frames=8, profile_idc=77, cabac=1, num_ref_frames=3, sub8x8_permille=900, skip_permille=40, seed=5),
    "p_cavlc_1ref": dict(_P, width=48, height=32, frames=6, profile_idc=66, cabac=0, num_ref_frames=1, seed=6),
    "p_cavlc_3ref_3slices_midrow": dict(_P, width=80, height=64, frames=6, profile_idc=66, cabac=0, num_ref_frames=3, slices=3, intra_stim=1, seed=7),
    "p_cavlc_sub_heavy_still": dict(_P, width=64, height=64, frames=8, profile_idc=66, cabac=0, num_ref_frames=3, sub8x8_permille=800, skip_permille=250,
                                    motion_x4=0, motion_y4=0, mv_reach=3, seed=8),
    # P_8x8ref0: CAVLC, several active references, P_8x8 macroblocks whose four indices are 0
    "p_cavlc_8x8ref0": dict(_P, width=80, height=64, frames=6, profile_idc=66, cabac=0, num_ref_frames=3, sub8x8_permille=800, seed=9),
}
B_RECIPES = {
    "b_spatial_cabac": dict(_B, width=96, height=80, frames=7, cabac=1, seed=11),
    "b_spatial_d4_cabac": dict(_B, width=80, height=64, frames=7, cabac=1, direct_4x4=1, seed=12),
    "b_spatial_d4_cavlc_still": dict(_B, width=80, height=64, frames=7, cabac=0, direct_4x4=1, motion_x4=1, motion_y4=-1, mv_reach=3, seed=201),
    "b_spatial_cavlc_8x8": dict(_B, width=64, height=64, frames=7, cabac=0, profile_idc=100, transform8x8=1, seed=14),
    "b_spatial_d4_cabac_8x8": dict(_B, width=64, height=64, frames=7, cabac=1, profile_idc=100, transform8x8=1, direct_4x4=1, seed=15),
    "b_temporal_cabac": dict(_B, width=96, height=80, frames=7, cabac=1, direct_temporal=1, seed=16),
    "b_temporal_d4_cavlc": dict(_B, width=80, height=64, frames=7, cabac=0, direct_temporal=1, direct_4x4=1, seed=17),
    "b_temporal_d4_cabac_8x8": dict(_B, width=64, height=64, frames=7, cabac=1, profile_idc=100, transform8x8=1, direct_temporal=1, direct_4x4=1, seed=18),
    "b_temporal_cavlc_8x8": dict(_B, width=64, height=48, frames=7, cabac=0, profile_idc=100, transform8x8=1, direct_temporal=1, seed=19),
    "b_pyramid_temporal_cabac": dict(_B, width=80, height=64, frames=8, cabac=1, bframes=3, b_pyramid=1, direct_temporal=1, seed=20),
    "b_pyramid_spatial_d4_cabac": dict(_B, width=80, height=64, frames=8, cabac=1, bframes=3, b_pyramid=1, direct_4x4=1, seed=21),
    "b_spatial_3slices_cabac": dict(_B, width=80, height=64, frames=7, cabac=1, slices=3, intra_stim=1, seed=22),
    # a long-term IDR picture: RefPicList1[0] of the first B pictures (colZeroFlag asks for a short-term one), and the picture a co-located block predicted from
    "b_spatial_long_term_cabac": dict(_B, width=80, height=64, frames=7, cabac=1, idr_long_term=1, seed=23),
    "b_temporal_long_term_cavlc": dict(_B, width=80, height=64, frames=7, cabac=0, direct_temporal=1, idr_long_term=1, seed=24),
}
FMO_RECIPES = {
    "fmo_checkerboard_p_cavlc": dict(_P, width=96, height=80, frames=5, profile_idc=66, cabac=0, num_ref_frames=2, slice_groups=2, fmo_type=1, seed=200),
}
_G = dict(_P, frames=4, profile_idc=77, cabac=1, num_ref_frames=2, seed=41)
GEOMETRY = {
    "geo_16x16": dict(_G, width=16, height=16), "geo_176x16": dict(_G, width=176, height=16), "geo_16x144": dict(_G, width=16, height=144),
    "geo_32x32": dict(_G, width=32, height=32), "geo_176x144": dict(_G, width=176, height=144),
    "geo_176x144_b": dict(_B, width=176, height=144, frames=4, cabac=1, seed=42),
}
RECIPES = dict(P_RECIPES, **B_RECIPES, **FMO_RECIPES, **GEOMETRY)


def is_b(kw):
    return bool(kw.get("bframes"))


def main_eligible(kw):
    """a P recipe that k_entropy_m takes when it is decoded alone: CABAC, no 8x8 transform, no slice groups, no B pictures"""
    return kw["cabac"] == 1 and not kw.get("transform8x8") and kw.get("slice_groups", 0) <= 1 and not is_b(kw)
