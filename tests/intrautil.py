"""Intra prediction (8.3) written once more, in numpy on int64, straight from 8.3.1.2, 8.3.2.2 (with 8.3.2.2.1), 8.3.3 and 8.3.4, with the availability
rules it needs (6.4.3 / 6.4.5 inverse block scans, 6.4.12 neighbouring locations, macroblock availability by slice and address,
constrained_intra_pred_flag): the yardstick of tests/test_intra_cells.py.

Independent of streamgen/sg_recon.c, oracle/h264o_recon.c and the kernels: no code and no table of theirs.  Availability is decided per SAMPLE LOCATION
(which macroblock it lies in by Table 6-3; inside the current macroblock: which block by the inverse scan, and "a block with a greater index is not
there yet"), never by a closed formula over block coordinates.  The neighbouring samples of a block are laid out on ONE line -- the left column bottom
to top, the corner, the row above left to right -- so that the three-tap modes are one filter over that line.  Every predicted block gets a class word
that says what it was and what it read; the counters (the generator's SG_R_IP_* definitions) are counted from the class words."""
import numpy as np

L, T, TL, TR = 1, 2, 4, 8            # an availability combination, as a block sees it
KIND_INTER, KIND_I4, KIND_I8, KIND_I16, KIND_PCM = range(5)   # the trace's macroblock kinds
SLOTS = ("4", "8", "16", "c")        # cell kinds: Intra4x4, Intra8x8, Intra16x16, chroma
NMODES = {"4": 9, "8": 9, "16": 4, "c": 4}


# ---- 6.4.3 / 6.4.5: inverse block scans, from the formula of 5.7 ----
def _inverse_raster_scan(a, b, c, d, e):
    return (a % (d // b)) * b if e == 0 else (a // (d // b)) * c


BLK4_XY = [(_inverse_raster_scan(i // 4, 8, 8, 16, 0) + _inverse_raster_scan(i % 4, 4, 4, 8, 0),
            _inverse_raster_scan(i // 4, 8, 8, 16, 1) + _inverse_raster_scan(i % 4, 4, 4, 8, 1)) for i in range(16)]
BLK8_XY = [(_inverse_raster_scan(i, 8, 8, 16, 0), _inverse_raster_scan(i, 8, 8, 16, 1)) for i in range(4)]
_IDX4_AT = {xy: i for i, xy in enumerate(BLK4_XY)}
_IDX8_AT = {xy: i for i, xy in enumerate(BLK8_XY)}


def _owner(xn, yn, size):
    """Table 6-3 (no MBAFF): the macroblock a location relative to the current macroblock's corner lies in: 'A', 'B', 'C', 'D', '' (the current one) or
    None (nowhere that can be there: right of the macroblock and not above it, or below it)"""
    if yn > size - 1:
        return None
    if xn < 0:
        return "D" if yn < 0 else "A"
    if xn > size - 1:
        return "C" if yn < 0 else None
    return "B" if yn < 0 else ""


def location_available(mb_there, xn, yn, size=16, unit=0, idx=0):
    """Is the sample at (xn, yn) relative to the current macroblock's corner available to block `idx` (unit 4 / 8: luma4x4BlkIdx / luma8x8BlkIdx; 0: the
    whole macroblock predicts at once)?  mb_there(letter) says whether neighbouring macroblock A / B / C / D may be predicted from."""
    who = _owner(xn, yn, size)
    if who is None:
        return False
    if who:
        return bool(mb_there(who))
    assert unit in (4, 8)
    other = (_IDX4_AT if unit == 4 else _IDX8_AT)[(xn // unit * unit, yn // unit * unit)]
    return other < idx            # a block of this macroblock with a greater index has not been decoded yet


def block_combination(mb_there, x0, y0, n, size=16, unit=0, idx=0):
    """the availability combination of the n x n block at (x0, y0) of the macroblock, with a check that the samples of one direction stand or fall together"""
    comb = 0
    for bit, ends in ((L, ((-1, 0), (-1, n - 1))), (T, ((0, -1), (n - 1, -1))), (TL, ((-1, -1),)), (TR, ((n, -1), (2 * n - 1, -1)))):
        got = {location_available(mb_there, x0 + dx, y0 + dy, size, unit, idx) for dx, dy in ends}
        assert len(got) == 1, "a direction half available"
        comb |= bit if got.pop() else 0
    return comb


# ---- which modes 8.3 allows, and which directions a mode reads (the clauses' "p[x, y] with ..." lists) ----
def mode_allowed(slot, mode, comb):
    if slot in ("4", "8"):
        need = {0: T, 1: L, 2: 0, 3: T, 4: L | T | TL, 5: L | T | TL, 6: L | T | TL, 7: T, 8: L}[mode]   # 3 / 7: the samples above right are substituted when absent
    elif slot == "16":
        need = {0: T, 1: L, 2: 0, 3: L | T | TL}[mode]
    else:
        need = {0: 0, 1: L, 2: T, 3: L | T | TL}[mode]
    return comb & need == need


def mode_reads(slot, mode, comb):
    """the directions whose samples the prediction is made of (DC: those that are there; Intra8x8: through the reference filter, which takes p[-1,-1] into
    p'[0,-1] and p'[-1,0], and p[8,-1] into p'[7,-1])"""
    if slot in ("4", "8"):
        r = {0: T, 1: L, 2: L | T, 3: T | TR, 4: L | T | TL, 5: L | T | TL, 6: L | T | TL, 7: T | TR, 8: L}[mode] & comb
        if slot == "8":
            r |= (TL | TR if r & T else 0) & comb
            r |= (TL if r & L else 0) & comb
        return r
    if slot == "16":
        return {0: T, 1: L, 2: L | T, 3: L | T | TL}[mode] & comb
    return {0: L | T, 1: L, 2: T, 3: L | T | TL}[mode] & comb


# ---- the class word of a predicted block ----
C_COMB_MASK = 15
C_MODE_SHIFT, C_SLOT_SHIFT = 4, 8
C_TR_REAL, C_TR_SUBST = 1 << 10, 1 << 11      # modes 3 / 7: the samples above right were there / were p[n-1,-1] repeated
C_F8_TOP_NO_TL, C_F8_LEFT_NO_TL = 1 << 12, 1 << 13
C_INTER_SHIFT, C_PCM_SHIFT = 14, 18           # four bits each: the direction's samples were read and lie in an inter / an I_PCM macroblock
C_IDX_SHIFT = 22


# ---- the line of neighbouring samples and the predictors ----
def _line(plane, X, Y, n, comb, ntop):
    """[p[-1,n-1] .. p[-1,0], p[-1,-1], p[0,-1] .. p[ntop-1,-1]] as int64; what is not available is 128 (never read by an allowed mode, except by DC, which asks)"""
    e = np.full(n + 1 + ntop, 128, dtype=np.int64)
    if comb & L:
        e[:n] = plane[Y:Y + n, X - 1][::-1]
    if comb & TL:
        e[n] = plane[Y - 1, X - 1]
    if comb & T:
        e[n + 1:n + 1 + n] = plane[Y - 1, X:X + n]
        if ntop > n:
            e[n + 1 + n:] = plane[Y - 1, X + n:X + 2 * n] if comb & TR else e[n + n]      # 8.3.1.2 / 8.3.2.2: p[n-1,-1] stands in
    return e


def _tap3(e):
    f = e.copy()
    f[1:-1] = (e[:-2] + 2 * e[1:-1] + e[2:] + 2) >> 2
    return f


def _filter_8x8(e, comb):
    """8.3.2.2.1 on the line of an 8x8 block (n = 8, sixteen samples above)"""
    n, f = 8, _tap3(e)
    out = e.copy()
    if comb & T:
        out[n + 1:] = f[n + 1:]
        out[n + 1] = f[n + 1] if comb & TL else (3 * e[n + 1] + e[n + 2] + 2) >> 2            # p'[0,-1]
        out[n + 16] = (e[n + 15] + 3 * e[n + 16] + 2) >> 2                                   # p'[15,-1]
    if comb & L:
        out[:n] = f[:n]
        out[n - 1] = f[n - 1] if comb & TL else (3 * e[n - 1] + e[n - 2] + 2) >> 2            # p'[-1,0]
        out[0] = (e[1] + 3 * e[0] + 2) >> 2                                                  # p'[-1,7]
    if comb & TL:
        if comb & T and comb & L:
            out[n] = f[n]
        elif comb & T:
            out[n] = (3 * e[n] + e[n + 1] + 2) >> 2
        elif comb & L:
            out[n] = (3 * e[n] + e[n - 1] + 2) >> 2
    return out


def _directional(e, n, mode, comb):
    """8.3.1.2.1 - 9 / 8.3.2.2.2 - 10 on the line e; t(k) = p[k,-1] (k = -1: the corner), l(k) = p[-1,k]"""
    f = _tap3(e)
    y, x = np.mgrid[0:n, 0:n]
    ti, li = (lambda k: n + 1 + k), (lambda k: n - 1 - k)
    if mode == 0:
        return e[ti(x)]
    if mode == 1:
        return e[li(y)]
    if mode == 2:
        st, sl = e[n + 1:n + 1 + n].sum(), e[:n].sum()
        sh = {4: 2, 8: 3}[n]
        if comb & T and comb & L:
            v = (st + sl + n) >> (sh + 1)
        elif comb & L:
            v = (sl + n // 2) >> sh
        elif comb & T:
            v = (st + n // 2) >> sh
        else:
            v = 128
        return np.full((n, n), v, dtype=np.int64)
    if mode == 3:
        out = f[ti(x + y + 1)]
        out[n - 1, n - 1] = (e[ti(2 * n - 2)] + 3 * e[ti(2 * n - 1)] + 2) >> 2
        return out
    if mode == 4:
        return f[n + x - y]
    if mode == 5:
        z, k = 2 * x - y, x - (y >> 1)
        even = (e[ti(np.maximum(k - 1, -1))] + e[ti(np.maximum(k, 0))] + 1) >> 1
        odd = f[ti(np.maximum(k - 1, -1))]
        far = f[li(np.clip(y - 2 * x - 2, 0, n - 2))]
        return np.where(z < -1, far, np.where(z == -1, f[n], np.where(z % 2 == 0, even, odd)))
    if mode == 6:
        z, k = 2 * y - x, y - (x >> 1)
        even = (e[li(np.maximum(k - 1, -1))] + e[li(np.maximum(k, 0))] + 1) >> 1
        odd = f[li(np.maximum(k - 1, -1))]
        far = f[ti(np.clip(x - 2 * y - 2, 0, n - 2))]
        return np.where(z < -1, far, np.where(z == -1, f[n], np.where(z % 2 == 0, even, odd)))
    if mode == 7:
        k = x + (y >> 1)
        return np.where(y % 2 == 0, (e[ti(k)] + e[ti(k + 1)] + 1) >> 1, f[ti(k + 1)])
    assert mode == 8
    z, k = x + 2 * y, y + (x >> 1)
    kk = np.minimum(k, n - 2)
    even, odd = (e[li(kk)] + e[li(kk + 1)] + 1) >> 1, f[li(np.minimum(k + 1, n - 2))]
    edge = (e[li(n - 2)] + 3 * e[li(n - 1)] + 2) >> 2
    return np.where(z > 2 * n - 3, e[li(n - 1)], np.where(z == 2 * n - 3, edge, np.where(z % 2 == 0, even, odd)))


def _plane(e, n, counts):
    """8.3.3.4 / 8.3.4.4 (4:2:0); counts[0] / counts[1] += samples below 0 / above 255 before Clip1"""
    h = n // 2
    k = np.arange(h)
    hh = ((k + 1) * (e[n + 1 + h + k] - e[n + 1 + h - 2 - k])).sum()
    vv = ((k + 1) * (e[n - 1 - h - k] - e[n - 1 - h + 2 + k])).sum()
    a = 16 * (e[0] + e[n + n])
    mul = 5 if n == 16 else 34
    b, c = (mul * hh + 32) >> 6, (mul * vv + 32) >> 6
    y, x = np.mgrid[0:n, 0:n]
    raw = (a + b * (x - (h - 1)) + c * (y - (h - 1)) + 16) >> 5
    counts[0] += int((raw < 0).sum())
    counts[1] += int((raw > 255).sum())
    return np.clip(raw, 0, 255)


def _dc16(e, comb):
    st, sl = e[17:33].sum(), e[:16].sum()
    if comb & T and comb & L:
        return (st + sl + 16) >> 5
    if comb & L:
        return (sl + 8) >> 4
    if comb & T:
        return (st + 8) >> 4
    return 128


def _chroma_dc(e, comb):
    """8.3.4.1 - 3: per 4x4 chroma block (xO, yO)"""
    out = np.empty((8, 8), dtype=np.int64)
    for yo in (0, 4):
        for xo in (0, 4):
            st, sl = e[9 + xo:13 + xo].sum(), e[4 - yo:8 - yo].sum()     # p[xO .. xO+3, -1], p[-1, yO .. yO+3]
            both = (st + sl + 4) >> 3
            top, left = (st + 2) >> 2, (sl + 2) >> 2
            if (xo, yo) in ((0, 0), (4, 4)):
                order = [(T | L, both), (T, top), (L, left)]
            elif yo == 0:       # xO > 0, yO = 0: the row above first
                order = [(T, top), (L, left)]
            else:               # xO = 0, yO > 0: the column to the left first
                order = [(L, left), (T, top)]
            out[yo:yo + 4, xo:xo + 4] = next((v for need, v in order if comb & need == need), 128)
    return out


# ---- counters (the names of streamgen.RANGE_NAMES) ----
COUNTERS = tuple("ip_av%s_m%d" % (s, m) for s in SLOTS for m in range(NMODES[s])) + tuple("ip_tr%d_b%d" % (k, b) for k, n in ((4, 16), (8, 4)) for b in range(n)) + (
    "ip_plane16_lo", "ip_plane16_hi", "ip_planec_lo", "ip_planec_hi", "ip_rec_luma_at0", "ip_rec_luma_at255", "ip_rec_chroma_at0", "ip_rec_chroma_at255",
    "ip_from_inter", "ip_from_pcm", "ip_f8_top_no_tl", "ip_f8_left_no_tl")
MASK_COUNTERS = tuple(c for c in COUNTERS if c.startswith(("ip_av", "ip_tr"))) + ("ip_from_inter", "ip_from_pcm")


def new_counters():
    return dict.fromkeys(COUNTERS, 0)


def count_class(c, cls):
    """one block's class word into the counters"""
    slot, mode, comb = SLOTS[(cls >> C_SLOT_SHIFT) & 3], (cls >> C_MODE_SHIFT) & 15, cls & C_COMB_MASK
    c["ip_av%s_m%d" % (slot, mode)] |= 1 << comb
    if cls & (C_TR_REAL | C_TR_SUBST):
        c["ip_tr%s_b%d" % (slot, cls >> C_IDX_SHIFT)] |= (1 if cls & C_TR_REAL else 0) | (2 if cls & C_TR_SUBST else 0)
    c["ip_f8_top_no_tl"] += bool(cls & C_F8_TOP_NO_TL)
    c["ip_f8_left_no_tl"] += bool(cls & C_F8_LEFT_NO_TL)
    c["ip_from_inter"] |= (cls >> C_INTER_SHIFT) & 15
    c["ip_from_pcm"] |= (cls >> C_PCM_SHIFT) & 15


def _class_word(slot, mode, comb, idx, kinds_of):
    """kinds_of(direction bit) -> the kind of the macroblock the direction's samples lie in, None for the current one"""
    cls = comb | mode << C_MODE_SHIFT | SLOTS.index(slot) << C_SLOT_SHIFT | idx << C_IDX_SHIFT
    if slot in ("4", "8") and mode in (3, 7):
        cls |= C_TR_REAL if comb & TR else C_TR_SUBST
    plain = mode_reads("4", mode, comb) if slot == "8" else 0
    if slot == "8" and not comb & TL:
        cls |= (C_F8_TOP_NO_TL if plain & T else 0) | (C_F8_LEFT_NO_TL if plain & L else 0)
    reads = mode_reads(slot, mode, comb)
    for i, bit in enumerate((L, T, TL, TR)):
        if reads & bit:
            k = kinds_of(bit)
            cls |= (1 << (C_INTER_SHIFT + i) if k == KIND_INTER else 0) | (1 << (C_PCM_SHIFT + i) if k == KIND_PCM else 0)
    return cls


def predict_picture(t, classes=None):
    """8.3 on one picture of streamgen.last_intra_trace(): every intra-predicted macroblock in address order, predicted from the picture's samples before
    the deblocking filter (t["planes"]) with the modes of t["ipmbs"].  Returns ((Y, Cb, Cr) prediction planes, 0 where nothing was intra-predicted;
    a mask per plane of the intra-predicted samples; counters).  The reconstruction clip is counted from the trace's residual, and prediction + residual,
    clipped, must be the picture's samples.  classes (a list) receives every block's class word."""
    mbs, mono, constrained = t["ipmbs"], bool(t["mono"]), bool(t["constrained_intra"])
    hmb, wmb = mbs.shape
    planes = [np.asarray(p).astype(np.int64) for p in t["planes"]]
    pred = [np.zeros(p.shape, dtype=np.int64) for p in planes]
    mask = [np.zeros(p.shape, dtype=bool) for p in planes]
    c = new_counters()
    offs = {"A": (-1, 0), "B": (0, -1), "C": (1, -1), "D": (-1, -1)}
    for my in range(hmb):
        for mx in range(wmb):
            cur = mbs[my, mx]
            if cur["kind"] not in (KIND_I4, KIND_I8, KIND_I16):
                continue
            addr = my * wmb + mx

            def nb(letter):
                x, y = mx + offs[letter][0], my + offs[letter][1]
                return mbs[y, x] if 0 <= x < wmb and 0 <= y < hmb else None

            def there(letter):
                m = nb(letter)
                if m is None or m["slice_id"] != cur["slice_id"] or (my + offs[letter][1]) * wmb + mx + offs[letter][0] > addr:
                    return False          # outside the picture, another slice, later in the slice
                return not (constrained and m["kind"] == KIND_INTER)

            def kinds_of_at(x0, y0, n, size):
                def f(bit):
                    dx, dy = {L: (-1, 0), T: (0, -1), TL: (-1, -1), TR: (n, -1)}[bit]
                    who = _owner(x0 + dx, y0 + dy, size)
                    return int(nb(who)["kind"]) if who else None
                return f

            def note(cls):
                count_class(c, cls)
                if classes is not None:
                    classes.append(cls)
            X, Y = 16 * mx, 16 * my
            if cur["kind"] == KIND_I16:
                comb, mode = block_combination(there, 0, 0, 16), int(cur["i16mode"])
                assert mode_allowed("16", mode, comb), ("Intra16x16 mode not allowed", mx, my, mode, comb)
                e = _line(planes[0], X, Y, 16, comb, 16)
                cnt = [0, 0]
                p = _plane(e, 16, cnt) if mode == 3 else (np.full((16, 16), _dc16(e, comb)) if mode == 2 else _directional(e, 16, mode, comb))
                c["ip_plane16_lo"] += cnt[0]
                c["ip_plane16_hi"] += cnt[1]
                pred[0][Y:Y + 16, X:X + 16] = p
                note(_class_word("16", mode, comb, 0, kinds_of_at(0, 0, 16, 16)))
            else:
                unit = 4 if cur["kind"] == KIND_I4 else 8
                slot = str(unit)
                for idx, (x0, y0) in enumerate(BLK4_XY if unit == 4 else BLK8_XY):
                    comb, mode = block_combination(there, x0, y0, unit, 16, unit, idx), int(cur["ipm"][(y0 // 4) * 4 + x0 // 4])
                    assert mode_allowed(slot, mode, comb), ("mode not allowed", mx, my, idx, mode, comb)
                    e = _line(planes[0], X + x0, Y + y0, unit, comb, 2 * unit)
                    if unit == 8:
                        e = _filter_8x8(e, comb)
                    pred[0][Y + y0:Y + y0 + unit, X + x0:X + x0 + unit] = _directional(e, unit, mode, comb)
                    note(_class_word(slot, mode, comb, idx, kinds_of_at(x0, y0, unit, 16)))
                    # the block's reconstruction is what the next block predicts from: it is in `planes` already (the picture before the filter)
            mask[0][Y:Y + 16, X:X + 16] = True
            if mono:
                continue
            comb, mode = block_combination(there, 0, 0, 8, size=8), int(cur["chroma_mode"])
            comb |= TR if there("C") else 0       # (chroma reads nothing there; the cell is the macroblock's neighbourhood)
            assert mode_allowed("c", mode, comb), ("chroma mode not allowed", mx, my, mode, comb)
            for pl in (1, 2):
                e = _line(planes[pl], 8 * mx, 8 * my, 8, comb, 8)
                cnt = [0, 0]
                p = _chroma_dc(e, comb) if mode == 0 else (_plane(e, 8, cnt) if mode == 3 else _directional(e, 8, {1: 1, 2: 0}[mode], comb))
                c["ip_planec_lo"] += cnt[0]
                c["ip_planec_hi"] += cnt[1]
                pred[pl][8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = p
                mask[pl][8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = True
            note(_class_word("c", mode, comb, 0, kinds_of_at(0, 0, 8, 8)))
    for pl in range(1 if mono else 3):
        raw = pred[pl] + np.asarray(t["res"][pl]).astype(np.int64)
        name = "ip_rec_luma" if pl == 0 else "ip_rec_chroma"
        c[name + "_at0"] += int((mask[pl] & (raw < 0)).sum())
        c[name + "_at255"] += int((mask[pl] & (raw > 255)).sum())
        bad = mask[pl] & (np.clip(raw, 0, 255) != planes[pl])
        assert not bad.any(), ("prediction + residual is not the picture", pl, np.argwhere(bad)[:4].tolist())
    return pred, mask, c


# ---- the cells that can be reached at all ----
def reachable_cells():
    """{(slot, mode, combination)}: all 16 neighbourhoods of a macroblock x every block position x the modes 8.3 allows there"""
    cells = set()
    for m in range(16):
        def there(letter, m=m):
            return bool(m & {"A": L, "B": T, "D": TL, "C": TR}[letter])
        combs = {"4": {block_combination(there, x, y, 4, 16, 4, i) for i, (x, y) in enumerate(BLK4_XY)},
                 "8": {block_combination(there, x, y, 8, 16, 8, i) for i, (x, y) in enumerate(BLK8_XY)},
                 "16": {block_combination(there, 0, 0, 16) & ~TR | (TR if there("C") else 0)},
                 "c": {block_combination(there, 0, 0, 8, size=8) & ~TR | (TR if there("C") else 0)}}
        for slot, cs in combs.items():
            cells |= {(slot, mode, cb) for cb in cs for mode in range(NMODES[slot]) if mode_allowed(slot, mode, cb)}
    return cells


def cells_of(r):
    """the cells in the counters r (streamgen.last_ranges() or predict_picture's)"""
    return {(s, m, cb) for s in SLOTS for m in range(NMODES[s]) for cb in range(16) if r["ip_av%s_m%d" % (s, m)] >> cb & 1}


def reachable_top_right():
    """{(slot, block index, 1 real / 2 substituted)}: what modes 3 and 7 can meet above and to the right, per block, over the 16 neighbourhoods"""
    out = set()
    for m in range(16):
        def there(letter, m=m):
            return bool(m & {"A": L, "B": T, "D": TL, "C": TR}[letter])
        for slot, unit, scan in (("4", 4, BLK4_XY), ("8", 8, BLK8_XY)):
            for i, (x, y) in enumerate(scan):
                cb = block_combination(there, x, y, unit, 16, unit, i)
                if cb & T:
                    out.add((slot, i, 1 if cb & TR else 2))
    return out


def merge(total, c):
    """the counters of one more picture into the total: bit masks are joined, counts added"""
    for k in COUNTERS:
        total[k] = total[k] | c[k] if k in MASK_COUNTERS else total[k] + c[k]
    return total


# ---- recipes of tests/test_intra_cells.py ----
# name -> generator parameters.  What each recipe must reach is in NEED below.  The conditions are not measurements: the seeds were chosen on the CPU until the
# generator alone met them, and the CPU test asserts them, so that a change to the generator cannot empty a recipe without a test failing.
_P = dict(idr_period=0, intra_stim=1)
CONTENT = {
    # constrained_intra_pred_flag 1 at about 50 % intra macroblocks: every one of the 16 neighbourhoods of a macroblock, made of inter neighbours
    "constrained_p_cabac": dict(_P, width=96, height=80, frames=8, profile_idc=77, cabac=1, constrained_intra=1, intra_in_p_permille=500, seed=1),
    "constrained_p_cavlc": dict(_P, width=96, height=80, frames=8, profile_idc=66, cabac=0, constrained_intra=1, intra_in_p_permille=500, seed=1),
    # the flag at 0: intra blocks predict from samples that K4 wrote and from I_PCM samples
    "k4_samples_pcm_cabac": dict(_P, width=96, height=80, frames=6, profile_idc=77, cabac=1, pcm_permille=120, intra_in_p_permille=450, seed=1),
    "k4_samples_pcm_cavlc_8x8": dict(_P, width=80, height=64, frames=6, profile_idc=100, cabac=0, transform8x8=1, pcm_permille=120, intra_in_p_permille=450, seed=1),
    # High profile: Intra8x8 with its reference filter, in every neighbourhood
    "high_8x8_constrained_cabac": dict(_P, width=96, height=80, frames=12, profile_idc=100, cabac=1, transform8x8=1, constrained_intra=1, intra_in_p_permille=500, seed=3),
    "high_8x8_constrained_cavlc": dict(_P, width=96, height=64, frames=12, profile_idc=100, cabac=0, transform8x8=1, constrained_intra=1, intra_in_p_permille=550, seed=6),
    # intra macroblocks of B pictures
    "b_intra_cabac": dict(_P, width=96, height=64, frames=7, profile_idc=77, cabac=1, bframes=2, num_ref_frames=3, constrained_intra=1, intra_in_p_permille=400, seed=1),
    # field pictures; PAFF with CABAC (the unpinned contexts: rangeutil.decoder_cfg)
    "field_cavlc": dict(_P, width=96, height=64, frames=4, profile_idc=77, cabac=0, field_pics=1, num_ref_frames=2, constrained_intra=1, intra_in_p_permille=450, seed=1),
    "paff_cabac_8x8": dict(_P, width=64, height=64, frames=5, profile_idc=100, cabac=1, transform8x8=1, field_pics=3, num_ref_frames=2, intra_in_p_permille=400, seed=1),
    "mono_cabac_8x8": dict(_P, width=64, height=48, frames=5, profile_idc=100, cabac=1, mono=1, transform8x8=1, constrained_intra=1, intra_in_p_permille=450, seed=1),
    # two slice groups dispersed (a checkerboard): the macroblocks above left and above right without the ones above and to the left
    "fmo_checkerboard_cavlc": dict(_P, width=96, height=80, frames=5, profile_idc=66, cabac=0, slice_groups=2, fmo_type=1, intra_in_p_permille=300, seed=1),
    # an explicit map, the slices in arbitrary order
    "fmo_explicit_aso_cavlc": dict(_P, width=96, height=80, frames=5, profile_idc=66, cabac=0, slice_groups=3, fmo_type=6, slices=2, aso=1, constrained_intra=1,
                                   intra_in_p_permille=400, seed=1),
    # three slices on five macroblock columns start in the middle of a row: above right without above, above and left without above left
    "slices3_midrow_cabac": dict(width=80, height=80, frames=4, idr_period=2, intra_stim=1, profile_idc=77, cabac=1, slices=3, intra_in_p_permille=400, seed=1),
    "slices3_midrow_cavlc_8x8": dict(width=80, height=64, frames=12, idr_period=1, intra_stim=1, profile_idc=100, cabac=0, transform8x8=1, slices=3, seed=1),
    # 0 / 255 content: the plane predictors and prediction + residual leave 0 .. 255 at both ends
    "contrast_cabac_8x8": dict(_P, width=64, height=48, frames=5, profile_idc=100, cabac=1, transform8x8=1, contrast=1, qp=30, intra_in_p_permille=500, seed=1),
    "contrast_cavlc": dict(width=64, height=64, frames=4, idr_period=1, intra_stim=1, profile_idc=66, cabac=0, contrast=1, qp=24, seed=1),
}
# what K3's schedules distinguish: one macroblock; one row; 17 rows (more than the wavefronts of k_intra, several bands of k_intra_x); 65 columns x 5 rows (the row
# above a macroblock straddles a chunk of 64 columns, two bands).  Each as an intra-only stream and as a P stream with constrained_intra_pred_flag 0
_GI = dict(frames=2, idr_period=1, intra_stim=1, profile_idc=77, cabac=1, seed=1)
_GP = dict(frames=4, idr_period=0, intra_stim=1, profile_idc=77, cabac=0, intra_in_p_permille=400, pcm_permille=30, seed=1)
GEOMETRY = {
    "geo_16x16_i": dict(_GI, width=16, height=16), "geo_16x16_p": dict(_GP, width=16, height=16, frames=6, seed=9),
    "geo_272x16_i": dict(_GI, width=272, height=16), "geo_272x16_p": dict(_GP, width=272, height=16),
    "geo_16x272_i": dict(_GI, width=16, height=272), "geo_16x272_p": dict(_GP, width=16, height=272),
    "geo_1040x80_i": dict(_GI, width=1040, height=80, profile_idc=100, transform8x8=1),
    "geo_1040x80_p150": dict(_GP, width=1040, height=80, intra_in_p_permille=150, seed=12),
    "geo_1040x80_p500": dict(_GP, width=1040, height=80, intra_in_p_permille=500, profile_idc=100, transform8x8=1, cabac=1, seed=4),
}
RECIPES = dict(CONTENT, **GEOMETRY)


def pictures_of(kw):
    return kw["frames"] * (2 if kw.get("field_pics") else 1)


# What every recipe must reach, as the seeds above reach it: (the availability masks ip_av* in the order of COUNTERS, four hex digits each; ip_tr* one hex
# digit each; the directions of ip_from_inter and of ip_from_pcm; the counting counters that must be above 0).  A recipe may reach more.
NEED = {
    "constrained_p_cabac": ("cc80 8aa2 ceb3 c480 8080 8080 8080 c480 8aa2 0000 0000 0000 0000 0000 0000 0000 0000 0000 c4c4 a2aa 85ff 8080 ffff a2aa c4cc 8080",
        "11121312111212120000", 0, 0, ()),
    "constrained_p_cavlc": ("cc80 8aa2 ceb3 c480 8080 8080 8080 c480 8aa2 0000 0000 0000 0000 0000 0000 0000 0000 0000 c4c4 a2aa 85ff 8080 ffff a2aa c4cc 8080",
        "11121312111212120000", 0, 0, ()),
    "k4_samples_pcm_cabac": ("8480 8082 8483 8480 8080 8080 8080 8480 8082 0000 0000 0000 0000 0000 0000 0000 0000 0000 8480 8082 8482 8080 8483 8082 8480 8080",
        "11121312111212120000", 15, 15, ()),
    "k4_samples_pcm_cavlc_8x8": ("8480 8082 8483 8480 8080 8080 8080 8480 8082 8480 8082 8483 8480 8080 8080 8080 8480 8082 8400 8082 8483 8080 8483 8082 8480 8080",
        "11121112111212121312", 15, 15, ("f8_top_no_tl", "f8_left_no_tl")),
    "high_8x8_constrained_cabac": ("c480 8aa2 ceb3 cc80 8080 8080 8080 c480 82a2 cc80 8aa2 ceb3 cc80 8080 8080 8080 cc80 8aa2 cccc a02a fddf 8080 fdff a8aa cccc 8080",
        "11121312111212121312", 0, 0, ("f8_top_no_tl", "f8_left_no_tl")),
    "high_8x8_constrained_cavlc": ("cc80 8aa2 ceb3 c480 8080 8080 8080 cc80 8aa2 cc80 82a2 ceb3 c480 8080 8080 8080 c480 8aa2 cccc a8aa fdc7 8080 ffff aaaa cccc 8080",
        "11121312111212121312", 0, 0, ("f8_top_no_tl", "f8_left_no_tl")),
    "b_intra_cabac": ("c480 8a82 ceb3 c480 8080 8080 8080 c480 8282 0000 0000 0000 0000 0000 0000 0000 0000 0000 844c 8aa2 8b3b 8080 dfff 8aaa cc4c 8080",
        "11121312111212120000", 0, 0, ()),
    "field_cavlc": ("c480 8082 c483 8480 8080 8080 8080 8480 8082 0000 0000 0000 0000 0000 0000 0000 0000 0000 4040 8022 0567 8080 c167 8022 c444 8080",
        "01120012111212120000", 0, 0, ()),
    "paff_cabac_8x8": ("8080 8082 8082 8080 8080 8080 8080 8080 8082 8480 8082 8483 8480 8080 8080 8080 8480 8082 8400 8002 8403 8000 8483 8082 8480 8080",
        "11121212011212121012", 15, 0, ("f8_top_no_tl", "f8_left_no_tl")),
    "mono_cabac_8x8": ("8480 8082 8483 8480 8080 8080 8080 8480 8082 0480 8082 8483 4480 0080 0080 8080 8480 8082 0400 0002 0503 8000 0000 0000 0000 0000",
        "11121012111212121012", 0, 0, ("f8_top_no_tl", "f8_left_no_tl")),
    "fmo_checkerboard_cavlc": ("8480 8282 8693 8480 8080 8080 8080 8480 8282 0000 0000 0000 0000 0000 0000 0000 0000 0000 0000 0000 1111 0000 1111 0000 0000 0000",
        "00120012111212120000", 0, 0, ()),
    "fmo_explicit_aso_cavlc": ("8480 82a2 8ea3 c480 8080 8080 8080 8480 8282 0000 0000 0000 0000 0000 0000 0000 0000 0000 0044 0002 0373 8080 2377 0a22 4044 8080",
        "11120112111212120000", 0, 0, ()),
    "slices3_midrow_cabac": ("8480 8a82 8e83 8c80 8080 8080 8080 8c80 8282 0000 0000 0000 0000 0000 0000 0000 0000 0000 8480 8a82 8f03 8080 8f83 8a82 8c80 8080",
        "11121112111212120000", 15, 0, ()),
    "slices3_midrow_cavlc_8x8": ("8c80 8282 8e83 8c80 8080 8080 8080 8c80 8a82 8c80 8a82 8e83 8c80 8080 8080 8080 8c80 8a82 0c00 0a82 0f83 0080 8f83 8a82 8c80 8080",
        "11121312111212121312", 0, 0, ("f8_top_no_tl", "f8_left_no_tl")),
    "contrast_cabac_8x8": ("8480 8082 8482 8480 8080 8080 8080 8480 8082 8480 8082 8483 8480 8080 8080 8080 8480 8082 8480 8082 8482 8000 8483 8082 8480 8080",
        "11121112111212121312", 15, 0, ("plane16_lo", "planec_lo", "planec_hi", "rec_luma_at0", "rec_luma_at255", "rec_chroma_at0", "rec_chroma_at255", "f8_top_no_tl", "f8_left_no_tl")),
    "contrast_cavlc": ("8480 8082 8483 8480 8080 8080 8080 8480 8082 0000 0000 0000 0000 0000 0000 0000 0000 0000 8480 8082 8483 8080 8483 8082 8480 8080",
        "11121112111212120000", 0, 0, ("plane16_lo", "plane16_hi", "planec_lo", "planec_hi", "rec_luma_at0", "rec_luma_at255", "rec_chroma_at0", "rec_chroma_at255")),
    "geo_16x16_i": ("8480 8082 8483 8480 8080 8080 0080 8480 8082 0000 0000 0000 0000 0000 0000 0000 0000 0000 0000 0000 0000 0000 0001 0000 0000 0000",
        "00100010001212000000", 0, 0, ()),
    "geo_16x16_p": ("8480 8082 8483 8480 8080 8080 8080 8480 8082 0000 0000 0000 0000 0000 0000 0000 0000 0000 0000 0000 0001 0000 0001 0000 0000 0000",
        "00100010011212020000", 0, 0, ()),
    "geo_272x16_i": ("8480 8082 8483 8480 8080 8080 8080 8480 8082 0000 0000 0000 0000 0000 0000 0000 0000 0000 0000 0002 0002 0000 0003 0002 0000 0000",
        "00120012111212120000", 0, 0, ()),
    "geo_272x16_p": ("8480 8082 8483 8080 8080 8080 8080 8480 8082 0000 0000 0000 0000 0000 0000 0000 0000 0000 0000 0002 0003 0000 0003 0002 0000 0000",
        "00120012111212120000", 5, 0, ()),
    "geo_16x272_i": ("8480 8082 8483 8480 8080 8080 8080 8480 8082 0000 0000 0000 0000 0000 0000 0000 0000 0000 0004 0000 0004 0000 0005 0000 0004 0000",
        "11121212111212120000", 0, 0, ()),
    "geo_16x272_p": ("8480 8082 8483 8480 8080 8080 8080 8480 8082 0000 0000 0000 0000 0000 0000 0000 0000 0000 0004 0000 0004 0000 0005 0000 0004 0000",
        "11121212111212120000", 14, 6, ()),
    "geo_1040x80_i": ("8480 8082 8483 8480 8080 8080 8080 8480 8082 8480 8082 8483 8480 8080 8080 8080 8480 8082 8480 8082 8482 8080 8483 8082 8480 8080",
        "11121112111212121312", 0, 0, ("f8_top_no_tl", "f8_left_no_tl")),
    "geo_1040x80_p150": ("8480 8082 8483 8480 8080 8080 8080 8480 8082 0000 0000 0000 0000 0000 0000 0000 0000 0000 8480 8082 8482 8080 8483 8082 8480 8080",
        "11121112111212120000", 15, 15, ()),
    "geo_1040x80_p500": ("8480 8082 8483 8480 8080 8080 8080 8480 8082 8480 8082 8483 8480 8080 8080 8080 8480 8082 8480 8082 8403 8080 8483 8082 8480 8080",
        "11121312111212121312", 15, 15, ("f8_top_no_tl", "f8_left_no_tl")),
}
_AV = tuple(c for c in COUNTERS if c.startswith("ip_av"))
_TR = tuple(c for c in COUNTERS if c.startswith("ip_tr"))
_COUNTING = tuple(c for c in COUNTERS if c not in MASK_COUNTERS)


def counter_line(name, r):
    """a recipe's intra counters as one line of tests/golden/intra_counters.txt"""
    av = " ".join("%s=%s" % (s, ",".join("%04x" % r["ip_av%s_m%d" % (s, m)] for m in range(NMODES[s]))) for s in SLOTS)
    tr = "tr4=%s tr8=%s" % ("".join("%x" % r["ip_tr4_b%d" % b] for b in range(16)), "".join("%x" % r["ip_tr8_b%d" % b] for b in range(4)))
    rest = " ".join("%s=%d" % (k[3:], r[k]) for k in COUNTERS if not k.startswith(("ip_av", "ip_tr")))
    return "  %-28s cells=%d %s %s %s" % (name, len(cells_of(r)), av, tr, rest)


def needed(name):
    """the conditions of a recipe as counters: bit masks that must be contained in the recipe's, 1 for a counter that must be above 0"""
    av, tr, inter, pcm, counting = NEED[name]
    need = dict(zip(_AV, (int(w, 16) for w in av.split())))
    need.update(zip(_TR, (int(d, 16) for d in tr)))
    need.update(ip_from_inter=inter, ip_from_pcm=pcm)
    need.update(("ip_" + k, 1) for k in counting)
    return need


def unmet(name, r):
    """The conditions of recipe `name` that the counters r = streamgen.last_ranges() do not meet (an empty list: all met)."""
    bad = []
    for k, v in needed(name).items():
        if k in MASK_COUNTERS:
            if v & ~r[k]:
                bad.append("%s: bits %#x of %#x missing" % (k, v & ~r[k], v))
        elif r[k] <= 0:
            bad.append(k)
    return bad


def required_somewhere():
    """what no recipe asks for, of: every reachable cell, every reachable state of the samples above right per block, every direction of foreign samples,
    every counting counter (an empty list: everything is asked for by at least one recipe)"""
    total = new_counters()
    for name in RECIPES:
        merge(total, dict(new_counters(), **needed(name)))
    missing = sorted(reachable_cells() - cells_of(total))
    missing += sorted(("top right",) + t for t in reachable_top_right() if not total["ip_tr%s_b%d" % (t[0], t[1])] & t[2])
    missing += [k for k in ("ip_from_inter", "ip_from_pcm") if total[k] != 15] + [k for k in _COUNTING if not total[k]]
    return missing


def required_beyond_reach():
    """cells a recipe asks for that the enumeration says cannot be reached (an empty list)"""
    extra = []
    for name in RECIPES:
        extra += sorted(cells_of(dict(new_counters(), **needed(name))) - reachable_cells())
    return extra
