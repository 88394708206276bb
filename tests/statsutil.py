"""The yardstick of K12: the contract "Frame statistics" of include/h264mi.h in numpy on int64, written from the header's text (not from the kernel).

A frame is a tight I420 array (what h264mi_frame_read(crop = 1) returns): h x w luma, then Cb and Cr of ceil(h / 2) x ceil(w / 2) each.  The statistics of
an item are a function of the source's frame S, a predecessor's frame P of the same size or None, a cell size and a threshold, and of nothing else."""
import struct

import numpy as np

CELL_SUM, CELL_SAD = 1, 2
PREV_NONE, PREV_HISTORY = -1, -2
RECORD_BYTES = 1120
U64 = ("sum_y", "sum_y2", "sum_cb", "sum_cr", "sad_y", "sse_y", "sad_cb", "sad_cr")
U32 = ("min_y", "max_y", "changed_y", "has_prev", "w", "h", "gw", "gh")
CELLS = (8, 16, 32, 64)
MAX_AXIS = 16384  # H264MI_SCALE_MAX


def planes(f, w, h):
    """(Y, Cb, Cr) of a tight I420 frame, as int64."""
    wc, hc = (w + 1) // 2, (h + 1) // 2
    f = np.asarray(f).astype(np.int64)
    assert f.size == w * h + 2 * wc * hc
    return f[:w * h].reshape(h, w), f[w * h:w * h + wc * hc].reshape(hc, wc), f[w * h + wc * hc:].reshape(hc, wc)


def spec_ok(cell, planes_, thresh=0, flags=0):
    return ((cell in CELLS and planes_ in (1, 2, 3)) or (cell == 0 and planes_ == 0)) and 0 <= thresh <= 255 and flags == 0


def grid_size(w, h, cell):
    return (0, 0) if cell == 0 else (-(-w // cell), -(-h // cell))


def item_bytes(w, h, cell=0, planes_=0):
    """Bytes of one item, or None where h264mi_stats_size refuses."""
    if not spec_ok(cell, planes_) or not (1 <= w <= MAX_AXIS and 1 <= h <= MAX_AXIS):
        return None
    gw, gh = grid_size(w, h, cell)
    return RECORD_BYTES + (4 * gw * gh * bin(planes_).count("1") + 15) // 16 * 16


def record(S, P, w, h, thresh):
    """The scalar fields and hist_y of the record (gw, gh are the grid's: the caller's)."""
    y, cb, cr = planes(S, w, h)
    r = dict(sum_y=int(y.sum()), sum_y2=int((y * y).sum()), sum_cb=int(cb.sum()), sum_cr=int(cr.sum()), sad_y=0, sse_y=0, sad_cb=0, sad_cr=0,
             min_y=int(y.min()), max_y=int(y.max()), changed_y=0, has_prev=0, w=w, h=h)
    if P is not None:
        py, pcb, pcr = planes(P, w, h)
        d = np.abs(y - py)
        r.update(sad_y=int(d.sum()), sse_y=int((d * d).sum()), sad_cb=int(np.abs(cb - pcb).sum()), sad_cr=int(np.abs(cr - pcr).sum()),
                 changed_y=int((d > thresh).sum()), has_prev=1)
    r["hist_y"] = np.bincount(y.reshape(-1), minlength=256).astype(np.int64)
    return r


def grid(S, P, w, h, cell):
    """(CELL_SUM plane, CELL_SAD plane), each int64 [gh, gw]: cell (j, i) covers display luma rows j * cell .. and columns i * cell .., partial at the edges."""
    gw, gh = grid_size(w, h, cell)
    y = planes(S, w, h)[0]
    d = np.abs(y - planes(P, w, h)[0]) if P is not None else np.zeros_like(y)
    out = []
    for a in (y, d):
        pad = np.zeros((gh * cell, gw * cell), np.int64)
        pad[:h, :w] = a
        out.append(pad.reshape(gh, cell, gw, cell).sum(axis=(1, 3)))
    return out[0], out[1]


def item(S, P, w, h, cell=0, planes_=0, thresh=0):
    """The bytes of one item as the device writes them: the record, the selected planes in ascending bit order, zeros up to a multiple of 16."""
    r = record(S, P, w, h, thresh)
    gw, gh = grid_size(w, h, cell)
    r.update(gw=gw, gh=gh)
    buf = struct.pack("<8Q8I", *([r[k] for k in U64] + [r[k] for k in U32])) + r["hist_y"].astype("<u4").tobytes()
    if cell:
        both = grid(S, P, w, h, cell)
        for bit in (0, 1):
            if planes_ >> bit & 1:
                buf += both[bit].astype("<u4").tobytes()
    buf += bytes(-len(buf) % 16)
    assert len(buf) == item_bytes(w, h, cell, planes_)
    return np.frombuffer(buf, np.uint8)


def parse(buf, planes_=0):
    """A record (and the planes behind it) from the bytes of one item: a dict of ints, hist_y and the planes as int64 arrays."""
    buf = bytes(bytearray(buf))
    v = struct.unpack_from("<8Q8I", buf, 0)
    r = dict(zip(U64 + U32, v))
    r["hist_y"] = np.frombuffer(buf, "<u4", 256, 96).astype(np.int64)
    at, n = RECORD_BYTES, r["gw"] * r["gh"]
    for bit, name in ((0, "cell_sum"), (1, "cell_sad")):
        if planes_ >> bit & 1:
            r[name] = np.frombuffer(buf, "<u4", n, at).astype(np.int64).reshape(r["gh"], r["gw"])
            at += 4 * n
    return r


def check_invariants(r, planes_=0):
    """The invariants the contract states, on a parsed item."""
    hist = r["hist_y"]
    assert hist.sum() == r["w"] * r["h"]
    assert (np.arange(256) * hist).sum() == r["sum_y"]
    nz = np.flatnonzero(hist)
    assert (nz[0], nz[-1]) == (r["min_y"], r["max_y"])
    if planes_ & CELL_SUM:
        assert r["cell_sum"].sum() == r["sum_y"]
    if planes_ & CELL_SAD:
        assert r["cell_sad"].sum() == r["sad_y"]
    if not r["has_prev"]:
        assert all(r[k] == 0 for k in ("sad_y", "sse_y", "sad_cb", "sad_cr", "changed_y"))
    assert all(r[k] < 1 << 46 for k in U64) and all(r[k] < 1 << 31 for k in U32) and hist.max() < 1 << 31
