"""The yardstick of the side-information planes (K11): the contract of include/h264mi.h, "Macroblock side information", in numpy.

Inputs: the bytes h264mi_frame_read_mbrecs / h264mi_frame_read_mbmv1 return, parsed by the offsets of mi_types.h (the ones mbtype.SliceData uses); the frame's
crop origin and display size; and the picture order counts of the reference lists per slice, passed in as plain arrays.  It shares no code with the kernel
or with the host's table."""
import numpy as np

NAMES = ("type", "qp", "nz", "slice", "mvx0", "mvy0", "ref0", "dpoc0", "mvx1", "mvy1", "ref1", "dpoc1")
BIT = {n: 1 << i for i, n in enumerate(NAMES)}
ALL = 0xFFF
SCALE_MAX = 16384
MB_NONE, MB_IPCM, MB_P16x16, MB_P8x8, MB_PSKIP, MB_B = 0, 4, 5, 8, 9, 10
# MbRec (128 bytes): type 0, qp 2, nzmask 8 (u16), slice_in_pic 14 (u16), ipm 16 (inter: [0..3] ref_idx_l1), ref_idx_l0 32 (4 x i8), refslot 36 (4 x i16),
# mv 48 (16 x 2 x i16), refslot1 120 (4 x i16)


def planes_of(bits):
    return [n for n in NAMES if bits & BIT[n]]


def size(bits, w, h):
    """(gw, gh, bytes) or None where h264mi_side_size refuses."""
    if bits <= 0 or bits & ~ALL or not (1 <= w <= SCALE_MAX and 1 <= h <= SCALE_MAX):
        return None
    gw, gh = (w + 3) // 4, (h + 3) // 4
    return gw, gh, 2 * gw * gh * len(planes_of(bits))


def clamp16(v):
    return max(-32768, min(32767, int(v)))


def mb_planes(recs, mv1, wmb, hmb, slice_pocs):
    """All twelve planes over the whole coded picture: int16 [12, 4 hmb, 4 wmb].
    recs: uint8 [n, 128]; mv1: int16 [n, 16, 2] or None; slice_pocs: {slice ordinal in the picture (MbRec::slice_in_pic; -1: concealed): (cur_poc, [pocs of list 0], [pocs of list 1])}."""
    recs = np.asarray(recs, np.uint8).reshape(wmb * hmb, 128)
    out = np.zeros((12, 4 * hmb, 4 * wmb), np.int16)
    out[[6, 10]] = -1
    for m in range(wmb * hmb):
        r = recs[m]
        t = int(r[0])
        ys, xs = slice(4 * (m // wmb), 4 * (m // wmb) + 4), slice(4 * (m % wmb), 4 * (m % wmb) + 4)
        out[0, ys, xs] = t
        out[1, ys, xs] = int(r[2])
        nz = int(r[8]) | int(r[9]) << 8
        out[2, ys, xs] = np.array([(nz >> k) & 1 for k in range(16)], np.int16).reshape(4, 4)
        out[3, ys, xs] = -1 if t == MB_NONE else int(r[14:16].view(np.int16)[0])
        if t < MB_P16x16:
            continue  # intra and not delivered: vectors 0, references -1, distances 0
        cur, l0, l1 = slice_pocs.get(int(r[14:16].view(np.int16)[0]), (0, [], []))
        lists = ((r[36:44].view(np.int16), r[32:36].view(np.int8), r[48:112].view(np.int16).reshape(16, 2), l0, 4),
                 (r[120:128].view(np.int16), r[16:20].view(np.int8), None if mv1 is None else np.asarray(mv1[m]).reshape(16, 2), l1, 8))
        for slots, refs, mv, pocs, base in lists:
            for q in range(4):
                if int(slots[q]) < 0:
                    continue
                qy, qx = slice(ys.start + 2 * (q >> 1), ys.start + 2 * (q >> 1) + 2), slice(xs.start + 2 * (q & 1), xs.start + 2 * (q & 1) + 2)
                ref = int(refs[q])
                for by in range(2):
                    for bx in range(2):
                        blk = (2 * (q >> 1) + by) * 4 + 2 * (q & 1) + bx
                        if mv is not None:
                            out[base, qy.start + by, qx.start + bx] = mv[blk][0]
                            out[base + 1, qy.start + by, qx.start + bx] = mv[blk][1]
                out[base + 2, qy, qx] = ref
                out[base + 3, qy, qx] = clamp16(pocs[ref] - cur) if 0 <= ref < len(pocs) else 0
    return out


def frame(recs, mv1, wmb, hmb, crop_x, crop_y, w, h, slice_pocs, bits=ALL):
    """The selected planes of one frame: int16 [C, gh, gw], cell (j, i) = coded block ((crop_x >> 2) + i, (crop_y >> 2) + j)."""
    gw, gh, _ = size(bits, w, h)
    full = mb_planes(recs, mv1, wmb, hmb, slice_pocs)
    bx0, by0 = crop_x >> 2, crop_y >> 2
    assert bx0 + gw <= 4 * wmb and by0 + gh <= 4 * hmb, "every cell lies inside the coded picture"
    sel = [i for i, n in enumerate(NAMES) if bits & BIT[n]]
    return np.ascontiguousarray(full[sel, by0:by0 + gh, bx0:bx0 + gw])
