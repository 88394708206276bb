"""The yardstick of the JPEG snapshots (K13): a numpy / pure-Python baseline JPEG encoder written from the text of include/h264mi.h ("JPEG snapshots"),
not from the kernel: the quantisation tables, the integer block rule, the range rule, the entropy coding, the restart intervals and the file structure.
The Annex K.3.3 Huffman tables are not typed in a second time: they are read out of a file that Pillow (libjpeg) writes, which carries the same four
tables -- a third party's copy.  `Counters` records what a set of inputs exercised, so that a test can assert that its set is not a tame one."""
import io
import math

import numpy as np

RANGE_AUTO, RANGE_KEEP, RANGE_FULL = 0, 1, 2
TRUNCATED = 1

# Annex K.1, tables K.1 (luminance) and K.2 (chrominance), row by row
BASE = (
    [16, 11, 10, 16, 24, 40, 51, 61,
     12, 12, 14, 19, 26, 58, 60, 55,
     14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77,
     24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101,
     72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99,
     18, 21, 26, 66, 99, 99, 99, 99,
     24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32,
)


def zigzag():
    """Natural index (8 * row + column) of every zigzag position, by walking the anti-diagonals."""
    order = []
    for s in range(15):
        cells = [(y, s - y) for y in range(8) if 0 <= s - y < 8]
        order += [8 * y + x for y, x in (cells if s % 2 else cells[::-1])]
    return order


ZZ = zigzag()


def quant_table(quality, chroma):
    sc = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.array([min(max((b * sc + 50) // 100, 1), 255) for b in BASE[chroma]], dtype=np.int64)


def dct_matrix():
    return np.array([[int(np.rint(16384 * (math.sqrt(1 / 8) if k == 0 else 0.5) * math.cos((2 * n + 1) * k * math.pi / 16))) for n in range(8)] for k in range(8)],
                    dtype=np.int64)


M = dct_matrix()


def block_levels(blocks, q):
    """The block rule: blocks [..., 8, 8] of samples, q [64] in natural order -> levels [..., 8, 8] (int64)."""
    x = np.asarray(blocks, dtype=np.int64) - 128
    r = (x @ M.T + 128) >> 8                      # r[y][k] = (sum_n M[k][n] x[y][n] + 128) >> 8
    c = M @ r                                     # c[v][k] = sum_y M[v][y] r[y][k]
    assert np.abs(c).max(initial=0) < 2 ** 31 - (255 << 19)
    qq = np.asarray(q, dtype=np.int64).reshape(8, 8)
    return np.sign(c) * ((np.abs(c) + (qq << 19)) // (qq << 20))


def full_range(plane, chroma):
    p = plane.astype(np.int64)
    if not chroma:
        return ((255 * (np.clip(p, 16, 235) - 16) + 109) // 219).astype(np.uint8)
    c = np.clip(p, 16, 240) - 128
    m = (255 * np.abs(c) + 112) // 224
    return np.clip(np.where(c < 0, 128 - m, 128 + m), 0, 255).astype(np.uint8)


_HUFF = None


def huffman_tables():
    """{(ac, table): (bits[16], values)} of Annex K.3.3, as Pillow writes them into a non-optimised 4:2:0 file."""
    global _HUFF
    if _HUFF is None:
        from PIL import Image
        f = io.BytesIO()
        Image.new("RGB", (16, 16), (90, 30, 200)).save(f, "JPEG", quality=75, subsampling=2, optimize=False)
        _HUFF = {}
        for marker, body in segments(f.getvalue()):
            at = 0
            while marker == 0xC4 and at < len(body):
                tc_th, bits = body[at], list(body[at + 1:at + 17])
                n = sum(bits)
                _HUFF[(tc_th >> 4, tc_th & 15)] = (bits, list(body[at + 17:at + 17 + n]))
                at += 17 + n
        assert sorted(_HUFF) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    return _HUFF


def huffman_codes(ac, table):
    """{symbol: (code, length)} by Annex C.2."""
    bits, vals = huffman_tables()[(ac, table)]
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


def segments(data):
    """(marker, body) of the segments of a JPEG file up to and including SOS; (0xDA, body) is followed by nothing."""
    assert data[:2] == b"\xff\xd8"
    at, out = 2, []
    while at < len(data):
        assert data[at] == 0xFF, at
        marker, n = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        out.append((marker, data[at + 4:at + 2 + n]))
        at += 2 + n
        if marker == 0xDA:
            break
    return out


def header(w, h, mono, quality, restart):
    """SOI .. SOS."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)
    nc = 1 if mono else 3
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(1 if mono else 2):
        q = quant_table(quality, t)
        out += seg(0xDB, bytes([t]) + bytes(int(q[ZZ[z]]) for z in range(64)))
    comps = [(1, 0x11 if mono else 0x22, 0)] + ([] if mono else [(2, 0x11, 1), (3, 0x11, 1)])
    out += seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc]) + bytes(v for c in comps for v in c))
    for t in range(1 if mono else 2):
        for ac in range(2):
            bits, vals = huffman_tables()[(ac, t)]
            out += seg(0xC4, bytes([ac << 4 | t]) + bytes(bits) + bytes(vals))
    out += seg(0xDD, restart.to_bytes(2, "big"))
    out += seg(0xDA, bytes([nc]) + bytes(v for c in comps for v in (c[0], c[2] << 4 | c[2])) + bytes([0, 63, 0]))
    return out


class Counters:
    def __init__(self):
        self.zrl = self.stuffed = self.max_dc_cat = self.max_ac_cat = self.no_eob = self.eob_only = self.pad_ff = self.intervals = 0

    def all_nonzero(self):
        return all(v > 0 for v in vars(self).values())


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        assert 0 <= code < (1 << length)
        self.acc, self.n = self.acc << length | code, self.n + length


def _category(v):
    return int(abs(int(v))).bit_length()


def _magnitude(v, s):
    v = int(v)
    return (v if v >= 0 else v - 1) & ((1 << s) - 1)


def planes_of(i420, w, h, mono):
    a = np.frombuffer(bytes(i420), dtype=np.uint8) if not isinstance(i420, np.ndarray) else i420.reshape(-1)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    y = a[:w * h].reshape(h, w)
    if mono:
        return [y]
    return [y, a[w * h:w * h + cw * ch].reshape(ch, cw), a[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)]


def encode(i420, w, h, mono=False, quality=90, full=False, restart_mcus=0, counters=None):
    """The file of one tight I420 frame (luma only is read for mono)."""
    k = counters if counters is not None else Counters()
    planes = planes_of(i420, w, h, mono)
    if full:
        planes = [full_range(p, i > 0) for i, p in enumerate(planes)]
    mcu = 8 if mono else 16
    mw, mh = -(-w // mcu), -(-h // mcu)
    levels = []
    for i, p in enumerate(planes):
        unit = mcu if i == 0 else 8
        p = np.pad(p, ((0, mh * unit - p.shape[0]), (0, mw * unit - p.shape[1])), mode="edge")  # the last row / column, replicated, per plane
        b = p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).swapaxes(1, 2)
        levels.append(block_levels(b, quant_table(quality, int(i > 0))).reshape(b.shape[0], b.shape[1], 64)[:, :, ZZ])
    dc = [huffman_codes(0, 0), huffman_codes(0, 1)]
    ac = [huffman_codes(1, 0), huffman_codes(1, 1)]
    restart = restart_mcus if restart_mcus else mw
    n_mcus = mw * mh
    n_int = -(-n_mcus // restart)
    out = bytearray(header(w, h, mono, quality, restart))
    for j in range(n_int):
        bits, pred = _Bits(), [0, 0, 0]
        for m in range(j * restart, min((j + 1) * restart, n_mcus)):
            mx, my = m % mw, m // mw
            blocks = [(0, my, mx)] if mono else [(0, 2 * my, 2 * mx), (0, 2 * my, 2 * mx + 1), (0, 2 * my + 1, 2 * mx), (0, 2 * my + 1, 2 * mx + 1), (1, my, mx), (2, my, mx)]
            for comp, by, bx in blocks:
                z = levels[comp][by, bx]
                t = int(comp > 0)
                diff = int(z[0]) - pred[comp]
                pred[comp] = int(z[0])
                s = _category(diff)
                assert s <= 11
                k.max_dc_cat = max(k.max_dc_cat, s)
                bits.put(*dc[t][s])
                bits.put(_magnitude(diff, s), s)
                run = 0
                for i in range(1, 64):
                    if z[i] == 0:
                        run += 1
                        continue
                    while run >= 16:
                        bits.put(*ac[t][0xF0])
                        k.zrl, run = k.zrl + 1, run - 16
                    s = _category(z[i])
                    assert s <= 10
                    k.max_ac_cat = max(k.max_ac_cat, s)
                    bits.put(*ac[t][run << 4 | s])
                    bits.put(_magnitude(z[i], s), s)
                    run = 0
                if z[63] == 0:
                    bits.put(*ac[t][0x00])
                    k.eob_only += int(not z[1:].any())
                else:
                    k.no_eob += 1
        pad = -bits.n % 8
        bits.put((1 << pad) - 1, pad)
        data = bits.acc.to_bytes(bits.n // 8, "big")
        k.pad_ff += int(pad > 0 and data[-1] == 0xFF)
        k.stuffed += data.count(0xFF)
        k.intervals += 1
        out += data.replace(b"\xff", b"\xff\x00")
        out += bytes([0xFF, 0xD0 + j % 8]) if j + 1 < n_int else b"\xff\xd9"
    return bytes(out)


def header_bytes(mono):
    return len(header(16, 16, mono, 50, 1))


def i420_of(planes):
    return np.concatenate([np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in planes])


def reference_blocks(seed=1):
    """The 42 000 blocks of the header's statement: uniform noise, 0 / 255 blocks, a narrow Gaussian."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (14000, 8, 8))
    b = rng.integers(0, 2, (14000, 8, 8)) * 255
    c = np.clip(np.rint(rng.normal(128, 6, (14000, 8, 8))), 0, 255).astype(np.int64)
    return np.concatenate([a, b, c]).astype(np.uint8)
