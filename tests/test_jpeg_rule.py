"""The JPEG rule on the CPU (K13): the pure functions of include/h264mi.h ("JPEG snapshots") against the yardstick tests/jpegutil.py, and the yardstick
against third parties -- Pillow's quantisation tables, scipy's floating-point DCT, and Pillow (libjpeg) as the decoder and as a second encoder of the same
planes.  The device's files: tests/test_output_jpeg.py."""
import ctypes
import io

import numpy as np
import pytest

import jpegutil as ju

QUALITIES = (1, 10, 50, 75, 90, 100)
# (w, h, mono, restart_mcus): one MCU; odd; odd and mono; several MCUs and rows; ten intervals (the RST index wraps); an interval per MCU; 3 MCUs an interval
SHAPES = [(16, 16, False, 0), (17, 17, False, 0), (33, 17, True, 0), (48, 32, False, 0), (16, 160, False, 0), (48, 32, False, 1), (48, 32, False, 3)]
# Against Pillow's own encode of the same planes (quality alike, subsampling=2).  The two encoders round the DCT differently (libjpeg: a scaled integer
# or float DCT and its own quantiser rounding; here: the block rule), restart markers, the DRI segment and the pad bits of every interval cost bytes, and
# the two replicate the edge of an odd size differently.  Measured on the yardstick over SHAPES (colour) plus 64 x 48 and 176 x 144, qualities 10, 50, 75,
# 90, 100: the luma PSNR is at most 0.041 dB below Pillow's (17 x 17, quality 50; at quality 100 it is 0.33 .. 0.64 dB ABOVE), the file at most 6.9 %
# longer (17 x 17, quality 100: 1067 against 998 bytes; 176 x 144: between 0.7 % shorter and 1.5 % longer).
PSNR_MARGIN_DB = 0.25
LENGTH_MARGIN = 1.10


@pytest.fixture(scope="module")
def L(H):
    return H.lib()


def _picture(w, h, seed):
    """Something a decoder might have made: smooth waves, block edges, a little noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    cw, ch = (w + 1) // 2, (h + 1) // 2
    yc, xc = np.mgrid[0:ch, 0:cw]
    planes = (128 + 60 * np.sin(x / 7.0 + seed) + 40 * np.cos(y / 5.0) + ((x // 8 + y // 8) % 2) * 12 + rng.normal(0, 4, (h, w)),
              128 + 30 * np.sin(xc / 9.0) + rng.normal(0, 2, (ch, cw)), 128 + 30 * np.cos(yc / 6.0) + rng.normal(0, 2, (ch, cw)))
    return [np.clip(np.rint(p), 0, 255).astype(np.uint8) for p in planes]


def test_quant_tables_are_the_ones_pillow_writes(L, H):
    from PIL import Image
    for q in QUALITIES:
        f = io.BytesIO()
        Image.new("RGB", (16, 16), (10, 200, 90)).save(f, "JPEG", quality=q, subsampling=2)
        theirs = Image.open(io.BytesIO(f.getvalue())).quantization  # natural order
        for chroma in (0, 1):
            arr = (ctypes.c_uint16 * 64)()
            assert L.h264mi_jpeg_quant_table(q, chroma, arr) == 0
            assert list(arr) == list(theirs[chroma]) == ju.quant_table(q, chroma).tolist() == H.jpeg_quant_table(q, chroma), (q, chroma)
    arr = (ctypes.c_uint16 * 64)()
    for bad in ((0, 0), (101, 0), (50, 2), (50, -1)):
        assert L.h264mi_jpeg_quant_table(bad[0], bad[1], arr) == -1, bad
    assert L.h264mi_jpeg_quant_table(50, 0, None) == -1


def _levels(L, blocks, q):
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 64)
    qa = (ctypes.c_uint16 * 64)(*[int(v) for v in q])
    out = np.zeros((len(blocks), 64), dtype=np.int16)
    u8, i16 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int16)
    for i in range(len(blocks)):
        assert L.h264mi_jpeg_block(ctypes.cast(blocks.ctypes.data + 64 * i, u8), qa, ctypes.cast(out.ctypes.data + 128 * i, i16)) == 0
    return out.reshape(-1, 8, 8)


@pytest.fixture(scope="module")
def blocks():
    b = ju.reference_blocks()
    b.setflags(write=False)
    return b


@pytest.mark.parametrize("quality", [100, 90, 10])
def test_block_rule_equals_the_yardstick_on_the_reference_set(quality, blocks, L):
    assert len(blocks) == 42000
    q = ju.quant_table(quality, 0)
    assert np.array_equal(_levels(L, blocks, q), ju.block_levels(blocks, q))


def test_block_rule_at_the_sign_aligned_extremes_of_every_row_of_m(L):
    """Samples 255 / 0 by the sign of M[j][y] * M[k][n], and the inverse: the largest |c| of every coefficient (j, k).  Q = 1 keeps every bit."""
    s = np.sign(ju.M)
    ext = np.array([[np.where(np.outer(s[j], s[k]) * sign > 0, 255, 0) for sign in (1, -1)] for j in range(8) for k in range(8)]).reshape(-1, 8, 8)
    for q in (np.ones(64, dtype=np.int64), ju.quant_table(90, 1), np.full(64, 255)):
        got, want = _levels(L, ext, q), ju.block_levels(ext, q)
        assert np.array_equal(got, want)
    top = np.abs(ju.block_levels(ext, np.ones(64, dtype=np.int64))).reshape(-1, 64)
    assert top[:, 0].max() == 1024 and top[:, 1:].max() <= 1023, "categories 11 for DC and 10 for AC suffice"
    assert top[:, 1:].max() >= 512, "... and 10 is needed"
    bad_q = (ctypes.c_uint16 * 64)(*([1] * 63 + [0]))
    zero = (ctypes.c_uint8 * 64)()
    lv = (ctypes.c_int16 * 64)()
    assert L.h264mi_jpeg_block(zero, bad_q, lv) == -1 and L.h264mi_jpeg_block(None, bad_q, lv) == -1
    bad_q[63] = 256
    assert L.h264mi_jpeg_block(zero, bad_q, lv) == -1


@pytest.mark.parametrize("quality,share", [(100, 0.02), (90, 0.005)])
def test_block_rule_is_within_one_of_a_float_dct(quality, share, blocks):
    """scipy's orthonormal DCT and round-half-away: never more than 1 apart, and apart in at most `share` of the coefficients (measured: 0.79 % at quality
    100, 0.13 % at 90 -- the conditions have margin)."""
    from scipy.fft import dctn
    q = ju.quant_table(quality, 0).reshape(8, 8)
    c = dctn(blocks.astype(np.float64) - 128, axes=(-2, -1), norm="ortho") / q
    want = (np.sign(c) * np.floor(np.abs(c) + 0.5)).astype(np.int64)
    got = ju.block_levels(blocks, q.reshape(-1))
    assert np.abs(got - want).max() <= 1
    assert np.count_nonzero(got != want) <= share * got.size


def _luma_psnr(data, luma):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", im.size)
    assert im.mode == "YCbCr"
    a = np.asarray(im)[:, :, 0].astype(np.float64)
    return 10 * np.log10(255.0 ** 2 / max(np.mean((a - luma) ** 2), 1e-9))


@pytest.mark.parametrize("w,h,mono,restart", SHAPES)
def test_pillow_opens_the_yardsticks_files(w, h, mono, restart):
    """The right size and mode; and, for colour, luma PSNR and length next to Pillow's own encode of the same planes."""
    from PIL import Image
    for quality in (50, 90):
        planes = _picture(w, h, w + h + quality)[:1 if mono else 3]
        k = ju.Counters()
        data = ju.encode(ju.i420_of(planes), w, h, mono, quality, False, restart, counters=k)
        assert k.intervals == -(-(-(-w // (8 if mono else 16)) * -(-h // (8 if mono else 16))) // (restart or -(-w // (8 if mono else 16))))
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (w, h) and im.mode == ("L" if mono else "RGB")
        if mono:
            assert 10 * np.log10(255.0 ** 2 / np.mean((np.asarray(im).astype(np.float64) - planes[0]) ** 2)) > 30
            continue
        up = [np.repeat(np.repeat(c, 2, 0), 2, 1)[:h, :w] for c in planes[1:]]  # (Pillow averages 2 x 2: the chroma planes it codes are these ones)
        f = io.BytesIO()
        Image.merge("YCbCr", [Image.fromarray(p) for p in [planes[0]] + up]).save(f, "JPEG", quality=quality, subsampling=2)
        ours, theirs = _luma_psnr(data, planes[0]), _luma_psnr(f.getvalue(), planes[0])
        print("%dx%d restart %d quality %d: luma PSNR %.3f dB (Pillow %.3f), %d bytes (Pillow %d)" % (w, h, restart, quality, ours, theirs, len(data), len(f.getvalue())))
        assert ours >= theirs - PSNR_MARGIN_DB
        assert len(data) <= LENGTH_MARGIN * len(f.getvalue())


def test_the_huffman_tables_in_the_file_are_pillows(H):
    """The DHT segments the library would write are in the yardstick's header byte for byte, and the yardstick took them from Pillow's file."""
    segs = ju.segments(ju.header(48, 32, False, 75, 3))
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert [b[0] for m, b in segs if m == 0xC4] == [0x00, 0x10, 0x01, 0x11]
    assert [m for m, _ in ju.segments(ju.header(33, 17, True, 75, 0x1234))] == [0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xDD, 0xDA]


def test_jpeg_size(L, H):
    for mono in (False, True):
        for w, h, r in ((16, 16, 0), (48, 32, 1), (173, 137, 0), (1920, 1080, 8)):
            hb, bound = H.jpeg_size(w, h, mono, 100, "keep", r)
            assert hb == ju.header_bytes(mono) == len(ju.header(w, h, mono, 100, r or 1)) and bound % 16 == 0
            if w * h < 40000:
                rng = np.random.default_rng(w + h)
                planes = [rng.integers(0, 256, (h, w))] + ([] if mono else [rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2)) for _ in range(2)])
                n = len(ju.encode(ju.i420_of(planes), w, h, mono, 100, False, r))
                assert hb + w * h // 2 < n < bound, (w, h, mono, n, bound)
    S = H._lib.JpegSpec
    hb, bb = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert L.h264mi_jpeg_size(ctypes.byref(S(90, 1, 0, 0)), 16, 16, 0, None, None) == 0
    for spec, w, h in ((S(0, 1, 0, 0), 16, 16), (S(101, 1, 0, 0), 16, 16), (S(90, 3, 0, 0), 16, 16), (S(90, -1, 0, 0), 16, 16), (S(90, 1, -1, 0), 16, 16),
                       (S(90, 1, 65536, 0), 16, 16), (S(90, 1, 0, 1), 16, 16), (S(90, 1, 0, 0), 0, 16), (S(90, 1, 0, 0), 16, 16385)):
        assert L.h264mi_jpeg_size(ctypes.byref(spec), w, h, 0, ctypes.byref(hb), ctypes.byref(bb)) == -1
    assert L.h264mi_jpeg_size(None, 16, 16, 0, ctypes.byref(hb), ctypes.byref(bb)) == -1 and (hb.value, bb.value) == (7, 7)
    # the largest legal item's bound fits the 32 bits of a result
    assert L.h264mi_jpeg_size(ctypes.byref(S(100, 1, 1, 0)), 16384, 16384, 0, ctypes.byref(hb), ctypes.byref(bb)) == 0 and bb.value < 2 ** 32
