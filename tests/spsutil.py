"""Rewrites the cropping fields of every SPS of an Annex-B stream, and states what a decoder must then put out.

Pixels do not depend on frame_cropping_flag and the four offsets (7.4.2.1.1 only says which part of a decoded picture is
output), so a generated stream keeps its coded-size reconstruction as the reference while its SPS announces any crop
rectangle -- including the ones the generator never writes (a left or top offset, four at once, odd monochrome sizes).
expected_frames() is 7-18 .. 7-21 and the I420 layout in numpy slicing; nothing here calls the product, the oracle or
the generator."""
import numpy as np

HIGH_PROFILES = (100, 110, 122, 244, 44, 83, 86, 118, 128, 138, 139, 134, 135)  # 7.3.2.1.1: these carry chroma_format_idc


def split_nals(stream):
    """[(start code, NAL unit bytes)] of an Annex-B stream with 3- and 4-byte start codes; whatever precedes the first one is
    returned as the start code of a unit without bytes."""
    stream = bytes(stream)
    starts, i, n = [], 0, len(stream)
    while i + 3 <= n:
        if stream[i] == 0 and stream[i + 1] == 0 and stream[i + 2] == 1:
            starts.append((i - 1 if i > 0 and stream[i - 1] == 0 and (not starts or starts[-1][1] < i) else i, i + 3))
            i += 3
        else:
            i += 1
    out = []
    if not starts or starts[0][0] > 0:
        out.append((stream[:starts[0][0] if starts else n], b""))
    for k, (a, b) in enumerate(starts):
        out.append((stream[a:b], stream[b:starts[k + 1][0] if k + 1 < len(starts) else n]))
    return out


def unescape(nal):
    """NAL unit bytes -> without emulation_prevention_three_byte (7.3.1)."""
    out, zeros = bytearray(), 0
    for c in nal:
        if zeros >= 2 and c == 3:
            zeros = 0
            continue
        out.append(c)
        zeros = zeros + 1 if c == 0 else 0
    return bytes(out)


def escape(raw):
    """The inverse: 00 00 0x (x <= 3) never appears in a NAL unit."""
    out, zeros = bytearray(), 0
    for c in raw:
        if zeros >= 2 and c <= 3:
            out.append(3)
            zeros = 0
        out.append(c)
        zeros = zeros + 1 if c == 0 else 0
    return bytes(out)


class _Bits:
    def __init__(self, data):
        self.s = "".join("{:08b}".format(c) for c in data)
        self.pos = 0

    def u(self, n):
        assert self.pos + n <= len(self.s), "SPS ends early"
        v = int(self.s[self.pos:self.pos + n], 2) if n else 0
        self.pos += n
        return v

    def ue(self):
        z = 0
        while self.u(1) == 0:
            z += 1
        return (1 << z) - 1 + self.u(z)

    def se(self):
        k = self.ue()
        return (k + 1) // 2 if k & 1 else -(k // 2)


def _ue_bits(v):
    b = "{:b}".format(v + 1)
    return "0" * (len(b) - 1) + b


def _walk_to_cropping(b):
    """Reads seq_parameter_set_data() (7.3.2.1.1) up to frame_cropping_flag; returns what the geometry needs."""
    profile = b.u(8)
    b.u(16)  # constraint flags, level_idc
    b.ue()   # seq_parameter_set_id
    cfi = 1
    if profile in HIGH_PROFILES:
        cfi = b.ue()
        if cfi == 3:
            b.u(1)  # separate_colour_plane_flag
        b.ue(), b.ue(), b.u(1)  # bit depths, qpprime_y_zero_transform_bypass_flag
        if b.u(1):  # seq_scaling_matrix_present_flag
            for i in range(8 if cfi != 3 else 12):
                if b.u(1):  # scaling_list(): 7.3.2.1.1.1
                    last = nxt = 8
                    for _ in range(16 if i < 6 else 64):
                        if nxt != 0:
                            nxt = (last + b.se() + 256) % 256
                        last = last if nxt == 0 else nxt
    b.ue()  # log2_max_frame_num_minus4
    poc_type = b.ue()
    if poc_type == 0:
        b.ue()
    elif poc_type == 1:
        b.u(1), b.se(), b.se()
        for _ in range(b.ue()):
            b.se()
    b.ue(), b.u(1)  # max_num_ref_frames, gaps_in_frame_num_value_allowed_flag
    wmb, hmu = b.ue() + 1, b.ue() + 1
    fmo = b.u(1)
    if not fmo:
        b.u(1)  # mb_adaptive_frame_field_flag
    b.u(1)  # direct_8x8_inference_flag
    return dict(chroma_format_idc=cfi, coded_w=wmb * 16, coded_h=hmu * (2 - fmo) * 16, frame_mbs_only=fmo)


def _recrop_sps(nal, crop):
    body = nal.rstrip(b"\x00")  # trailing_zero_8bits, if any, stay where they are
    raw = unescape(body)
    b = _Bits(raw[1:])
    info = _walk_to_cropping(b)
    p0 = b.pos
    if b.u(1):
        for _ in range(4):
            b.ue()
    p1 = b.pos
    stop = b.s.rindex("1")  # rbsp_stop_one_bit
    assert stop >= p1, "no VUI flag / trailing bits"
    bits = b.s[:p0] + ("1" + "".join(_ue_bits(v) for v in crop) if any(crop) else "0") + b.s[p1:stop] + "1"
    bits += "0" * (-len(bits) % 8)
    rbsp = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    return escape(raw[:1] + rbsp) + nal[len(body):], info


def recrop(stream, left, right, top, bottom):
    """The stream with frame_cropping_flag and the four frame_crop_*_offset of every SPS replaced (flag 0 when all are 0), everything
    else -- VUI included -- bit for bit as it was.  Returns (stream, dict(chroma_format_idc, coded_w, coded_h, frame_mbs_only))."""
    out, info = [], None
    for sc, nal in split_nals(stream):
        if nal and (nal[0] & 31) == 7:
            nal, info = _recrop_sps(nal, (left, right, top, bottom))
        out.append(sc + nal)
    assert info is not None, "no SPS in the stream"
    return b"".join(out), info


def sps_rbsps(stream):
    """RBSP (behind the NAL header byte) of every SPS of the stream."""
    return [unescape(nal)[1:] for _, nal in split_nals(stream) if nal and (nal[0] & 31) == 7]


def crop_rect(info, left, right, top, bottom):
    """(x0, y0, w, h) of the output rectangle in luma samples: 7-18 .. 7-21 with CropUnitX = SubWidthC, CropUnitY = SubHeightC *
    (2 - frame_mbs_only_flag) for 4:2:0 and CropUnitX = 1, CropUnitY = 2 - frame_mbs_only_flag for ChromaArrayType 0."""
    assert info["chroma_format_idc"] in (0, 1)
    ux = 1 if info["chroma_format_idc"] == 0 else 2
    uy = (1 if info["chroma_format_idc"] == 0 else 2) * (2 - info["frame_mbs_only"])
    x0, y0 = ux * left, uy * top
    w, h = info["coded_w"] - ux * (left + right), info["coded_h"] - uy * (top + bottom)
    assert w > 0 and h > 0
    return x0, y0, w, h


def i420_size(w, h):
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


def expected_frames(rec, info, left, right, top, bottom):
    """uint8[n, i420_size(w, h)]: the crop rectangle of each coded-size I420 frame of `rec` -- luma [y0:y0+h, x0:x0+w], then Cb and Cr
    [y0//2 : y0//2 + ceil(h/2), x0//2 : x0//2 + ceil(w/2)]."""
    W, H = info["coded_w"], info["coded_h"]
    x0, y0, w, h = crop_rect(info, left, right, top, bottom)
    wc, hc = (w + 1) // 2, (h + 1) // 2
    rec = np.asarray(rec)
    assert rec.ndim == 2 and rec.shape[1] == W * H * 3 // 2
    out = np.empty((rec.shape[0], i420_size(w, h)), dtype=np.uint8)
    for f in range(rec.shape[0]):
        y = rec[f, :W * H].reshape(H, W)
        cb = rec[f, W * H:W * H * 5 // 4].reshape(H // 2, W // 2)
        cr = rec[f, W * H * 5 // 4:].reshape(H // 2, W // 2)
        out[f] = np.concatenate([y[y0:y0 + h, x0:x0 + w].reshape(-1)] +
                                [c[y0 // 2:y0 // 2 + hc, x0 // 2:x0 // 2 + wc].reshape(-1) for c in (cb, cr)])
    return out
