"""Rewrites every SPS of an Annex-B stream so that it carries a VUI that holds only video_signal_type (E.1.1): video_format 5, the given
video_full_range_flag and, optionally, a colour description with the given matrix_coefficients (colour_primaries and transfer_characteristics 2,
"unspecified").  Every other VUI flag is 0 and cropping stays as it is.  Pixels do not depend on the VUI, so the generator's reconstruction stays the
reference.  The generator always writes vui_parameters_present_flag 0, which is what the rewrite expects to find.  Built on tests/spsutil.py."""
import spsutil


def _vui_bits(full_range, matrix):
    bits = "0" + "0" + "1"  # aspect_ratio_info_present_flag, overscan_info_present_flag, video_signal_type_present_flag
    bits += "{:03b}".format(5) + ("1" if full_range else "0")  # video_format, video_full_range_flag
    if matrix is None:
        bits += "0"
    else:
        bits += "1" + "{:08b}{:08b}{:08b}".format(2, 2, matrix)  # colour_description_present_flag, primaries, transfer, matrix_coefficients
    return bits + "0" * 6  # chroma_loc_info, timing_info, nal_hrd, vcl_hrd, pic_struct, bitstream_restriction: all absent


def _with_vui(nal, full_range, matrix):
    body = nal.rstrip(b"\x00")
    raw = spsutil.unescape(body)
    b = spsutil._Bits(raw[1:])
    spsutil._walk_to_cropping(b)
    if b.u(1):
        for _ in range(4):
            b.ue()
    p = b.pos
    assert b.u(1) == 0, "the SPS already has a VUI"
    assert b.s.rindex("1") == p + 1, "rbsp_trailing_bits expected behind vui_parameters_present_flag"
    bits = b.s[:p] + "1" + _vui_bits(full_range, matrix) + "1"
    bits += "0" * (-len(bits) % 8)
    rbsp = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    return spsutil.escape(raw[:1] + rbsp) + nal[len(body):]


def with_video_signal_type(stream, full_range=0, matrix=None):
    """The stream with the VUI described above in every SPS; everything else byte for byte as it was."""
    out, n = [], 0
    for sc, nal in spsutil.split_nals(stream):
        if nal and (nal[0] & 31) == 7:
            nal, n = _with_vui(nal, full_range, matrix), n + 1
        out.append(sc + nal)
    assert n, "no SPS in the stream"
    return b"".join(out)
