"""Random access, the parts without a decoder: h264mi_sei_recovery_point against known answers, the generator's open groups of pictures
(open_gop_period) against the oracle and against the syntax an entry point is made of, and the mode switch's declarations."""
import ctypes
import os
import re

import numpy as np
import pytest

import rautil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EBITSTREAM = -1, -2
RP = b"\x06\x01\xc4"  # payloadType 6, payloadSize 1: recovery_frame_cnt 0, exact_match_flag 1, broken_link_flag 0, changing_slice_group_idc 0


def _rp(H, nal):
    out = H._lib.RecoveryPoint()
    r = H.lib().h264mi_sei_recovery_point(bytes(nal), len(nal), ctypes.byref(out))
    return r, (out.found, out.recovery_frame_cnt, out.exact_match_flag, out.broken_link_flag, out.changing_slice_group_idc)


@pytest.mark.parametrize("nal, want", [
    (b"\x06" + RP + b"\x80", (0, (1, 0, 1, 0, 0))),
    (b"\x06\x06\x02\x32\xc0\x80", (0, (1, 5, 0, 1, 1))),
    (b"\x06\x00\x03\xaa\xbb\xcc" + RP + b"\x80", (0, (1, 0, 1, 0, 0))),                  # a 3-byte payload of type 0 in front
    (b"\x06\x05\xff\x2d" + b"\x55" * 300 + RP + b"\x80", (0, (1, 0, 1, 0, 0))),          # type 5, size 255 + 45 in front
    (b"\x06\xff\x0a\xff\xff\x02" + b"\x33" * 512 + RP + b"\x80", (0, (1, 0, 1, 0, 0))),  # type 265, size 512: extension bytes in both
    (b"\x06\x05\x04\x55\x55\x55\x55\x80", (0, (0, 0, 0, 0, 0))),                         # no recovery point
    (b"\x06\x00\x03\x00\x00\x03\x01" + RP + b"\x80", (0, (1, 0, 1, 0, 0))),              # the payload 00 00 01 needs an emulation prevention byte
    (b"\x06\x06\x01", (EBITSTREAM, (0, 0, 0, 0, 0))),                                    # cut off in front of the payload
    (b"\x06\x05\xff", (EBITSTREAM, (0, 0, 0, 0, 0))),                                    # ... inside a payload size
    (b"\x06\x05\x09\x55\x55\x80", (EBITSTREAM, (0, 0, 0, 0, 0))),                        # ... inside a payload
    (b"\x06\x06\x00\x80", (EBITSTREAM, (0, 0, 0, 0, 0))),                                # a recovery point without a bit
    (b"\x21\x06\x01\xc4\x80", (EINVAL, (0, 0, 0, 0, 0))),                                # a unit of type 1
])
def test_sei_recovery_point_known_answers(H, nal, want):
    r, got = _rp(H, nal)
    assert r == want[0]
    if r == 0:
        assert got == want[1]


def test_mode_switch_is_declared_exported_and_bound(H):
    L, header = H.lib(), open(os.path.join(ROOT, "include", "h264mi.h")).read()
    for sym in ("h264mi_decoder_set_random_access", "h264mi_sei_recovery_point", "h264mi_frame_entry", "h264mi_stream_random_access_stats"):
        assert re.search(r"int32_t %s\(" % sym, header) and sym in H._lib.EXPORTS and hasattr(L, sym), sym
    assert re.search(r"#define H264MI_RA_OFF 0\b", header) and re.search(r"#define H264MI_RA_RECOVERY_POINT 1\b", header)
    assert (H.RA_OFF, H.RA_RECOVERY_POINT) == (0, 1)
    # a setter, not a field of the configuration
    assert H._lib.Config._fields_[-1][0] == "conceal_errors"
    for mode in (0, 1, 2):
        assert L.h264mi_decoder_set_random_access(None, mode) == EINVAL  # no decoder
    assert L.h264mi_frame_entry(None, 0, 0, None) == EINVAL and L.h264mi_stream_random_access_stats(None, 0, None) == EINVAL
    go = open(os.path.join(ROOT, "go", "h264", "h264mi.go")).read()
    for sym in ("h264mi_decoder_set_random_access", "h264mi_sei_recovery_point", "h264mi_frame_entry", "h264mi_stream_random_access_stats"):
        assert "C." + sym in go, sym


def _slice_type(stream, unit):
    """slice_type of a slice NAL unit: the second ue(v) of its header"""
    s, e, _ = unit
    h = s + (4 if stream[s:s + 4] == b"\x00\x00\x00\x01" else 3)
    bits = "".join(format(b, "08b") for b in stream[h + 1:h + 9])
    at, vals = 0, []
    for _ in range(2):
        z = 0
        while bits[at + z] == "0":
            z += 1
        vals.append(int(bits[at + z:at + 2 * z + 1], 2) - 1)
        at += 2 * z + 1
    return vals[1] % 5


@pytest.mark.parametrize("name", sorted(rautil.RECIPES))
def test_generator_open_gop(sg, oracle_mod, H, name):
    c = rautil.case(sg, name)
    assert c.features & sg.FEATURE_OPEN_GOP and len(c.entries) >= 2
    frames, _ = oracle_mod.decode(c.stream, crop=False)
    assert np.array_equal(frames, c.recon)  # the oracle passes over SEI and decodes non-IDR I pictures of a whole stream
    assert [t for _, _, t in c.units[:3]] == [7, 8, 5]
    first_ps = c.stream[c.units[0][0]:c.units[2][0]]
    period = -(-c.kw["open_gop_period"] // (c.kw["bframes"] + 1)) * (c.kw["bframes"] + 1)
    for k, en in enumerate(c.entries):
        u = en["unit"]
        assert [t for _, _, t in c.units[u:u + 3]] == [7, 8, 6]
        assert c.stream[c.units[u][0]:c.units[u + 2][0]] == first_ps, "the parameter sets again, byte for byte"
        s, e, _ = c.units[u + 2]
        h = s + (4 if c.stream[s:s + 4] == b"\x00\x00\x00\x01" else 3)
        assert _rp(H, c.stream[h:e]) == (0, (1, 0, 1, 0, 0))
        # then the slices of the entry picture (both fields of a frame of fields): type 1, all I
        v = u + 3
        for _ in range(c.pics_per_frame * c.kw.get("slices", 1)):
            assert c.units[v][2] == 1 and _slice_type(c.stream, c.units[v]) == 2
            v += 1
        assert c.units[v][2] == 1 and _slice_type(c.stream, c.units[v]) != 2, "the picture behind it predicts"
        # every multiple of the period is an entry point, and the B pictures in front of it in display order follow it
        assert en["leading"] == c.kw["bframes"] * c.pics_per_frame
        assert en["frame"] == (k + 1) * period - (c.kw["bframes"] if c.kw["bframes"] else 0)


def test_generator_open_gop_off_and_refusals(sg):
    kw = dict(rautil.RECIPES["b"], frames=8)
    assert sg.encode(**dict(kw, open_gop_period=0))[0] == sg.encode(**{k: v for k, v in kw.items() if k != "open_gop_period"})[0]
    assert not sg.last_features() & sg.FEATURE_OPEN_GOP and sg.last_entries() == []
    # (appended to the struct; the two fields of the residual trace and stimulus were appended after it)
    assert [f[0] for f in sg.Params._fields_[-3:]] == ["open_gop_period", "trace_residual", "residual_stim"]
    for extra in (dict(mmco=1), dict(rplm=1), dict(idr_long_term=1), dict(fn_gap_period=3), dict(wp_range=2, weighted_pred=1), dict(direct_temporal=1)):
        with pytest.raises(RuntimeError, match="open_gop_period"):
            sg.encode(**dict(rautil.RECIPES["a"], frames=8, **extra))
