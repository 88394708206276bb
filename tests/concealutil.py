"""Yardstick of the error-concealment tests: damages generator streams and writes the REPAIRED stream the rule is stated in.

The rule (include/h264mi.h, h264mi_config.conceal_errors): the lost macroblocks of a concealable picture come out bit for bit as a conforming
decoder reconstructs the stream in which they are coded as P slices of P_Skip macroblocks only -- num_ref_idx_active_override_flag 1 with one
active reference, no list modification, a pred_weight_table() with all flags 0 where the PPS asks for one, slice_qp_delta 0,
disable_deblocking_filter_idc 0 with zero offsets where the PPS has the fields, and nal_ref_idc, frame_num, the picture-order fields and the
marking syntax of the picture they belong to.  `make(stream, picks, mode)` returns that stream and the damaged one:

  mode "lost":    the chosen slice NAL units are removed
  mode "header":  they are replaced by a slice NAL unit whose header does not parse (slice_type 20)
  mode "damaged": their slice data is replaced by zero bytes (cabac_zero_words).  CAVLC: the first mb_skip_run has no code word (entropy error 1).
                  CABAC: the arithmetic decoder's offset stays 0, so every bin is the most probable symbol and end_of_slice_flag never is 1 --
                  the slice cannot end before it runs out of its macroblock range (error 30) or trips over something else on the way.

The slice headers are written with the generator's bit writer and the slice data of CABAC streams with its arithmetic encoder (streamgen/sg_bits.c,
called through ctypes; nothing of the generator changes): one context, mb_skip_flag with ctxIdxInc 0 throughout an all-skip slice, and
end_of_slice_flag.  The headers of the removed slices are read with the product's CPU-side parser (h264mi_slice_header_parse)."""
import ctypes

import numpy as np

import h264decode_amd as H
import streamgen

ZERO_BYTES = 16384  # of slice data in a "damaged" slice: more bits than a slice of these pictures can consume


# ---------------------------------------------------------------- Annex-B
def split_units(stream):
    """The stream cut at its start codes: [bytes], each with its (3- or 4-byte) start code in front."""
    starts, i, n = [], 0, len(stream)
    while i + 3 <= n:
        if stream[i] == 0 and stream[i + 1] == 0 and stream[i + 2] == 1:
            starts.append(i - 1 if i > 0 and stream[i - 1] == 0 else i)
            i += 3
        else:
            i += 1
    starts.append(n)
    return [bytes(stream[a:b]) for a, b in zip(starts, starts[1:])]


def _sc_len(unit):
    return 4 if unit[:4] == b"\x00\x00\x00\x01" else 3


def escape(rbsp):
    """Emulation prevention (7.4.1.1); an RBSP that ends in 0x00 gets a final 0x03."""
    out, zeros = bytearray(), 0
    for b in rbsp:
        if zeros >= 2 and b <= 3:
            out.append(3)
            zeros = 0
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    if out and out[-1] == 0:
        out.append(3)
    return bytes(out)


# ---------------------------------------------------------------- the generator's bit writer through ctypes
class _BW:
    def __init__(self, cap=1 << 16):
        L = streamgen.lib()
        vp = ctypes.c_void_p
        for name, args, res in (("sg_bw_init", [vp, vp, ctypes.c_size_t], None), ("sg_put", [vp, ctypes.c_uint32, ctypes.c_int], None),
                                ("sg_put_ue", [vp, ctypes.c_uint32], None), ("sg_put_se", [vp, ctypes.c_int32], None), ("sg_trailing", [vp], None),
                                ("sg_bw_bytes", [vp], ctypes.c_size_t), ("sg_bw_aligned", [vp], ctypes.c_int),
                                ("sg_cabac_init_ctx", [vp, ctypes.c_int, ctypes.c_int], None), ("sg_cabac_start", [vp], None),
                                ("sg_cabac_bin", [vp, ctypes.c_int, ctypes.c_int], None), ("sg_cabac_terminate", [vp, ctypes.c_int], None)):
            f = getattr(L, name)
            f.argtypes, f.restype = args, res
        self.L = L
        self.buf = ctypes.create_string_buffer(cap)
        L.sg_bw_sizeof.restype = ctypes.c_size_t
        self.w = ctypes.create_string_buffer(L.sg_bw_sizeof())  # an sg_bw (sg_int.h), opaque here
        L.sg_bw_init(self.w, self.buf, cap)

    def u(self, v, n):
        if n:
            self.L.sg_put(self.w, v, n)

    def ue(self, v):
        self.L.sg_put_ue(self.w, v)

    def se(self, v):
        self.L.sg_put_se(self.w, v)

    def aligned(self):
        return bool(self.L.sg_bw_aligned(self.w))

    def bytes(self):
        return self.buf.raw[:self.L.sg_bw_bytes(self.w)]


# ---------------------------------------------------------------- parsing
class SliceInfo:
    """One slice NAL unit: where it is (unit), which picture (pic, in decoding order) and which place inside it (pos: by first_mb), its
    parsed header and parameter sets, and the macroblock addresses it covers (mbs)."""


def parse(stream):
    """(units, slices, pics): pics[p] = the SliceInfo of picture p ordered by first_mb_in_slice."""
    units = split_units(stream)
    L = H.lib()
    sps = pps = None
    slices, pics = [], []
    first = None
    seen = set()
    for ui, u in enumerate(units):
        nal = u[_sc_len(u):]
        t = nal[0] & 31
        if t == 7:
            sps = H.NewSPS(H.NewNalUnit(nal).RBSP())
        elif t == 8:
            pps = H.NewPPS(sps, H.NewNalUnit(nal).RBSP())
        elif t in (1, 5):
            nu = H.NewNalUnit(nal)
            hdr = H.NewSliceContext(H.VideoStream(sps, pps), nu, nu.RBSP()).Slice.Header
            s = SliceInfo()
            s.unit, s.hdr, s.sps, s.pps, s.ref_idc, s.type, s.rbsp = ui, hdr, sps, pps, (nal[0] >> 5) & 3, t, nu.RBSP()
            new = first is None or hdr.first_mb_in_slice in seen or L.h264mi_slice_starts_picture(ctypes.byref(sps._c), ctypes.byref(first.hdr._c), ctypes.byref(hdr._c)) == 1
            if new:
                pics.append([])
                first, seen = s, set()
            seen.add(hdr.first_mb_in_slice)
            s.pic = len(pics) - 1
            pics[-1].append(s)
            slices.append(s)
    for p in pics:
        p.sort(key=lambda s: s.hdr.first_mb_in_slice)
        h0 = p[0]
        wmb, hmb = h0.sps.pic_width_in_mbs, h0.sps.pic_height_in_mbs // (2 if h0.hdr.field_pic else 1)
        total = wmb * hmb
        sgmap = H.MbToSliceGroupMap(h0.sps, h0.pps, h0.hdr) if h0.pps.num_slice_groups_minus1 > 0 else np.zeros(total, dtype=np.uint8)
        for i, s in enumerate(p):
            s.pos, s.n_in_pic, s.wmb, s.hmb = i, len(p), wmb, hmb
            f = s.hdr.first_mb_in_slice
            end = total
            for o in p[i + 1:]:
                if sgmap[o.hdr.first_mb_in_slice] == sgmap[f]:
                    end = o.hdr.first_mb_in_slice
                    break
            s.mbs = [a for a in range(f, end) if sgmap[a] == sgmap[f]]
    return units, slices, pics


# ---------------------------------------------------------------- writers
def _header(bw, s):
    """slice_header() (7.3.3) of the replacement P slice of `s`."""
    h, sps, pps = s.hdr, s.sps, s.pps
    assert not sps.use_separate_color_plane and not h.field_pic and s.type == 1
    bw.ue(h.first_mb_in_slice)
    bw.ue(0)  # slice_type P
    bw.ue(h.pps_id)
    bw.u(h.frame_num, sps.log2_max_frame_num_minus4 + 4)
    if not sps.frame_mbs_only:
        bw.u(0, 1)  # field_pic_flag
    if sps.pic_order_count_type == 0:
        bw.u(h.pic_order_cnt_lsb, sps.log2_max_pic_order_cnt_lsb_min4 + 4)
        if pps.bottom_field_pic_order_in_frame_present:
            bw.se(h.delta_pic_order_cnt_bottom)
    if sps.pic_order_count_type == 1 and not sps.delta_pic_order_always_zero:
        bw.se(int(h.delta_pic_order_cnt[0]))
        if pps.bottom_field_pic_order_in_frame_present:
            bw.se(int(h.delta_pic_order_cnt[1]))
    if pps.redundant_pic_cnt_present:
        bw.ue(0)
    bw.u(1, 1)  # num_ref_idx_active_override_flag
    bw.ue(0)    # num_ref_idx_l0_active_minus1
    bw.u(0, 1)  # ref_pic_list_modification_flag_l0
    if pps.weighted_pred:  # pred_weight_table(): denominators 0, no flag set
        bw.ue(0)
        if sps.chroma_format != 0:
            bw.ue(0)
        bw.u(0, 1)
        if sps.chroma_format != 0:
            bw.u(0, 1)
    if s.ref_idc:  # dec_ref_pic_marking() of the picture
        bw.u(h.adaptive_ref_pic_marking_mode_flag, 1)
        if h.adaptive_ref_pic_marking_mode_flag:
            for k in range(h.n_memory_management_control_operations):
                op = int(h.memory_management_control_operation[k])
                bw.ue(op)
                if op in (1, 2, 3, 4):
                    bw.ue(int(h.mmco_arg1[k]))
                if op in (3, 6):
                    bw.ue(int(h.mmco_arg2[k]))
            bw.ue(0)
    if pps.entropy_coding_mode:
        bw.ue(0)  # cabac_init_idc
    bw.se(0)      # slice_qp_delta
    if pps.deblocking_filter_control_present:
        bw.ue(0)  # disable_deblocking_filter_idc
        bw.se(0)
        bw.se(0)
    if pps.num_slice_groups_minus1 > 0 and 3 <= pps.slice_group_map_type <= 5:
        units = (sps.pic_width_in_mbs_minus1 + 1) * (sps.pic_height_in_map_units_minus1 + 1)
        rate = pps.slice_group_change_rate_minus1 + 1
        n = 0
        while ((1 << n) - 1) * rate < units:
            n += 1
        bw.u(h.slice_group_change_cycle, n)


def pskip_unit(s, sc):
    """The NAL unit (with start code `sc`) that codes the macroblocks of slice `s` as a P slice of P_Skip macroblocks."""
    bw = _BW()
    _header(bw, s)
    n = len(s.mbs)
    if s.pps.entropy_coding_mode:
        while not bw.aligned():
            bw.u(1, 1)  # cabac_alignment_one_bit
        bw.L.sg_cabac_init_ctx(bw.w, 1, 26 + s.pps.pic_init_qp_minus26)  # P slice, cabac_init_idc 0, SliceQPY of slice_qp_delta 0
        bw.L.sg_cabac_start(bw.w)
        for i in range(n):
            bw.L.sg_cabac_bin(bw.w, 11, 1)  # mb_skip_flag: ctxIdxInc 0 (the neighbours are unavailable or skipped)
            bw.L.sg_cabac_terminate(bw.w, int(i == n - 1))  # end_of_slice_flag
        while not bw.aligned():
            bw.u(0, 1)
    else:
        bw.ue(n)  # mb_skip_run
        bw.L.sg_trailing(bw.w)
    return sc + bytes([(s.ref_idc << 5) | 1]) + escape(bw.bytes())


def zeroed_unit(s, sc):
    """The slice with its header intact and zero bytes for slice data."""
    bw = _BW(ZERO_BYTES + len(s.rbsp) + 64)
    nbits = s.hdr.slice_data_bit_offset
    for i in range(nbits):
        bw.u((s.rbsp[i >> 3] >> (7 - (i & 7))) & 1, 1)
    while not bw.aligned():
        bw.u(1 if s.pps.entropy_coding_mode else 0, 1)
    rbsp = bw.bytes() + bytes(ZERO_BYTES)
    return sc + bytes([(s.ref_idc << 5) | s.type]) + escape(rbsp)


def bad_header_unit(s, sc):
    """A slice NAL unit whose header does not parse: first_mb_in_slice 0, slice_type 20 (7.4.3: 0..9), pic_parameter_set_id 0."""
    return sc + bytes([(s.ref_idc << 5) | s.type]) + b"\x85\x7f"


# ---------------------------------------------------------------- damage
def default_picks(pics):
    """(picture, place) pairs for a stream of 3-4 (or more) slices per picture: the first two slices of picture 1, the last slice of picture 2,
    a middle slice of picture 4 -- whatever the types of those pictures are."""
    picks = [(1, 0), (1, 1), (2, len(pics[2]) - 1)]
    if len(pics) > 4 and pics[4][0].type == 1:
        picks.append((4, 1))
    return picks


def check_picks(pics, picks):
    """The conditions every case of the concealment matrix has to meet, so that none passes by doing little."""
    by_pic = {}
    for p, i in picks:
        assert pics[p][0].type == 1 and not pics[p][0].hdr.field_pic, "only non-IDR frame pictures are concealable"
        by_pic.setdefault(p, set()).add(i)
    assert len(picks) >= 3 and len(by_pic) >= 2
    for p, places in by_pic.items():
        assert len(places) < len(pics[p]), "never all slices of a picture"
    assert any(0 in v for v in by_pic.values()), "a first slice"
    assert any(len(pics[p]) - 1 in v for p, v in by_pic.items()), "a last slice"
    assert any(0 < i < len(pics[p]) - 1 for p, v in by_pic.items() for i in v), "a middle slice"
    assert any(i + 1 in v for v in by_pic.values() for i in v), "two adjacent slices of one picture"
    assert any(p + 1 in by_pic for p in by_pic), "slices of consecutive pictures"
    lost = sum(len(pics[p][i].mbs) for p, i in picks)
    total = sum(s.wmb * s.hmb for s in (p[0] for p in pics))
    assert lost * 20 >= total, "at least 5 %% of the stream's macroblocks (%d of %d)" % (lost, total)


def make(stream, picks=None, mode="lost", check=True, repair=True):
    """(damaged, repaired, per_picture, n_slices): per_picture[p] = macroblocks of picture p that are lost.  repair=False (with picks that need not
    meet the matrix conditions: IDR pictures, field pictures): no repaired stream exists or is wanted, None is returned for it."""
    units, slices, pics = parse(stream)
    if picks is None:
        picks = default_picks(pics)
    if check and repair:
        check_picks(pics, picks)
    damaged, repaired = list(units), list(units)
    per_picture = [0] * len(pics)
    for p, i in picks:
        s = pics[p][i]
        sc = units[s.unit][:_sc_len(units[s.unit])]
        damaged[s.unit] = b"" if mode == "lost" else (bad_header_unit(s, sc) if mode == "header" else zeroed_unit(s, sc))
        if repair:
            repaired[s.unit] = pskip_unit(s, sc)
        per_picture[p] += len(s.mbs)
    return b"".join(damaged), b"".join(repaired) if repair else None, per_picture, len(picks)


def lost_mbs(stream, picks=None):
    """{picture: sorted macroblock addresses} of the picks, and the pictures' (wmb, hmb)."""
    _, _, pics = parse(stream)
    if picks is None:
        picks = default_picks(pics)
    out = {}
    for p, i in picks:
        out.setdefault(p, []).extend(pics[p][i].mbs)
    return {p: sorted(v) for p, v in out.items()}, (pics[0][0].wmb, pics[0][0].hmb)


# ---------------------------------------------------------------- the matrix
B = dict(width=176, height=144, idr_period=0, frames=8)
CONCEAL_MATRIX = {
    # (the first two are the cases with deblock_idc 1 of the CPU copy test: one reference frame, so the concealment reference is the previous picture)
    "cavlc_poc2_idc1": dict(B, profile_idc=66, cabac=0, slices=4, poc_type=2, deblock_idc=1, seed=601),
    "cabac_idc1_qpdelta": dict(B, profile_idc=77, cabac=1, slices=3, deblock_idc=1, slice_qp_delta=4, qp_jitter=3, seed=602),
    "cavlc_idc2_offsets": dict(B, profile_idc=66, cabac=0, slices=4, deblock_idc=2, alpha_off_div2=3, beta_off_div2=-2, intra_in_p_permille=150, seed=603),
    "cabac_idc0_offsets_cqp": dict(B, profile_idc=77, cabac=1, slices=3, deblock_idc=0, alpha_off_div2=-2, beta_off_div2=2, chroma_qp_offset=3, slice_qp_delta=5,
                                   cabac_init_idc=-1, seed=604),
    "cabac_wp1_multiref": dict(B, frames=10, profile_idc=77, cabac=1, slices=3, weighted_pred=1, num_ref_frames=3, seed=605),
    "cavlc_wp2_rplm_mmco": dict(B, frames=12, profile_idc=77, cabac=0, slices=4, weighted_pred=2, num_ref_frames=3, rplm=1, mmco=1, qp=30, seed=606),
    "cabac_rplm_mmco_nonref": dict(B, frames=12, profile_idc=77, cabac=1, slices=3, num_ref_frames=4, rplm=1, mmco=1, nonref_period=3, poc_type=1, qp=30, seed=607),
    "cabac_cip_intra": dict(B, profile_idc=77, cabac=1, slices=4, constrained_intra=1, intra_in_p_permille=300, deblock_idc=2, seed=608),
    "high8x8_cabac_idc2": dict(B, profile_idc=100, cabac=1, transform8x8=1, slices=3, deblock_idc=2, alpha_off_div2=1, beta_off_div2=1, sub8x8_permille=300, seed=609),
    "b_ibbp_cabac_implicit": dict(B, frames=10, profile_idc=77, cabac=1, slices=3, bframes=2, num_ref_frames=3, weighted_bipred=2, bskip_permille=200, seed=610),
    "b_ibbp_cavlc_explicit": dict(B, frames=10, profile_idc=77, cabac=0, slices=4, bframes=2, num_ref_frames=3, weighted_bipred=1, weighted_pred=1, deblock_idc=2, seed=611),
    "b_pyramid_cabac": dict(B, frames=12, profile_idc=77, cabac=1, slices=3, bframes=3, b_pyramid=1, bskip_permille=300, sub8x8_permille=200, seed=612),
    "b_temporal_cavlc": dict(B, frames=10, profile_idc=77, cabac=0, slices=3, bframes=2, num_ref_frames=2, direct_temporal=1, bskip_permille=300, seed=613),
    "fmo_dispersed_aso": dict(B, profile_idc=66, cabac=0, slice_groups=2, fmo_type=1, slices=2, aso=1, intra_in_p_permille=150, seed=614),
    "fmo_boxout_aso_idc2": dict(B, profile_idc=66, cabac=0, slice_groups=2, fmo_type=3, slices=2, aso=1, deblock_idc=2, num_ref_frames=2, seed=615),
    "cropped_cabac": dict(B, width=200, height=150, profile_idc=100, cabac=1, transform8x8=1, slices=3, long_start_code=0, seed=616),
    "mono_cabac_wp": dict(B, profile_idc=100, mono=1, cabac=1, transform8x8=1, slices=3, weighted_pred=1, num_ref_frames=2, seed=617),
    "mono_cavlc": dict(B, profile_idc=100, mono=1, cabac=0, slices=4, num_ref_frames=2, deblock_idc=0, intra_in_p_permille=200, seed=618),
}


def nslices(kw):
    return max(1, kw.get("slices", 1)) * max(1, kw.get("slice_groups", 1))
