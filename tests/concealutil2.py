"""Yardstick of the tests of wholly lost pictures (H264MI_CONCEAL_PICTURES): removes whole pictures from generator streams and writes the REPAIRED
stream the rule is stated in (include/h264mi.h, h264mi_config.conceal_errors).

In the repaired stream every missing reference frame is coded, in front of the first slice NAL unit of the picture that reveals the gap, as a frame of
nal_unit_type 1 / nal_ref_idc 1 with one P slice of P_Skip macroblocks per slice group -- the slice writer is concealutil.pskip_unit, fed a header made
up here.  The writer takes only what a decoder can know: the first slice it sees of the revealing picture, and PrevRefFrameNum / prevPicOrderCntLsb as
they stand in front of the gap.  It never looks at the lost pictures."""
import numpy as np

import concealutil as cu
import h264decode_amd as H

MAX_GAP = 16  # H264MI_CONCEAL_MAX_GAP


def _copy_header(h):
    c = type(h._c).from_buffer_copy(h._c)
    return H.SliceHeader(c)


def missing_frame_units(rev, frame_num, poc_lsb):
    """The NAL units of one missing frame: `rev` is the first slice (concealutil.SliceInfo) the decoder sees of the revealing picture."""
    sps, pps = rev.sps, rev.pps
    base = _copy_header(rev.hdr)
    c = base._c
    c.frame_num, c.field_pic, c.bottom_field = frame_num, 0, 0
    c.pic_order_cnt_lsb, c.delta_pic_order_cnt_bottom = poc_lsb, 0
    c.delta_pic_order_cnt[0] = c.delta_pic_order_cnt[1] = 0
    c.adaptive_ref_pic_marking_mode_flag = c.n_memory_management_control_operations = 0  # sliding window
    total = sps.pic_width_in_mbs * sps.pic_height_in_mbs
    sgmap = H.MbToSliceGroupMap(sps, pps, base) if pps.num_slice_groups_minus1 > 0 else np.zeros(total, dtype=np.uint8)
    assert len(sgmap) == total
    unit = rev.units[rev.unit]
    sc = unit[:cu._sc_len(unit)]
    out = []
    for grp in sorted(set(int(g) for g in sgmap)):  # one slice per slice group: a single slice over a picture with slice groups is not a valid stream
        s = cu.SliceInfo()
        s.hdr = _copy_header(base)
        s.mbs = [a for a in range(total) if sgmap[a] == grp]
        s.hdr._c.first_mb_in_slice = s.mbs[0]
        s.sps, s.pps, s.ref_idc, s.type = sps, pps, 1, 1
        out.append(cu.pskip_unit(s, sc))
    return b"".join(out)


def _has_op5(s):
    h = s.hdr
    return s.ref_idc and s.type != 5 and h.adaptive_ref_pic_marking_mode_flag and 5 in [int(h.memory_management_control_operation[k]) for k in range(h.n_memory_management_control_operations)]


def frame_index(pics):
    """[picture] -> index of the frame it belongs to (the second field of a frame shares its first field's), in decoding order."""
    out, n = [], -1
    for p, sl in enumerate(pics):
        h = sl[0].hdr
        second = False
        if p and h.field_pic and sl[0].type != 5 and out and out[-1] == n:
            q = pics[p - 1][0].hdr
            alone = p < 2 or out[p - 2] != out[p - 1]  # (the picture before is not already a second field)
            second = bool(q.field_pic) and q.bottom_field != h.bottom_field and q.frame_num == h.frame_num and alone
        if not second:
            n += 1
        out.append(n)
    return out


class Lost:
    """What lose_pictures() did: damaged / repaired streams, and per FRAME of the repaired stream (decoding order) `inserted` (bool), `frame_num`,
    `copy_of` (for an inserted frame: the frame it is a copy of -- the reference frame decoded last before it), `new_seq`; `mbs` per frame."""


def lose_pictures(stream, lost):
    """Removes the pictures `lost` (indices in decoding order; both fields of a frame coded as two fields) and repairs every run of them."""
    units, slices, pics = cu.parse(stream)
    for s in slices:
        s.units = units
    lost = sorted(set(lost))
    damaged, repaired = list(units), list(units)
    for p in lost:
        assert 0 < p < len(pics) - 1 and pics[p][0].type == 1 and pics[p][0].ref_idc, "a non-IDR reference picture with a picture behind it"
        assert not _has_op5(pics[p][0]), "the lost picture carried operation 5: the repaired stream is another stream"
        for s in pics[p]:
            damaged[s.unit] = repaired[s.unit] = b""
    fidx = frame_index(pics)
    n_inserted = {}  # revealing picture -> number of frames in front of it
    p = 0
    while p < len(pics):
        if p not in lost:
            p += 1
            continue
        a = p
        while p in lost:
            p += 1
        rev = min(pics[p], key=lambda s: s.unit)  # the first slice the decoder sees (arbitrary slice order: not the one of macroblock 0)
        prev = next(pics[q][0] for q in range(a - 1, -1, -1) if pics[q][0].ref_idc)  # the previous reference picture in decoding order
        sps = rev.sps
        prev_fn, prev_lsb = prev.hdr.frame_num, prev.hdr.pic_order_cnt_lsb
        if _has_op5(prev):  # 7.4.3 / 8.2.1.1: the picture counts as one with frame_num 0, and prevPicOrderCntLsb is its TopFieldOrderCnt after the reset (0: top field first)
            assert not prev.hdr.field_pic and prev.hdr.delta_pic_order_cnt_bottom >= 0
            prev_fn = prev_lsb = 0
        max_fn, max_lsb = 1 << (sps.log2_max_frame_num_minus4 + 4), 1 << (sps.log2_max_pic_order_cnt_lsb_min4 + 4)
        assert not sps.gaps_in_frame_num_value_allowed and rev.type != 5
        m = (rev.hdr.frame_num - prev_fn - 1) % max_fn
        assert 0 < m, "no gap: only non-reference pictures were lost"
        new = [missing_frame_units(rev, (prev_fn + 1 + k) % max_fn, (prev_lsb + 2 * (k + 1)) % max_lsb) for k in range(m)]
        repaired[rev.unit] = b"".join(new) + units[rev.unit]
        n_inserted[p] = (m, prev_fn, max_fn)
    r = Lost()
    r.damaged, r.repaired = b"".join(damaged), b"".join(repaired)
    r.n_pictures, r.n_lost = len(pics), len(lost)
    r.inserted, r.frame_num, r.copy_of, r.new_seq, r.ref = [], [], [], [], []
    last_ref = None
    seen = set()
    for p, sl in enumerate(pics):
        if p in lost:
            continue
        m, prev_fn, max_fn = n_inserted.get(p, (0, 0, 1))
        for k in range(m):
            r.inserted.append(True), r.copy_of.append(last_ref), r.new_seq.append(False), r.ref.append(True)
            r.frame_num.append((prev_fn + 1 + k) % max_fn)
            last_ref = len(r.inserted) - 1
        if fidx[p] in seen:  # second field
            continue
        seen.add(fidx[p])
        r.inserted.append(False), r.copy_of.append(None), r.frame_num.append(sl[0].hdr.frame_num), r.ref.append(bool(sl[0].ref_idc))
        r.new_seq.append(sl[0].type == 5 or bool(_has_op5(sl[0])))
        if sl[0].ref_idc:
            last_ref = len(r.inserted) - 1
    r.first_touched = r.inserted.index(True)
    r.mbs = pics[0][0].sps.pic_width_in_mbs * pics[0][0].sps.pic_height_in_mbs
    return r


def check_lost(r, pocs):
    """The conditions every case of the matrix has to meet (on the oracle's PicOrderCnt list of the repaired stream), so that none passes by doing little."""
    assert len(pocs) == len(r.inserted)
    cur = set()
    for i, poc in enumerate(pocs):
        if r.new_seq[i]:
            cur = set()
        assert int(poc) not in cur, "two pictures of one coded video sequence have PicOrderCnt %d" % poc
        cur.add(int(poc))
    assert r.n_lost * 20 >= r.n_pictures, "at least 5 %% of the stream's pictures (%d of %d)" % (r.n_lost, r.n_pictures)


# ---------------------------------------------------------------- the cases: name -> (generator recipe, lost pictures)
B = cu.B
P_ONLY = ("cabac_cip_intra", "cabac_idc0_offsets_cqp", "cabac_idc1_qpdelta", "cabac_wp1_multiref", "cavlc_idc2_offsets", "cavlc_poc2_idc1", "cavlc_wp2_rplm_mmco",
          "cropped_cabac", "fmo_boxout_aso_idc2", "fmo_dispersed_aso", "high8x8_cabac_idc2", "mono_cabac_wp", "mono_cavlc")
# the matrix: recipes of concealutil.CONCEAL_MATRIX; every case has to meet check_lost()
MATRIX_CASES = {name + "_2_3": (cu.CONCEAL_MATRIX[name], [2, 3]) for name in P_ONLY}  # two consecutive losses
MATRIX_CASES.update({
    "cabac_rplm_mmco_nonref_3": (cu.CONCEAL_MATRIX["cabac_rplm_mmco_nonref"], [3]),
    "b_pyramid_cabac_10": (cu.CONCEAL_MATRIX["b_pyramid_cabac"], [10]),
})
PAFF = dict(width=176, height=128, frames=6, idr_period=0, profile_idc=77, field_pics=1, cabac=0, slices=2, num_ref_frames=2, seed=316)
OTHER_CASES = {
    # one slice per picture, the shape of real streams: a lost NAL unit is a lost picture
    "one_slice_main_cabac_3": (dict(B, profile_idc=77, cabac=1, slices=1, seed=701), [3]),
    "one_slice_mono_high_1_2": (dict(B, profile_idc=100, mono=1, cabac=1, transform8x8=1, slices=1, num_ref_frames=2, seed=705), [1, 2]),  # directly behind the IDR picture
    # (picture order count type 1 with the generator's cycle: the inserted frames, coded with both deltas 0, land on counts other pictures have)
    "two_slices_poc1_wp_2_5_6": (dict(B, frames=10, poc_type=1, weighted_pred=1, num_ref_frames=3, slices=2, seed=703), [2, 5, 6]),
    # PAFF: both fields of the frame with frame_num 2 (pictures 4 and 5); the inserted picture is a frame picture
    "paff_cavlc": (PAFF, [4, 5]),
    "paff_cabac_bottom_first": (dict(PAFF, field_pics=2, cabac=1, seed=317), [4, 5]),
    # A recipe of the matrix, but outside it: the frame inserted for picture 6 gets PicOrderCnt 2 (picture order count type 1, both deltas 0), which
    # the non-reference picture 5 in front of it has as well, so check_lost()'s "no two pictures of a sequence share a PicOrderCnt" does not
    # hold.  The stream has no B pictures: nothing depends on the counts.
    "cabac_rplm_mmco_nonref_6": (cu.CONCEAL_MATRIX["cabac_rplm_mmco_nonref"], [6]),
}
CASES = dict(MATRIX_CASES, **OTHER_CASES)


def access_units(stream):
    """The stream cut in front of every picture's first unit (parameter sets stay with the picture they precede)."""
    units, slices, pics = cu.parse(stream)
    first_unit = sorted(min(s.unit for s in p) for p in pics)
    cuts = [0]
    for u in first_unit[1:]:
        while u > 0 and (units[u - 1][cu._sc_len(units[u - 1])] & 31) in (7, 8):
            u -= 1
        cuts.append(u)
    cuts.append(len(units))
    return [b"".join(units[a:b]) for a, b in zip(cuts, cuts[1:])]


# ================================================================ field pictures (H264MI_CONCEAL_FIELDS)
def slice_header(bw, s):
    """slice_header() (7.3.3) of the replacement P slice of `s`, frame or field picture: concealutil._header plus field_pic_flag / bottom_field_flag,
    and without delta_pic_order_cnt_bottom / delta_pic_order_cnt[1] in a field (they are present only when field_pic_flag is 0)."""
    h, sps, pps = s.hdr, s.sps, s.pps
    assert not sps.use_separate_color_plane and s.type == 1
    field = bool(h.field_pic)
    assert not field or not sps.frame_mbs_only
    bw.ue(h.first_mb_in_slice)
    bw.ue(0)  # slice_type P
    bw.ue(h.pps_id)
    bw.u(h.frame_num, sps.log2_max_frame_num_minus4 + 4)
    if not sps.frame_mbs_only:
        bw.u(int(field), 1)  # field_pic_flag
        if field:
            bw.u(int(h.bottom_field), 1)
    if sps.pic_order_count_type == 0:
        bw.u(h.pic_order_cnt_lsb, sps.log2_max_pic_order_cnt_lsb_min4 + 4)
        if pps.bottom_field_pic_order_in_frame_present and not field:
            bw.se(h.delta_pic_order_cnt_bottom)
    if sps.pic_order_count_type == 1 and not sps.delta_pic_order_always_zero:
        bw.se(int(h.delta_pic_order_cnt[0]))
        if pps.bottom_field_pic_order_in_frame_present and not field:
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
    """concealutil.pskip_unit with the field-aware header."""
    bw = cu._BW()
    slice_header(bw, s)
    n = len(s.mbs)
    if s.pps.entropy_coding_mode:
        while not bw.aligned():
            bw.u(1, 1)  # cabac_alignment_one_bit
        bw.L.sg_cabac_init_ctx(bw.w, 1, 26 + s.pps.pic_init_qp_minus26)
        bw.L.sg_cabac_start(bw.w)
        for i in range(n):
            bw.L.sg_cabac_bin(bw.w, 11, 1)  # mb_skip_flag, ctxIdxInc 0
            bw.L.sg_cabac_terminate(bw.w, int(i == n - 1))  # end_of_slice_flag
        while not bw.aligned():
            bw.u(0, 1)
    else:
        bw.ue(n)  # mb_skip_run
        bw.L.sg_trailing(bw.w)
    return sc + bytes([(s.ref_idc << 5) | 1]) + cu.escape(bw.bytes())


def field_picks(pics):
    """(picture, place) pairs for a PAFF stream of three slices per field whose frames are all field pairs (pictures 2k, 2k + 1): a slice of the second
    field of the IDR frame, a first, a middle and a last slice, two adjacent slices, in both parities, slices of consecutive pictures."""
    picks = [(1, 1), (2, 0), (3, 1), (3, 2), (4, 2)]
    if len(pics) > 7:
        picks.append((7, 0))
    return picks


def check_field_picks(pics, picks):
    by_pic = {}
    for p, i in picks:
        s = pics[p][0]
        assert s.type == 1 and s.hdr.field_pic, "only non-IDR field pictures"
        by_pic.setdefault(p, set()).add(i)
    assert len(picks) >= 5
    for p, places in by_pic.items():
        assert len(places) < len(pics[p]), "never all slices of a picture"
    assert any(pics[p - 1][0].type == 5 for p in by_pic), "a slice of the second field of the IDR frame"
    for par in (0, 1):
        mine = {p: v for p, v in by_pic.items() if bool(pics[p][0].hdr.bottom_field) == bool(par)}
        assert mine, "both parities"
    assert any(0 in v for v in by_pic.values()), "a first slice"
    assert any(len(pics[p]) - 1 in v for p, v in by_pic.items()), "a last slice"
    assert any(0 < i < len(pics[p]) - 1 for p, v in by_pic.items() for i in v), "a middle slice"
    assert any(i + 1 in v for v in by_pic.values() for i in v), "two adjacent slices of one picture"
    assert any(p + 1 in by_pic for p in by_pic), "slices of consecutive pictures"
    lost = sum(len(pics[p][i].mbs) for p, i in picks)
    total = sum(s.wmb * s.hmb for s in (p[0] for p in pics))
    assert lost * 20 >= total, "at least 5 %% of the stream's macroblocks (%d of %d)" % (lost, total)


def make_fields(stream, picks=None, mode="lost"):
    """concealutil.make for field pictures: (damaged, repaired, per_frame, n_slices); per_frame[f] = lost macroblocks of frame f (both fields)."""
    units, slices, pics = cu.parse(stream)
    if picks is None:
        picks = field_picks(pics)
    check_field_picks(pics, picks)
    fidx = frame_index(pics)
    damaged, repaired = list(units), list(units)
    per_frame = [0] * (fidx[-1] + 1)
    for p, i in picks:
        s = pics[p][i]
        sc = units[s.unit][:cu._sc_len(units[s.unit])]
        damaged[s.unit] = b"" if mode == "lost" else (cu.bad_header_unit(s, sc) if mode == "header" else cu.zeroed_unit(s, sc))
        repaired[s.unit] = pskip_unit(s, sc)
        per_frame[fidx[p]] += len(s.mbs)
    return b"".join(damaged), b"".join(repaired), per_frame, len(picks)


FB = dict(width=176, height=128, frames=5, idr_period=0, profile_idc=77, field_pics=1, slices=3)
FIELD_CASES = {
    "field_cavlc_refs2_idc2": dict(FB, cabac=0, num_ref_frames=2, deblock_idc=2, alpha_off_div2=2, beta_off_div2=-1, seed=306),
    "field_cabac_refs2": dict(FB, cabac=1, num_ref_frames=2, seed=307),
    "field_b_cavlc": dict(FB, frames=7, cabac=0, bframes=1, num_ref_frames=2, seed=308),
    "field_bottom_first_refs3_idc1": dict(FB, cabac=0, field_pics=2, num_ref_frames=3, deblock_idc=1, sub8x8_permille=300, seed=331),
    "field_cabac_bottom_first_wp1": dict(FB, cabac=1, field_pics=2, weighted_pred=1, num_ref_frames=1, seed=332),
    "field_cavlc_wp2_ref1_qpdelta": dict(FB, cabac=0, weighted_pred=2, num_ref_frames=1, slice_qp_delta=4, qp_jitter=3, seed=333),
    "field_b_cabac_bottom_first_implicit": dict(FB, frames=7, cabac=1, field_pics=2, bframes=2, num_ref_frames=3, weighted_bipred=2, bskip_permille=250, seed=334),
    "field_high8x8_cabac_intra_idc0": dict(FB, profile_idc=100, transform8x8=1, cabac=1, num_ref_frames=2, intra_in_p_permille=250, deblock_idc=0, alpha_off_div2=-2, beta_off_div2=2,
                                           chroma_qp_offset=3, seed=335),
    "field_mono_cavlc_poc2": dict(FB, profile_idc=100, mono=1, cabac=0, num_ref_frames=2, poc_type=2, seed=336),
}
