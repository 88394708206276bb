"""Yardstick of the tests of concealed IDR pictures (H264MI_CONCEAL_IDR): damages slices of IDR frame pictures of generator streams and writes the
REPAIRED stream the rule is stated in (include/h264mi.h, h264mi_config.conceal_errors).

In the repaired stream a damaged IDR picture X is a NON-IDR picture that ends in memory management operation 5: every slice NAL unit of X has
nal_unit_type 1 (nal_ref_idc unchanged), every slice header of X carries frame_num F' = (PrevRefFrameNum + 1) mod MaxFrameNum, no idr_pic_id and a
dec_ref_pic_marking() of adaptive_ref_pic_marking_mode_flag 1, operation 5, end code 0.  Operation 5 takes effect after the picture is decoded, so X
predicts from the references the IDR picture would have dropped and leaves behind exactly the state an IDR picture leaves.  The intact I slices keep
every other header field and their slice data (slice_type 7 is written as 2: the picture holds P slices now); each lost slice is a P slice of P_Skip
macroblocks written by concealutil.pskip_unit from a header with the same frame_num and marking.  Picks in other pictures of the stream (non-IDR
frame pictures) are repaired as concealutil.make repairs them, so one stream can carry both kinds of damage.

`make(stream, picks, mode)` returns the damaged stream (modes as in concealutil.make), the repaired one and the stream in which X is only
relabelled (no slice lost: it must decode exactly like the original)."""
import concealutil as cu
import concealutil2 as c2


# ---------------------------------------------------------------- writers
def _x_header(bw, s, frame_num):
    """slice_header() (7.3.3) of an intact I slice `s` of X in the repaired stream: nal_unit_type 1, frame_num F', no idr_pic_id, operation 5."""
    h, sps, pps = s.hdr, s.sps, s.pps
    assert not sps.use_separate_color_plane and not h.field_pic and s.type == 5 and h.slice_type % 5 == 2 and s.ref_idc
    bw.ue(h.first_mb_in_slice)
    bw.ue(2)  # slice_type I: not 7, the picture holds P slices too
    bw.ue(h.pps_id)
    bw.u(frame_num, sps.log2_max_frame_num_minus4 + 4)
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
    bw.u(1, 1)  # dec_ref_pic_marking(): adaptive_ref_pic_marking_mode_flag
    bw.ue(5)    # memory_management_control_operation 5
    bw.ue(0)    # end
    bw.se(h.slice_qp_delta)
    if pps.deblocking_filter_control_present:
        bw.ue(h.disable_deblocking_filter)
        if h.disable_deblocking_filter != 1:
            bw.se(h.slice_alpha_c0_offset_div2)
            bw.se(h.slice_beta_offset_div2)
    if pps.num_slice_groups_minus1 > 0 and 3 <= pps.slice_group_map_type <= 5:
        units = (sps.pic_width_in_mbs_minus1 + 1) * (sps.pic_height_in_map_units_minus1 + 1)
        rate = pps.slice_group_change_rate_minus1 + 1
        n = 0
        while ((1 << n) - 1) * rate < units:
            n += 1
        bw.u(h.slice_group_change_cycle, n)


def _bit(rbsp, i):
    return (rbsp[i >> 3] >> (7 - (i & 7))) & 1


def relabelled_unit(s, sc, frame_num):
    """The intact I slice `s` of X as the repaired stream carries it: the new header, the slice data unchanged."""
    rbsp = s.rbsp
    bw = cu._BW(len(rbsp) + 256)
    _x_header(bw, s, frame_num)
    off = s.hdr.slice_data_bit_offset
    if s.pps.entropy_coding_mode:
        # the parsed offset points in front of the cabac_alignment_one_bits: the arithmetic code starts at the next byte boundary, and is copied bytewise
        while not bw.aligned():
            bw.u(1, 1)
        out = bw.bytes() + bytes(rbsp[(off + 7) // 8:])
    else:
        n = len(rbsp)
        while n > 0 and rbsp[n - 1] == 0:
            n -= 1
        stop = (n - 1) * 8 + 7 - ((rbsp[n - 1] & -rbsp[n - 1]).bit_length() - 1)  # rbsp_stop_one_bit: the last 1 bit
        assert off <= stop
        for i in range(off, stop):
            bw.u(_bit(rbsp, i), 1)
        bw.L.sg_trailing(bw.w)  # (the bit writer hands out whole bytes only: without new trailing bits the tail would be lost)
        out = bw.bytes()
    return sc + bytes([(s.ref_idc << 5) | 1]) + cu.escape(out)


def x_pskip_unit(s, sc, frame_num):
    """The lost slice `s` of X as the repaired stream carries it: concealutil.pskip_unit over the same macroblocks, frame_num F' and operation 5."""
    r = cu.SliceInfo()
    r.hdr = c2._copy_header(s.hdr)
    c = r.hdr._c
    c.frame_num = frame_num
    c.adaptive_ref_pic_marking_mode_flag, c.n_memory_management_control_operations = 1, 1
    c.memory_management_control_operation[0] = 5
    r.sps, r.pps, r.ref_idc, r.type, r.mbs = s.sps, s.pps, s.ref_idc, 1, s.mbs
    return cu.pskip_unit(r, sc)


def frame_num_of_x(pics, p):
    """F' of the IDR picture p: (PrevRefFrameNum + 1) mod MaxFrameNum, from the reference picture decoded last before it."""
    prev = next(pics[q][0] for q in range(p - 1, -1, -1) if pics[q][0].ref_idc)
    prev_fn = 0 if prev.type == 5 or c2._has_op5(prev) else prev.hdr.frame_num
    return (prev_fn + 1) % (1 << (pics[p][0].sps.log2_max_frame_num_minus4 + 4))


# ---------------------------------------------------------------- damage
def resolve(pics, spec):
    """Picks given relative to the IDR pictures of the stream -> (picture, place): ("idr", k, place) a slice of the k-th IDR picture (k = 0: the stream's
    first picture); ("p", k, j, place) a slice of the j-th picture behind the k-th IDR picture in decoding order, a non-IDR picture of its GOP.
    place < 0 counts from the last slice."""
    idrs = [p for p, sl in enumerate(pics) if sl[0].type == 5]
    out = []
    for e in spec:
        p = idrs[e[1]] + (e[2] if e[0] == "p" else 0)
        assert (pics[p][0].type == 5) == (e[0] == "idr") and (e[0] == "idr" or p < (idrs + [len(pics)])[e[1] + 1])
        place = e[-1]
        out.append((p, place if place >= 0 else len(pics[p]) + place))
    return out


def check_case(pics, picks):
    """The conditions every case has to meet, so that none passes by doing little."""
    by_pic = {}
    for p, i in picks:
        assert p > 0, "picture 0 is never picked"
        assert not pics[p][0].hdr.field_pic
        by_pic.setdefault(p, set()).add(i)
    xs = [p for p in by_pic if pics[p][0].type == 5]
    assert xs, "at least one slice of an IDR picture"
    for p, places in by_pic.items():
        assert len(places) < len(pics[p]), "never all slices of a picture"
    for p in xs:
        lost = sum(len(pics[p][i].mbs) for i in by_pic[p])
        assert lost * 10 >= pics[p][0].wmb * pics[p][0].hmb, "at least 10 %% of X (%d macroblocks)" % lost
    return by_pic, xs


def gop_of(pics, p):
    """The index of the IDR picture that opens the GOP of picture p."""
    while pics[p][0].type != 5:
        p -= 1
    return p


def check_matrix(resolved):
    """Over the matrix ([(pics, picks)]): a first, a middle and a last slice of an IDR picture, two adjacent slices of one, two damaged IDR pictures in
    one stream, and in at least two cases a pick in a P picture of the damaged GOP too."""
    first = middle = last = adjacent = two = with_p = 0
    for pics, picks in resolved:
        by_pic, xs = check_case(pics, picks)
        for p in xs:
            v, n = by_pic[p], len(pics[p])
            first += 0 in v
            last += n - 1 in v
            middle += any(0 < i < n - 1 for i in v)
            adjacent += any(i + 1 in v for i in v)
        two += len(xs) >= 2
        with_p += any(pics[p][0].type != 5 and gop_of(pics, p) in xs for p in by_pic)
    assert first and middle and last, "a first, a middle and a last slice of an IDR picture"
    assert adjacent, "two adjacent slices of one IDR picture"
    assert two, "two damaged IDR pictures in one stream"
    assert with_p >= 2, "a pick in a P picture of the same GOP, in two cases"


class Made:
    """What make() did: `damaged`, `repaired`, `relabelled` streams; per picture in decoding order `per_picture` (lost macroblocks); `n_slices` picked;
    `xs` the damaged IDR pictures; `pics` the parsed original."""


def make(stream, spec, mode="lost", check=True):
    units, slices, pics = cu.parse(stream)
    picks = resolve(pics, spec)
    by_pic = {}
    for p, i in picks:
        by_pic.setdefault(p, set()).add(i)
    xs = sorted(p for p in by_pic if pics[p][0].type == 5)
    if check:
        check_case(pics, picks)
    damaged, repaired, relabelled = list(units), list(units), list(units)
    per_picture = [0] * len(pics)
    for p, places in by_pic.items():
        fn = frame_num_of_x(pics, p) if p in xs else None
        for i, s in enumerate(pics[p]):
            sc = units[s.unit][:cu._sc_len(units[s.unit])]
            if p in xs:
                relabelled[s.unit] = relabelled_unit(s, sc, fn)
            if i in places:
                damaged[s.unit] = b"" if mode == "lost" else (cu.bad_header_unit(s, sc) if mode == "header" else cu.zeroed_unit(s, sc))
                repaired[s.unit] = x_pskip_unit(s, sc, fn) if p in xs else cu.pskip_unit(s, sc)
                per_picture[p] += len(s.mbs)
            elif p in xs:
                repaired[s.unit] = relabelled[s.unit]
    m = Made()
    m.damaged, m.repaired, m.relabelled = b"".join(damaged), b"".join(repaired), b"".join(relabelled)
    m.per_picture, m.n_slices, m.xs, m.pics, m.picks = per_picture, len(picks), xs, pics, picks
    m.lost = {p: sorted(a for i in v for a in pics[p][i].mbs) for p, v in by_pic.items()}
    return m


# ---------------------------------------------------------------- the matrix: name -> (generator recipe, picks as resolve() reads them)
B = dict(width=176, height=144)
IDR_MATRIX = {
    # the six recipes the rule was tried on, X the second IDR picture
    "cabac_main": (dict(B, frames=9, idr_period=4, profile_idc=77, cabac=1, slices=3, seed=701), [("idr", 1, 0)]),
    "cavlc_poc2_idc2": (dict(B, frames=9, idr_period=3, profile_idc=66, cabac=0, slices=4, poc_type=2, deblock_idc=2, seed=702), [("idr", 1, 1), ("idr", 1, 2), ("p", 1, 1, 0)]),
    "cabac_b_multiref": (dict(B, frames=10, idr_period=6, profile_idc=77, cabac=1, slices=3, bframes=2, num_ref_frames=3, seed=703), [("idr", 1, -1)]),
    "cavlc_poc1": (dict(B, frames=9, idr_period=4, profile_idc=77, cabac=0, slices=3, poc_type=1, seed=704), [("idr", 1, 1), ("idr", 2, 0)]),
    "high8x8_mmco_rplm_wp": (dict(B, frames=10, idr_period=4, profile_idc=100, cabac=1, transform8x8=1, slices=3, mmco=1, rplm=1, weighted_pred=1, num_ref_frames=3, seed=705),
                             [("idr", 1, 0), ("idr", 1, 1), ("p", 1, 2, -1)]),
    "fmo_dispersed_aso": (dict(B, frames=9, idr_period=4, profile_idc=66, cabac=0, slice_groups=2, fmo_type=1, slices=2, aso=1, seed=706), [("idr", 1, 2), ("p", 0, 2, 1)]),
    # the copy test's cases: deblock_idc 1 in the intact slices, only IDR picks in the damaged GOP
    "cavlc_idc1": (dict(B, frames=9, idr_period=3, profile_idc=66, cabac=0, slices=4, deblock_idc=1, seed=707), [("idr", 1, 1), ("idr", 1, 2), ("idr", 2, -1)]),
    "cabac_idc1_wp2_3byte_sc": (dict(B, frames=9, idr_period=4, profile_idc=77, cabac=1, slices=3, deblock_idc=1, weighted_pred=2, long_start_code=0, slice_qp_delta=3, seed=708),
                                [("idr", 1, 1), ("idr", 1, 2)]),
    "cropped_cabac_idc0_offsets": (dict(width=200, height=150, frames=10, idr_period=5, profile_idc=100, cabac=1, transform8x8=1, slices=3, deblock_idc=0, alpha_off_div2=2,
                                        beta_off_div2=-1, long_start_code=0, seed=709), [("idr", 1, 1)]),
    "mono_cavlc_b_spatial": (dict(B, frames=12, idr_period=4, profile_idc=100, mono=1, cabac=0, slices=3, bframes=1, num_ref_frames=2, seed=710), [("idr", 1, 0), ("idr", 2, 2)]),
}
COPY_CASES = ("cavlc_idc1", "cabac_idc1_wp2_3byte_sc")
HEADER_CASES = ("cabac_main", "cavlc_idc1", "fmo_dispersed_aso")  # mode "header" runs on these


def nslices(kw):
    return cu.nslices(kw)
