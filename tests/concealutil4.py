"""Yardstick of the tests of wholly lost FIELDS (H264MI_CONCEAL_LONE_FIELDS): removes whole field pictures from PAFF generator streams and writes the
REPAIRED stream the rule is stated in (include/h264mi.h, h264mi_config.conceal_errors).

A first field F is lone when what follows it is not its second field: another picture, or an end-of-sequence / end-of-stream NAL unit.  In the
repaired stream the missing field F' is coded in front of that unit as one P slice of P_Skip macroblocks per slice group (concealutil2.pskip_unit, fed a
header made up here): nal_unit_type 1, F's nal_ref_idc, pic_parameter_set_id, slice_group_change_cycle and frame_num, the opposite bottom_field_flag,
pic_order_cnt_lsb = F's + 1 / delta_pic_order_cnt[0] = 0, sliding-window marking.  The writer takes only what a decoder can know: it walks the pictures
that are left with the second-field test of 7.4.1.2.4 and never looks at a lost one.  Beside the streams it keeps a model of the frames of the repaired
stream -- which fields each holds, which were inserted, and which field entry 0 of the initial P list for fields (8.2.4.2.5) of an inserted field is
(streams without marking operations and list modification: the window holds the last max_num_ref_frames reference frames) --, so that a test can state
"F' is a copy of that field" on the oracle's frames in numpy."""
import numpy as np

import concealutil as cu
import concealutil2 as c2
import h264decode_amd as H

SLICES, PICTURES, FIELDS, LONE = 1, 2, 4, 64  # H264MI_CONCEAL_*
EOS = b"\x00\x00\x01\x0a"  # an end-of-sequence NAL unit


def _nal_type(unit):
    return unit[cu._sc_len(unit)] & 31


def field_units(F, units):
    """The NAL units of the field that completes the frame of F (concealutil.SliceInfo: the first slice the decoder sees of the lone field)."""
    sps, pps = F.sps, F.pps
    base = c2._copy_header(F.hdr)
    c = base._c
    assert c.field_pic and not sps.frame_mbs_only
    c.bottom_field = 0 if F.hdr.bottom_field else 1
    c.pic_order_cnt_lsb = (F.hdr.pic_order_cnt_lsb + 1) % (1 << (sps.log2_max_pic_order_cnt_lsb_min4 + 4))
    c.delta_pic_order_cnt_bottom = 0
    c.delta_pic_order_cnt[0] = c.delta_pic_order_cnt[1] = 0
    c.adaptive_ref_pic_marking_mode_flag = c.n_memory_management_control_operations = 0  # sliding window
    total = sps.pic_width_in_mbs * (sps.pic_height_in_mbs // 2)
    sgmap = H.MbToSliceGroupMap(sps, pps, base) if pps.num_slice_groups_minus1 > 0 else np.zeros(total, dtype=np.uint8)
    assert len(sgmap) == total
    unit = units[F.unit]
    sc = unit[:cu._sc_len(unit)]
    out = []
    for grp in sorted(set(int(g) for g in sgmap)):
        s = cu.SliceInfo()
        s.hdr = c2._copy_header(base)
        s.mbs = [a for a in range(total) if sgmap[a] == grp]
        s.hdr._c.first_mb_in_slice = s.mbs[0]
        s.sps, s.pps, s.ref_idc, s.type = sps, pps, F.ref_idc, 1
        out.append(c2.pskip_unit(s, sc))
    return b"".join(out)


def _is_second(F, s):
    """The second-field test (7.4.1.2.4, 3.30): `s` is the first slice of the picture that follows the first field F."""
    h = s.hdr
    return bool(h.field_pic) and s.type != 5 and bool(h.bottom_field) != bool(F.hdr.bottom_field) and h.frame_num == F.hdr.frame_num and bool(s.ref_idc) == bool(F.ref_idc)


class Lone:
    """What make_lone() did.  damaged / repaired: the streams.  frames: one dict per frame of the REPAIRED stream in decoding order -- frame_num, ref,
    idr, field_coded, fields (parities it holds), inserted: [dict(parity, copy_of=(frame, parity))], whole (True: a frame inserted for a lost pair).
    kinds: what the case exercises (check_matrix).  n_lost, n_pictures, field_mbs."""

    def per_frame(self):
        """Concealed macroblocks per frame of the repaired stream."""
        return [len(f["inserted"]) * self.field_mbs + (2 * self.field_mbs if f["whole"] else 0) for f in self.frames]

    def n_inserted(self):
        return sum(len(f["inserted"]) for f in self.frames)

    def first_touched(self):
        return min(i for i, f in enumerate(self.frames) if f["inserted"] or f["whole"])


def _walk(units, pics, lost, whole_pics=()):
    """The pictures that are left, in the order of their first unit, with the end-of-sequence units between them: the model of the frames, and what
    has to be put in front of which unit.  whole_pics: pictures (frames) that were inserted for a lost pair of fields."""
    sps = pics[0][0].sps
    max_refs = max(int(sps.max_num_ref_frames), 1)
    events = [(min(s.unit for s in pics[p]), p) for p in range(len(pics)) if p not in lost]
    events += [(ui, None) for ui, u in enumerate(units) if _nal_type(u) in (10, 11)]
    frames, window, put, kinds = [], [], {}, set()
    pend = None  # (first slice seen of a first field, its frame)
    fidx = c2.frame_index(pics)  # of the stream with nothing lost
    was_first = {}

    def insert(at, by):
        F, fi = pend
        par = 0 if F.hdr.bottom_field else 1
        src = next(((j, par) for j in reversed(window) if j != fi and par in frames[j]["fields"]), None)
        if src is None and fi in window:
            src = (fi, 1 - par)  # no other reference frame has a field of this parity: the first field of the same frame (the IDR frame)
        assert src is not None, "entry 0 of the initial P list of the inserted field does not exist"
        frames[fi]["fields"].add(par)
        frames[fi]["inserted"].append(dict(parity=par, copy_of=src))
        put[at] = put.get(at, b"") + field_units(F, units)
        if was_first.get(fi):
            kinds.add("first_field")
        elif frames[fi]["idr"]:
            kinds.add("second_of_idr")
        elif not frames[fi]["ref"]:
            kinds.add("nonref_b" if F.hdr.slice_type % 5 == 1 else "nonref")
        else:
            kinds.add("second_of_p_bottom" if par else "second_of_p_top")
        kinds.add({None: "revealed_by_eos", 0: "revealed_by_frame", 1: "revealed_by_field"}[by])
        if fi > 0 and frames[fi - 1]["inserted"]:
            kinds.add("consecutive_frames")

    for ui, p in sorted(events):
        if p is None:
            if pend:
                insert(ui, None)
                pend = None
            continue
        s = min(pics[p], key=lambda x: x.unit)
        h = s.hdr
        if pend and _is_second(pend[0], s):
            frames[pend[1]]["fields"].add(int(bool(h.bottom_field)))
            pend = None
            continue
        if pend:
            insert(ui, int(bool(h.field_pic)))
            pend = None
        if s.type == 5:
            window = []
        fi = len(frames)
        frames.append(dict(frame_num=int(h.frame_num), ref=bool(s.ref_idc), idr=s.type == 5, field_coded=bool(h.field_pic), inserted=[], whole=p in whole_pics,
                           fields={int(bool(h.bottom_field))} if h.field_pic else {0, 1}))
        if h.field_pic:
            pend = (s, fi)
            was_first[fi] = p > 0 and p - 1 in lost and fidx[p] == fidx[p - 1]  # the first field of its frame is lost: this one was coded as a second field
        if s.ref_idc:
            while len(window) >= max_refs:
                window.pop(0)
            window.append(fi)
    assert pend is None, "a lone field at the very end of input stays unconcealed: end the stream with an end-of-sequence unit"
    return frames, put, kinds


def make_lone(stream, lost_pictures, lost_pairs=()):
    """Removes every slice NAL unit of the field pictures `lost_pictures` (indices in decoding order) and repairs the stream.  lost_pairs: pictures
    (both fields of a frame, consecutive indices) lost as well -- the frame_num gap they leave is repaired by concealutil2.lose_pictures (bit 2)."""
    units, slices, pics = cu.parse(stream)
    lost, pairs = sorted(set(lost_pictures)), sorted(set(lost_pairs))
    assert not set(lost) & set(pairs)
    for p in lost:
        assert 0 < p < len(pics) and pics[p][0].hdr.field_pic and pics[p][0].type == 1, "a non-IDR field picture"
    r = Lone()
    r.n_pictures, r.n_lost = len(pics), len(lost) + len(pairs)
    r.field_mbs = pics[0][0].sps.pic_width_in_mbs * (pics[0][0].sps.pic_height_in_mbs // 2)
    whole = ()
    if pairs:
        # one lost frame, then the lone fields on top of it: in the stream repaired for the pair, the two pictures are one inserted frame picture
        assert len(pairs) == 2 and pairs[1] == pairs[0] + 1 and all(p < pairs[0] - 1 or p > pairs[1] + 1 for p in lost)
        lp = c2.lose_pictures(stream, pairs)
        assert sum(lp.inserted) == 1
        gone = b"".join(u for i, u in enumerate(units) if i not in {s.unit for p in lost + pairs for s in pics[p]})
        units, slices, pics = cu.parse(lp.repaired)
        lost = [p if p < pairs[0] else p - 1 for p in lost]
        whole = (pairs[0],)
    else:
        gone = b"".join(u for i, u in enumerate(units) if i not in {s.unit for p in lost for s in pics[p]})
    r.frames, put, r.kinds = _walk(units, pics, set(lost), whole)
    if pairs:
        r.kinds.add("with_lost_frame")
    dead = {s.unit for p in lost for s in pics[p]}
    r.damaged = gone
    r.repaired = b"".join(put.get(i, b"") + (b"" if i in dead else u) for i, u in enumerate(units))
    return r


def parity_rows(frame, W, Hf, parity):
    """(Y, Cb, Cr) rows of one parity of a coded frame of the oracle (tight I420, W x Hf)."""
    y = frame[:W * Hf].reshape(Hf, W)
    cb = frame[W * Hf:W * Hf * 5 // 4].reshape(Hf // 2, W // 2)
    cr = frame[W * Hf * 5 // 4:].reshape(Hf // 2, W // 2)
    return y[parity::2], cb[parity::2], cr[parity::2]


# ---------------------------------------------------------------- the cases: name -> (generator recipe, lost field pictures, lost pair, end-of-sequence unit appended)
FB = dict(width=176, height=128, frames=6, idr_period=0, profile_idc=77, field_pics=1)
LONE_CASES = {
    # the second field of the IDR frame (picture 1) and the second (bottom) field of a P frame
    "idr_second_cavlc_refs2_idc0": (dict(FB, cabac=0, slices=1, num_ref_frames=2, deblock_idc=0, alpha_off_div2=1, beta_off_div2=-1, seed=801), [1, 7], (), False),
    # bottom field first: the second fields are top fields; explicit weights, one reference frame
    "second_top_cabac_bff_wp1_ref1_idc1": (dict(FB, cabac=1, field_pics=2, slices=2, weighted_pred=1, num_ref_frames=1, deblock_idc=1, seed=802), [3, 9], (), False),
    # lost FIRST fields: the survivor is taken for a first field and gets its complement behind it
    "first_field_cavlc_refs3_idc2": (dict(FB, cabac=0, slices=3, num_ref_frames=3, deblock_idc=2, seed=803), [4, 8], (), False),
    # fields lost in two consecutive frames, picture order count type 1
    "consecutive_cabac_poc1_refs2": (dict(FB, cabac=1, slices=1, poc_type=1, num_ref_frames=2, seed=804), [3, 5, 9], (), False),
    # monochrome, picture order count type 2, the stream ends in an end-of-sequence unit that reveals the last loss
    "mono_cavlc_poc2_eos": (dict(FB, profile_idc=100, mono=1, cabac=0, slices=2, poc_type=2, num_ref_frames=2, seed=805), [5, 11], (), True),
    # B fields (I P B P B ...: pictures 4 / 5, 8 / 9 are non-reference B fields): the second field of a B frame, the second field of a P frame and
    # the FIRST field of the next B frame, whose survivor is revealed by a P field
    "b_cavlc_refs2": (dict(FB, frames=7, cabac=0, slices=1, bframes=1, num_ref_frames=2, seed=806), [5, 7, 8], (), False),
    # (I P B B P B B, bottom field first: pictures 4 .. 7 are B fields) second fields of three consecutive frames
    "b_cabac_bff_implicit_refs3": (dict(FB, frames=7, cabac=1, field_pics=2, slices=2, bframes=2, num_ref_frames=3, weighted_bipred=2, seed=807), [5, 7, 9], (), False),
    # picture-adaptive (picture 2 and pictures 9, 10 are frame pictures): the second field of the IDR frame, revealed by a FRAME picture -- which without
    # the inserted field has no reference frame at all --, and two more
    "mixed_paff_cavlc_refs3": (dict(FB, frames=8, field_pics=3, cabac=0, slices=1, num_ref_frames=3, seed=808), [1, 4, 8], (), False),
    # with bit 2: both fields of one frame and one field of two others
    "with_lost_frame_cavlc_refs2": (dict(FB, frames=7, cabac=0, slices=2, num_ref_frames=2, seed=809), [3, 9], (6, 7), False),
    # slice groups: one P slice per group in the inserted field, its map in the staging buffer
    "fmo_dispersed_cavlc_refs2": (dict(FB, cabac=0, slices=1, slice_groups=3, fmo_type=1, num_ref_frames=2, seed=811), [3, 6], (), False),
    "eos_cabac_wp2_refs2": (dict(FB, cabac=1, slices=3, weighted_pred=2, num_ref_frames=2, seed=810), [7, 11], (), True),
}


def picks_of(name):
    """The lost field pictures of a case (indices in decoding order)."""
    return LONE_CASES[name][1]


def build_case(name, sg, want_recon=False):
    """(recipe, original stream, Lone) of a case."""
    kw, _, pairs, eos = LONE_CASES[name]
    stream = sg.encode(want_recon=want_recon, **kw)[0] + (EOS if eos else b"")
    return kw, stream, make_lone(stream, picks_of(name), pairs)


def check_case(r):
    """What every case has to meet, so that none passes by doing little."""
    assert r.n_lost >= 2 and r.n_inserted() >= 2, "at least two lost fields"
    assert r.n_lost * 10 >= r.n_pictures, "at least 10 %% of the stream's pictures (%d of %d)" % (r.n_lost, r.n_pictures)
    assert all(len(f["inserted"]) <= 1 for f in r.frames)


def check_matrix(results):
    """Over the matrix (name -> Lone): every kind of loss the rule speaks of."""
    kinds = set()
    for r in results.values():
        check_case(r)
        kinds |= r.kinds
    for k in ("second_of_idr", "second_of_p_top", "second_of_p_bottom", "first_field", "consecutive_frames", "nonref_b", "with_lost_frame", "revealed_by_eos",
              "revealed_by_frame", "revealed_by_field"):
        assert k in kinds, "no case with: " + k


def check_recipes():
    kws = [c[0] for c in LONE_CASES.values()]
    assert len(kws) >= 8
    assert {kw["cabac"] for kw in kws} == {0, 1} and {kw["field_pics"] for kw in kws} == {1, 2, 3}
    assert {kw["slices"] for kw in kws} == {1, 2, 3} and {kw.get("num_ref_frames", 1) for kw in kws} == {1, 2, 3}
    assert any(kw.get("weighted_pred") == 1 for kw in kws)
    assert {kw.get("poc_type", 0) for kw in kws} == {0, 1, 2} and {kw.get("deblock_idc", 0) for kw in kws} == {0, 1, 2}
    assert any(kw.get("bframes") for kw in kws) and any(kw.get("mono") for kw in kws)
    assert any(c[3] for c in LONE_CASES.values()) and any(c[2] for c in LONE_CASES.values())
    assert all(kw["width"] == 176 and kw["height"] == 128 and 5 <= kw["frames"] <= 8 for kw in kws)
