// h264decode_amd/csrc/mi_picture.cpp -- what one slice NAL does to one stream's picture under construction: where pictures and slices go in the
// batch's tables (Stage, mi_decoder.hpp), asking mi_dpb.cpp -- picture management, 8.2 -- for slots, counts and lists; the pictures inserted for
// lost frames and lone fields.  Launches nothing (a first B slice has mi_batch.cpp set up what B pictures need: ensure_b_buffers).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mi_decoder.hpp"

void finish_picture(h264mi_decoder *d, int si) {
    StreamState &s = d->st[si];
    Stage &g = d->stage[d->prep];
    Dpb &dpb = s.dpb;
    if (dpb.cur_slot < 0) return;
    dpb.finish_picture(s.sps[s.active_sps]);
    PicDesc &pd = g.h_pics[s.cur_pic];
    pd.n_slices = static_cast<uint32_t>(s.cur_slices);
    if (dpb.cur_field) {
        // a field: the frame goes out when its second field is complete -- or, if that never comes, when the next picture starts (flush_pending_field)
        if (dpb.pend_slot < 0) {
            const Slot &f = dpb.slots[dpb.cur_slot];
            s.pend_out.poc = f.poc;
            s.pend_out.top_foc = f.fpoc[0], s.pend_out.bottom_foc = f.fpoc[1];
            // (pic_order_cnt_type 2 gives both fields of a reference frame one count, and output order is decoding order, 8.2.1.3: this picture is the second field)
            s.pend_out.first_parity = f.fpoc[0] != f.fpoc[1] ? f.fpoc[1] < f.fpoc[0] : 2 - dpb.cur_field;
            if (dpb.cur_second) s.pend_out.pic2 = s.cur_pic;
            g.out[si].push_back(s.pend_out);
        }
    } else if (!g.out[si].empty()) {
        OutFrame &o = g.out[si].back();
        const Slot &f = dpb.slots[dpb.cur_slot];
        o.poc = f.poc, o.top_foc = f.fpoc[0], o.bottom_foc = f.fpoc[1]; // operation 5 rewrites them (first_parity is from before: start_picture)
    }
    // Every macroblock of the picture belongs to exactly one slice wavefront (SliceDesc::fill_from / end_mb): order the
    // slices by first_mb (arbitrary slice order is legal in Baseline); a slice's range ends where the next one starts.
    std::vector<uint32_t> idx(pd.n_slices);
    for (uint32_t i = 0; i < pd.n_slices; i++) idx[i] = pd.first_slice + i;
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return g.h_slices[a].first_mb < g.h_slices[b].first_mb; });
    const uint32_t total = pd.wmb * pd.hmb;
    if (pd.fmo) {
        // slice groups: a slice ends where the next slice of ITS group starts; nothing is filled by the wavefronts (the records of
        // the whole picture are zeroed before the launch: launch_entropy)
        const uint8_t *map = g.h_bits + pd.sgmap_off;
        for (uint32_t i = 0; i < pd.n_slices; i++) {
            SliceDesc &sd = g.h_slices[idx[i]];
            sd.fill_from = sd.first_mb, sd.end_mb = total;
            for (uint32_t j = i + 1; j < pd.n_slices; j++)
                if (map[g.h_slices[idx[j]].first_mb] == map[sd.first_mb]) {
                    sd.end_mb = std::max(g.h_slices[idx[j]].first_mb, sd.first_mb);
                    break;
                }
        }
        g.fmo_pics.push_back(static_cast<uint32_t>(s.cur_pic));
    } else
        for (uint32_t i = 0; i < pd.n_slices; i++) {
            SliceDesc &sd = g.h_slices[idx[i]];
            sd.fill_from = i == 0 ? 0 : sd.first_mb;
            sd.end_mb = i + 1 < pd.n_slices ? std::max(g.h_slices[idx[i + 1]].first_mb, sd.first_mb) : total;
        }
    dpb.cur_slot = s.cur_pic = -1;
}

static int scaling_set_for(h264mi_decoder *d, const h264mi_pps &p) {
    ScalingSet tmp;
    build_scaling(p.scaling_list_4x4, p.scaling_list_8x8, &tmp);
    uint32_t &mine = d->scaling_used[d->prep];
    for (int i = 0; i < d->n_scaling; i++)
        if (!memcmp(&d->h_tables->scaling[i], &tmp, sizeof(tmp))) {
            mine |= 1u << i;
            return i;
        }
    // a new matrix: the next free entry, or one that only batches which have finished referred to (the batch of the other staging set
    // may still be executing: its entries stay as they are -- the upload rewrites them with the bytes they hold)
    int at = d->n_scaling < MI_MAX_SCALING_SETS ? d->n_scaling : -1;
    if (at < 0) {
        uint32_t busy = 0;
        for (int st = 0; st < MI_STAGES; st++) busy |= d->scaling_used[st];
        for (int i = 0; i < MI_MAX_SCALING_SETS && at < 0; i++)
            if (!(busy >> i & 1)) at = i;
        if (at < 0) return -1;
    } else
        d->n_scaling++;
    d->h_tables->scaling[at] = tmp;
    d->tables_dirty = true;
    mine |= 1u << at;
    return at;
}

// 8.2.5.2 decoding process for gaps in frame_num (h264/sps.go:311-312 parses the flag, nothing in the reference uses it): a
// non-IDR picture whose frame_num is neither PrevRefFrameNum nor its successor says that reference frames are missing.  With
// gaps_in_frame_num_value_allowed_flag every skipped value becomes a "non-existing" short-term frame that goes through the
// sliding window like a decoded one -- it pushes older frames out and takes its place in the initial lists, so that the
// indices of the surviving pictures come out as the encoder meant them.  Without the flag pictures were lost: the stream is
// refused (H264MI_EBITSTREAM; with isolation it alone leaves the batch and waits for its next IDR picture) rather than
// predicted from the wrong pictures.
static int fill_frame_num_gap(h264mi_decoder *d, int si, const h264mi_sps &sps, const h264mi_slice_header &sh) {
    Dpb &dpb = d->st[si].dpb;
    const int m = dpb.missing_frames(sps, sh), max_fn = 1 << (sps.log2_max_frame_num_minus4 + 4);
    if (!m) return H264MI_OK;
    if (!sps.gaps_in_frame_num_value_allowed) {
        set_error("stream %d: frame_num %d after %d: reference pictures are missing", si, sh.frame_num, dpb.prev_ref_frame_num);
        return H264MI_EBITSTREAM;
    }
    for (int k = 0; k < m; k++)
        if (!dpb.add_nonexisting_frame(sps, (dpb.prev_ref_frame_num + 1) % max_fn)) {
            set_error("stream %d: frame pool exhausted", si);
            return H264MI_ECAPACITY;
        }
    return H264MI_OK;
}

// The pictures of this batch that live in the frame slot a list entry names (a frame, or either field: whichever of them this batch decodes) have to
// be reconstructed (deblocked) before picture `pic`, which predicts from it: Stage::Pic::wave
static void wave_after(Stage &g, const Dpb &dpb, int pic, int entry) {
    if (entry < 0) return;
    const Slot &rs = dpb.slots[MI_REF_SLOT(entry)]; // (frame pictures never set the parity bit)
    for (int p : {rs.pic, rs.fpic[0], rs.fpic[1]})
        if (p >= 0 && p != pic && p < static_cast<int>(g.pics.size())) g.pics[pic].wave = std::max(g.pics[pic].wave, g.pics[p].wave + 1);
}

// PicOrderCnt of a reference list entry: a field's own count in a field picture (entries name fields: slot | MI_REF_PARITY), the frame's otherwise
static int list_entry_poc(const Dpb &dpb, int e, bool fieldpic) {
    return fieldpic ? dpb.slots[MI_REF_SLOT(e)].fpoc[(e & MI_REF_PARITY) ? 1 : 0] : dpb.slots[e].poc;
}

// The first slice header of a picture WITHOUT SLICES (conceal_lone_field, conceal_frame_num_gap): what the repaired stream's slices of it say, as far as
// picture management looks
static h264mi_slice_header inserted_header(const h264mi_sps &sps, const h264mi_pps &pps, int pps_id, int frame_num, int ref_idc, int cycle, int poc_lsb) {
    h264mi_slice_header f;
    memset(&f, 0, sizeof(f));
    f.pps_id = pps_id, f.frame_num = frame_num, f.nal_ref_idc = ref_idc, f.nal_unit_type = 1, f.slice_group_change_cycle = cycle;
    if (sps.pic_order_count_type == 0) f.pic_order_cnt_lsb = poc_lsb % (1 << (sps.log2_max_pic_order_cnt_lsb_min4 + 4));
    f.num_ref_idx_active_override = 1;
    f.slice_qp_y = 26 + pps.pic_init_qp_minus26;
    return f;
}

// The first slice of a new picture (`sh`, of NAL unit type `type`; second: the second field of the frame in Dpb::pend_slot): its frame slot, its place
// in the batch's tables, its PicDesc and the frame it goes out as.  The picture is then under construction (Dpb::cur_slot, StreamState::cur_*) until finish_picture.
static int start_picture(h264mi_decoder *d, int si, const h264mi_sps &sps, const h264mi_pps &pps, uint32_t pps_id, const h264mi_slice_header &sh, int type, bool second) {
    StreamState &s = d->st[si];
    Stage &g = d->stage[d->prep];
    const int wmb = sps.pic_width_in_mbs, hmb = sps.pic_height_in_mbs, hmb_pic = sh.field_pic ? hmb / 2 : hmb;
    // (a field counts as a picture of its own against max_frames_per_batch: include/h264mi.h)
    if (s.n_pics_in_batch >= d->cfg.max_frames_per_batch || g.n_pics >= d->pics_cap) {
        set_error("stream %d: more than %d pictures in one batch", si, d->cfg.max_frames_per_batch);
        return H264MI_ECAPACITY;
    }
    int r, slot = second ? s.dpb.pend_slot : s.dpb.first_free_slot();
    if (slot < 0) {
        set_error("stream %d: frame pool exhausted", si);
        return H264MI_ECAPACITY;
    }
    if (g.mb_used + static_cast<uint64_t>(wmb) * hmb_pic > d->mb_cap) {
        set_error("macroblock record pool exhausted");
        return H264MI_ECAPACITY;
    }
    // Error concealment of an IDR frame picture (H264MI_CONCEAL_IDR; the rule: include/h264mi.h): its concealment reference is entry 0 of the initial P
    // list of a frame picture with frame_num (PrevRefFrameNum + 1) mod MaxFrameNum -- what the picture predicts from in the repaired stream, where it is
    // a non-IDR picture that ends in memory management operation 5 --, looked up now: before the picture takes its slot and long before its marking
    // drops the references (Dpb::finish_picture).  The slot named stays put for the batch: it is held, or a picture of this batch.  The references
    // must have been decoded under an SPS this picture could still predict under (MaxFrameNum: the previous sequence's, which is then this one's).
    StreamState::RefSeq seq;
    seq.wmb = wmb, seq.hmb = hmb, seq.chroma_format = sps.chroma_format, seq.frame_mbs_only = sps.frame_mbs_only, seq.log2_max_frame_num_minus4 = sps.log2_max_frame_num_minus4;
    int idr_ref = -1;
    if (d->conceal_idr && type == 5 && !sh.field_pic && !second && seq == s.ref_seq) {
        const int best = s.dpb.initial_p_entry0(sps, (s.dpb.prev_ref_frame_num + 1) % (1 << (sps.log2_max_frame_num_minus4 + 4)), 0);
        if (best >= 0 && !s.dpb.slots[best].nonexisting) idr_ref = best;
    }
    s.ref_seq = seq;
    s.cur_pic = g.n_pics++;
    s.cur_slices = 0;
    s.cur_first_mbs.clear();
    s.dpb.begin_picture(sps, sh, slot, second, s.cur_pic);
    const Slot &sl = s.dpb.slots[slot];
    PicDesc &pd = g.h_pics[s.cur_pic];
    memset(&pd, 0, sizeof(pd));
    pd.stream = si, pd.slot = slot, pd.wmb = wmb, pd.hmb = hmb_pic;
    // where the picture lives in its frame slot: a field picture in the rows of its parity (PicDesc)
    pd.field = static_cast<uint8_t>(s.dpb.cur_field);
    pd.pitch = static_cast<uint32_t>(wmb * 16 * (sh.field_pic ? 2 : 1)), pd.plane = static_cast<uint32_t>(wmb * 16) * static_cast<uint32_t>(hmb * 16);
    pd.inv_wmb = wmb > 1 ? static_cast<uint32_t>((1ull << 32) / static_cast<uint32_t>(wmb)) + 1u : 0u; // (one macroblock column: mi_types.h)
    pd.pool_base = d->h_pools[si].base, pd.slot_bytes = d->slot_bytes, pd.n_slots = static_cast<uint32_t>(d->n_slots);
    g.pics.resize(s.cur_pic), g.pics.emplace_back();
    g.pics[s.cur_pic].init_qp = static_cast<uint8_t>(std::min(std::max(26 + pps.pic_init_qp_minus26, 0), 51));
    pd.conceal_ref = -1;
    if (d->conceal && type != 5 && (!sh.field_pic || d->conceal_fields)) {
        // Error concealment: the picture is concealable when the initial P list, built for THIS picture whatever the types of its slices, is not
        // empty; its entry 0 is what lost macroblocks are copied from.  A field picture's (H264MI_CONCEAL_FIELDS) is a field -- the first field of the
        // same frame, if this is its second field and that one is a short-term reference --, written like every entry of a field list as
        // slot | parity (MI_REF_PARITY).  (A frame inferred by the frame_num gap process holds no samples: not concealable.)
        const int best = s.dpb.initial_p_entry0(sps, sh.frame_num, s.dpb.cur_field);
        if (best >= 0 && !s.dpb.slots[MI_REF_SLOT(best)].nonexisting) {
            pd.conceal_ref = static_cast<int16_t>(best);
            // ... and the picture is reconstructed behind it when this batch decodes it: a non-IDR I picture would otherwise be in wave 0, and the
            // MODIFIED lists of a P picture's slices need not hold this entry
            wave_after(g, s.dpb, s.cur_pic, best);
        }
    }
    if (idr_ref >= 0) { // ... and like a non-IDR I picture that is concealable, the IDR picture is reconstructed behind its concealment reference, damaged or not
        pd.conceal_ref = static_cast<int16_t>(idr_ref);
        wave_after(g, s.dpb, s.cur_pic, idr_ref);
    }
    // K11: the picture order counts of the picture and of its concealment reference as they are NOW (Stage::Pic::conceal_poc)
    g.pics[s.cur_pic].conceal_poc = {sh.field_pic ? sl.fpoc[sh.bottom_field ? 1 : 0] : sl.poc, pd.conceal_ref >= 0 ? list_entry_poc(s.dpb, pd.conceal_ref, sh.field_pic != 0) : 0};
    if (s.pending_drops) { // slices without a readable header in front of this picture's first good one: lost slices of it, if it can be concealed
        const int n = s.pending_drops, e = s.pending_drop_err;
        s.pending_drops = 0;
        if (pd.conceal_ref < 0 || s.pending_drop_type != (type == 5 ? 5 : 1)) { // (a dropped unit of the other kind was no slice of this picture)
            set_error("stream %d: a slice header does not parse, in a picture that cannot be concealed", si);
            return e;
        }
        g.pics[s.cur_pic].dropped = static_cast<uint16_t>(std::min(n, 65535));
    }
    pd.mb_base = g.mb_used;
    g.mb_used += static_cast<uint64_t>(wmb) * hmb_pic;
    pd.first_slice = g.n_slices;
    pd.cabac = pps.entropy_coding_mode, pd.t8x8_mode = pps.transform_8x8_mode, pd.cip = pps.constrained_intra_pred;
    pd.mono = sps.chroma_format == 0;
    pd.weighted_pred = pps.weighted_pred;
    pd.cqp_off[0] = static_cast<int8_t>(pps.chroma_qp_index_offset), pd.cqp_off[1] = static_cast<int8_t>(pps.second_chroma_qp_index_offset);
    pd.is_intra_only = 1;
    int ss = scaling_set_for(d, pps);
    if (ss < 0) {
        set_error("more than %d distinct scaling matrices in flight", MI_MAX_SCALING_SETS);
        return H264MI_ECAPACITY;
    }
    pd.scaling_set = static_cast<uint8_t>(ss);
    pd.order = s.n_pics_in_batch++;
    if (pps.num_slice_groups_minus1 > 0) { // FMO: this picture's macroblock-to-slice-group map travels with the bitstream (8.2.2; h264/slice.go:134-158)
        const size_t n_mbs = static_cast<size_t>(wmb) * hmb_pic, moff = (g.map_cursor + 15) & ~static_cast<size_t>(15);
        if (moff + n_mbs + 4096 > d->bits_cap) {
            set_error("bitstream staging buffer too small for the slice group maps (%zu bytes)", d->bits_cap);
            return H264MI_ECAPACITY;
        }
        r = mb_to_slice_group_map(&sps, &pps, s.sg_ids[pps_id].data(), s.sg_ids[pps_id].size(), sh.slice_group_change_cycle, sh.field_pic ? 1 : 0, g.h_bits + moff, n_mbs, nullptr);
        if (r != H264MI_OK) return r;
        pd.fmo = 1, pd.sgmap_off = static_cast<uint32_t>(moff);
        g.map_cursor = moff + n_mbs;
        g.bits_end = std::max(g.bits_end, g.map_cursor);
    }
    if (!second) { // the frame this picture belongs to, as it will be shown: pushed now (frame picture), or when its fields are through (finish_picture / flush_pending_field)
        OutFrame of{slot, wmb, hmb, crop_unit_x(&sps) * sps.frame_crop_left_offset, crop_unit_y(&sps) * sps.frame_crop_top_offset, sps.width, sps.height, sl.poc, sh.frame_num,
                    sh.nal_ref_idc, sh.nal_unit_type == 5, s.cur_pic, sh.nal_unit_type == 5};
        if (sh.nal_ref_idc && sh.adaptive_ref_pic_marking_mode_flag)
            for (int k = 0; k < sh.n_memory_management_control_operations; k++)
                if (sh.memory_management_control_operation[k] == 5) of.new_sequence = 1;
        // (a frame picture: both counts are known now; a frame of two fields gets them when it goes out: finish_picture / flush_pending_field)
        of.mono = sps.chroma_format == 0;
        of.field_coded = sh.field_pic != 0, of.top_foc = sl.fpoc[0], of.bottom_foc = sl.fpoc[1], of.first_parity = !sh.field_pic && sl.fpoc[1] < sl.fpoc[0];
        if (sps.vui_parameters_present && sps.video_signal_type_present) {
            of.video_full_range = sps.video_full_range;
            if (sps.color_description_present) of.matrix_coefficients = sps.matrix_coefficients;
        }
        if (sh.field_pic)
            s.pend_out = of, s.pend_sps_id = pps.sps_id, s.pend_pps_id = static_cast<int>(pps_id), s.pend_stale = false;
        else
            g.out[si].push_back(of);
    }
    g.wmb_max = std::max(g.wmb_max, wmb);
    g.hmb_max = std::max(g.hmb_max, hmb_pic);
    g.mbs_max = std::max(g.mbs_max, wmb * hmb_pic);
    g.info.n_macroblocks += static_cast<int64_t>(wmb) * hmb_pic;
    if (si == 0) g.info.width = sps.width, g.info.height = sps.height, g.info.coded_width = wmb * 16, g.info.coded_height = hmb * 16;
    return H264MI_OK;
}

// Error concealment of a lone field (H264MI_CONCEAL_LONE_FIELDS; the rule: include/h264mi.h).  The frame in Dpb::pend_slot holds one field F and the
// other one is not coming: the field F' of the opposite parity is put in front of whatever revealed that (`next`: the picture, with the parameter
// sets it is decoded under; nullptr: an end-of-sequence / end-of-stream unit) as a picture WITHOUT SLICES -- the second field of F's frame, a picture
// of the batch like any other (PicDesc, records, PicOrderCnt, marking), all of whose macroblocks k_conceal writes as P_Skip copies of
// PicDesc::conceal_ref: entry 0 of the initial P list for fields built for F' (the field of F''s parity of the nearest reference frame that has one;
// F itself when there is none).  The header made up here is what the repaired stream's slices of F' say, as far as picture management looks.  Returns H264MI_OK (inserted: the frame went out
// complete), 1 (not concealable: the caller paints the rows grey as without the bit) or an error.
static int conceal_lone_field(h264mi_decoder *d, int si, const h264mi_sps *nsps, const h264mi_pps *npps, const h264mi_slice_header *next) {
    StreamState &s = d->st[si];
    Stage &g = d->stage[d->prep];
    // the parameter sets F was decoded under must still be the ones the stream stores
    if (s.pend_stale || s.pend_sps_id < 0 || s.pend_pps_id < 0 || !s.sps_ok[s.pend_sps_id] || !s.pps_ok[s.pend_pps_id] || s.pps[s.pend_pps_id].sps_id != s.pend_sps_id) return 1;
    const h264mi_sps &sps = s.sps[s.pend_sps_id];
    const h264mi_pps &pps = s.pps[s.pend_pps_id];
    const h264mi_slice_header &fh = s.dpb.first_sh; // F's first slice: F is the picture that was completed last
    const Slot &fs = s.dpb.slots[s.dpb.pend_slot];
    if (!fh.field_pic || fs.fields != (fh.bottom_field ? 2 : 1) || fs.frame_num != fh.frame_num) return 1;
    if (pps.entropy_coding_mode && !d->cfg.allow_unpinned_field_cabac) return 1;
    const int parity = fh.bottom_field ? 1 : 2; // of F' (Dpb::cur_field: 1 top, 2 bottom)
    const int ref0 = s.dpb.second_field_p_entry0(sps, fs.frame_num, parity);
    if (ref0 < 0 || s.dpb.slots[MI_REF_SLOT(ref0)].nonexisting) return 1;
    // F' -- and the revealing picture, which has to fit with the bit set wherever it fits with the bit clear -- in what the batch has left
    // (with H264MI_CONCEAL_PICTURES the revealing picture may open a frame_num gap as well: the frames conceal_frame_num_gap would insert with this bit
    // clear must still fit with it set, or the inserted field would turn a concealed gap into a refused stream)
    int gap = 0;
    if (next && d->conceal_pics && next->nal_unit_type != 5 && !nsps->gaps_in_frame_num_value_allowed) {
        const int max_fn = 1 << (nsps->log2_max_frame_num_minus4 + 4);
        const int prev_ref = fh.nal_ref_idc ? fs.frame_num : s.dpb.prev_ref_frame_num; // PrevRefFrameNum once F' is through
        if (next->frame_num != prev_ref) gap = (next->frame_num - (prev_ref + 1) % max_fn + max_fn) % max_fn;
        if (gap > H264MI_CONCEAL_MAX_GAP) gap = 0; // (not concealed either way)
    }
    const int need = (next ? 2 : 1) + gap;
    const uint64_t field_mbs = static_cast<uint64_t>(sps.pic_width_in_mbs) * (sps.pic_height_in_mbs / 2);
    const uint64_t next_mbs = next ? static_cast<uint64_t>(nsps->pic_width_in_mbs) * (next->field_pic ? nsps->pic_height_in_mbs / 2 : nsps->pic_height_in_mbs) : 0;
    if (s.n_pics_in_batch + need > d->cfg.max_frames_per_batch || g.n_pics + need > d->pics_cap) return 1;
    const uint64_t gap_mbs = gap ? static_cast<uint64_t>(gap) * nsps->pic_width_in_mbs * nsps->pic_height_in_mbs : 0;
    if (g.mb_used + field_mbs + next_mbs + gap_mbs > d->mb_cap) return 1;
    size_t cursor = g.map_cursor; // every picture's slice group map goes into the staging buffer (start_picture)
    for (int k = 0; k < need; k++) // F', the revealing picture, the frames of its gap
        if ((k ? npps : &pps)->num_slice_groups_minus1 > 0) {
            const size_t moff = (cursor + 15) & ~static_cast<size_t>(15), n_mbs = static_cast<size_t>(k == 0 ? field_mbs : (k == 1 ? next_mbs : gap_mbs / gap));
            if (moff + n_mbs + 4096 > d->bits_cap) return 1;
            cursor = moff + n_mbs;
        }
    if (scaling_set_for(d, pps) < 0) return 1;
    h264mi_slice_header f = inserted_header(sps, pps, s.pend_pps_id, fs.frame_num, fh.nal_ref_idc, fh.slice_group_change_cycle, fh.pic_order_cnt_lsb + 1);
    f.field_pic = 1, f.bottom_field = fh.bottom_field ? 0 : 1;
    const int drops = s.pending_drops; // slices with an unreadable header in front of the revealing picture belong to IT, not to the inserted field
    s.pending_drops = 0;
    int r = start_picture(d, si, sps, pps, static_cast<uint32_t>(s.pend_pps_id), f, 1, true);
    if (r == H264MI_OK && g.h_pics[s.cur_pic].conceal_ref != ref0) { // (cannot happen: the same list was built above)
        set_error("stream %d: the field inserted for a lone field has no reference", si);
        r = H264MI_EBITSTREAM;
    }
    if (r == H264MI_OK) finish_picture(d, si); // (both fields are through: the frame goes out there)
    s.pending_drops = drops;
    return r;
}

// A first field whose second field did not come: the frame goes out with one field decoded, the rows of the other parity painted mid-grey
// (at the start of the batch's reconstruction: whatever the slot held before must not show) -- or, with H264MI_CONCEAL_LONE_FIELDS and where
// that is possible, complete: conceal_lone_field.  `next`: the picture that follows, nullptr: none (an end-of-sequence / end-of-stream unit).
int flush_pending_field(h264mi_decoder *d, int si, const h264mi_sps *nsps, const h264mi_pps *npps, const h264mi_slice_header *next) {
    StreamState &s = d->st[si];
    if (s.dpb.pend_slot < 0) return H264MI_OK;
    if (d->conceal_lone) {
        const int r = conceal_lone_field(d, si, nsps, npps, next);
        if (r != 1) return r;
    }
    Stage &g = d->stage[d->prep];
    const Slot &f = s.dpb.slots[s.dpb.pend_slot];
    OutFrame o = s.pend_out;
    o.poc = f.poc;
    o.first_parity = f.fields == 1 ? 0 : 1; // the field there is; the missing one is reported with the same count
    o.top_foc = o.bottom_foc = f.fpoc[o.first_parity];
    g.out[si].push_back(o);
    g.grey.push_back({static_cast<uint32_t>(si), static_cast<uint32_t>(s.dpb.pend_slot), f.fields == 1 ? 1u : 0u, static_cast<uint32_t>(o.wmb * 16), static_cast<uint32_t>(o.hmb * 16)});
    s.dpb.pend_slot = -1;
    return H264MI_OK;
}

// Error concealment of wholly lost reference frames (H264MI_CONCEAL_PICTURES; the rule: include/h264mi.h).  `sh` is the first slice of a picture that is
// not the second field of the frame before it.  Where fill_frame_num_gap would refuse the stream -- frame_num skips values and the SPS does not allow
// gaps -- and the gap is concealable, one frame picture WITHOUT SLICES per missing frame_num is put in front of the revealing picture: a picture of the
// batch like any other (slot, PicDesc, records, output frame, POC, sliding window), all of whose macroblocks k_conceal writes as P_Skip copies of
// PicDesc::conceal_ref -- which of the second inserted picture on is the inserted picture before it.  Returns H264MI_OK (inserted), 1 (no gap, or not
// concealable: the caller goes on as without the bit) or an error.
static int conceal_frame_num_gap(h264mi_decoder *d, int si, const h264mi_sps &sps, const h264mi_pps &pps, uint32_t pps_id, const h264mi_slice_header &sh) {
    StreamState &s = d->st[si];
    Stage &g = d->stage[d->prep];
    const int m = s.dpb.missing_frames(sps, sh);
    if (!m || sps.gaps_in_frame_num_value_allowed || m > H264MI_CONCEAL_MAX_GAP) return 1;
    const int max_fn = 1 << (sps.log2_max_frame_num_minus4 + 4), first = (s.dpb.prev_ref_frame_num + 1) % max_fn;
    const int ref0 = s.dpb.initial_p_entry0(sps, first, 0);
    if (ref0 < 0 || s.dpb.slots[ref0].nonexisting) return 1;
    // the m pictures and the revealing one must fit into what the batch has left (a slot taken by a picture of this batch stays taken until the next
    // prepare, so counting the free ones now is exact)
    const uint64_t frame_mbs = static_cast<uint64_t>(sps.pic_width_in_mbs) * sps.pic_height_in_mbs;
    if (s.n_pics_in_batch + m + 1 > d->cfg.max_frames_per_batch || g.n_pics + m + 1 > d->pics_cap || s.dpb.free_slots() < m + 1) return 1;
    if (g.mb_used + frame_mbs * m + (sh.field_pic ? frame_mbs / 2 : frame_mbs) > d->mb_cap) return 1;
    if (pps.num_slice_groups_minus1 > 0) { // every picture's slice group map goes into the staging buffer (start_picture)
        size_t cursor = g.map_cursor;
        for (int k = 0; k <= m; k++) {
            const size_t moff = (cursor + 15) & ~static_cast<size_t>(15);
            if (moff + frame_mbs + 4096 > d->bits_cap) return 1;
            cursor = moff + frame_mbs;
        }
    }
    if (scaling_set_for(d, pps) < 0) return 1;
    const int drops = s.pending_drops; // slices with an unreadable header in front of `sh` belong to ITS picture, not to an inserted one
    s.pending_drops = 0;
    for (int k = 0; k < m; k++) {
        const h264mi_slice_header f = inserted_header(sps, pps, static_cast<int>(pps_id), (first + k) % max_fn, 1, sh.slice_group_change_cycle, s.dpb.prev_poc_lsb + 2);
        int r = start_picture(d, si, sps, pps, pps_id, f, 1, false);
        if (r != H264MI_OK) return r;
        if (g.h_pics[s.cur_pic].conceal_ref < 0) { // (cannot happen: entry 0 was looked up above, and from then on it is the picture inserted before)
            set_error("stream %d: frame_num %d after %d: reference pictures are missing", si, sh.frame_num, s.dpb.prev_ref_frame_num);
            return H264MI_EBITSTREAM;
        }
        finish_picture(d, si);
    }
    s.pending_drops = drops;
    return H264MI_OK;
}

// one slice NAL of stream `si`
// `off` / `rlen`: where batch_prepare's parallel pass put the slice's RBSP in the pinned staging buffer (16-byte aligned)
int add_slice(h264mi_decoder *d, int si, size_t off, size_t rlen, int ref_idc, int type) {
    StreamState &s = d->st[si];
    Stage &g = d->stage[d->prep];
    if (g.n_slices >= d->slices_cap) {
        set_error("more than %d slices in the batch", d->slices_cap);
        return H264MI_ECAPACITY;
    }
    uint8_t *rbsp = g.h_bits + off;
    // random access: the stream waits for an entry point -- no slice in front of it is an error, whatever it lacks (skip_waiting)
    const bool waiting = d->random_access && (s.need_idr || !s.decoded_any);
    auto skip_waiting = [&s] {
        s.ra.skipped_waiting_nals++;
        s.sei = {0, 0, 0, 0, 0}; // (the message belonged to this picture)
        return H264MI_OK;
    };
    // peek pps id: first_mb_in_slice, slice_type, pic_parameter_set_id
    BitReader br(rbsp, rlen);
    br.ue();
    br.ue();
    uint32_t pps_id = br.ue();
    if (waiting && (pps_id > 255 || !s.pps_ok[pps_id] || !s.sps_ok[s.pps[pps_id].sps_id])) return skip_waiting();
    if (pps_id > 255 || !s.pps_ok[pps_id]) {
        set_error("stream %d: slice refers to missing PPS %u", si, pps_id);
        return H264MI_EBITSTREAM;
    }
    const h264mi_pps &pps = s.pps[pps_id];
    if (!s.sps_ok[pps.sps_id]) {
        set_error("stream %d: PPS %u refers to missing SPS %d", si, pps_id, pps.sps_id);
        return H264MI_EBITSTREAM;
    }
    const h264mi_sps &sps = s.sps[pps.sps_id];
    h264mi_slice_header sh;
    int r = parse_slice_header(&sps, &pps, ref_idc, type, rbsp, rlen, &sh);
    if (r != H264MI_OK && waiting) return skip_waiting();
    if (r != H264MI_OK) {
        // error concealment: a damaged slice header is a lost slice -- its macroblocks stay undelivered and k_conceal fills them in -- but only in a
        // picture that is concealable; anywhere else it fails the stream as without the mode.  Which picture a slice without a header belongs to is not
        // known: it is taken for a slice of the picture under construction if that one is of its kind -- a unit of type 1: a non-IDR picture, a unit of
        // type 5 (tolerated with H264MI_CONCEAL_IDR only): an IDR picture --, else, or if there is none, of the picture the next slice starts (decided there).
        if (d->conceal && (type == 1 || (type == 5 && d->conceal_idr)) && !s.need_idr && (r == H264MI_EBITSTREAM || r == H264MI_EINVAL)) {
            if (s.dpb.cur_slot < 0 || (s.dpb.first_sh.nal_unit_type == 5) != (type == 5)) {
                s.pending_drop_type = s.pending_drops && s.pending_drop_type != type ? -1 : type;
                s.pending_drops++, s.pending_drop_err = r;
                return H264MI_OK;
            }
            if (g.h_pics[s.cur_pic].conceal_ref >= 0) {
                g.pics[s.cur_pic].dropped++;
                return H264MI_OK;
            }
        }
        return r;
    }
    if (sh.redundant_pic_cnt > 0) return H264MI_OK; // redundant pictures are dropped
    bool entry = false; // random access: the stream enters at the picture this slice starts
    if (waiting) {
        // an entry point: an IDR picture, or a primary coded picture whose access unit carried a recovery point with recovery_frame_cnt 0
        if (type != 5 && !(s.sei.found && s.sei.recovery_frame_cnt == 0)) return skip_waiting();
        entry = true;
        s.need_idr = false;
        if (type != 5) { // empty picture management, and what precedes the picture in output order is not coming: leading pictures
            if (!s.dpb.start_at_entry(sps, sh.frame_num)) {
                set_error("stream %d: frame pool exhausted", si);
                return H264MI_ECAPACITY;
            }
            s.lead = true, s.skipping = false;
            s.ra.entries++;
        }
    } else if (s.need_idr) { // after an error nothing can be trusted before the next IDR picture
        if (type != 5) {
            s.sei = {0, 0, 0, 0, 0};
            return H264MI_OK;
        }
        s.need_idr = false;
    }
    const int st = sh.slice_type % 5;
    if (st > 2) {
        set_error("stream %d: slice_type %d is out of scope (SP / SI slices)", si, sh.slice_type);
        return H264MI_EUNSUPPORTED;
    }
    // chroma_format_idc 0 (monochrome; h264/sps.go:226-243 ChromaFormat, h264/slice.go:179-219 SubWidthC / SubHeightC): the entropy kernels leave out the
    // chroma syntax (PicDesc::mono), and nothing else changes -- the frame pool starts out at 128, intra chroma prediction is the DC of planes that are
    // 128 everywhere, inter prediction copies 128, the residual is zero and the filters leave constants alone: the chroma planes a 4:2:0 display expects
    if (sps.chroma_format > 1 || sps.bit_depth_luma_minus8 || sps.bit_depth_chroma_minus8 || sps.qprime_y_zero_transform_bypass) {
        set_error("stream %d: only 4:2:0 and monochrome 8-bit streams are supported (chroma_format_idc %d; 4:2:2 / 4:4:4 and more than 8 bits are out of scope)", si, sps.chroma_format);
        return H264MI_EUNSUPPORTED;
    }
    // frame_mbs_only_flag = 0 (h264/sps.go:316-322): the pictures are frames (decoded like progressive ones: map units are two macroblock rows
    // high, crop units double) or field pictures (h264/slice.go:867-872: field_pic_flag / bottom_field_flag; PAFF), in any mix.
    // Macroblock-adaptive frame/field coding (MBAFF, h264/slice.go:563-568, 624-634) is not implemented.
    if (!sps.frame_mbs_only && sps.mb_adaptive_frame_field) {
        set_error("stream %d: macroblock-adaptive frame/field coding (MBAFF) is out of scope", si);
        return H264MI_EUNSUPPORTED;
    }
    if (sh.field_pic) {
        if (pps.entropy_coding_mode && !d->cfg.allow_unpinned_field_cabac) {
            // ctxIdx 277..398 and 436..459 (significant_coeff_flag / last_significant_coeff_flag of field-coded blocks, Tables 9-19 .. 9-24): the values in
            // this library's tables were written down without the standard at hand and nothing on its build machine pins them (mi_cabac_mn.cpp) -- a
            // decoder with wrong tables produces plausible, wrong pictures, so it takes an explicit request (h264mi_config.allow_unpinned_field_cabac)
            set_error("stream %d: field pictures with CABAC are refused: the context initialisation values of field-coded blocks (ctxIdx 277-398, 436-459) in "
                      "this library's tables are unpinned (h264mi_config.allow_unpinned_field_cabac = 1 decodes with them); CAVLC field pictures are decoded", si);
            return H264MI_EUNSUPPORTED;
        }
        if (ref_idc && type != 5 && sh.adaptive_ref_pic_marking_mode_flag)
            for (int k = 0; k < sh.n_memory_management_control_operations; k++)
                if (sh.memory_management_control_operation[k] != 1) {
                    set_error("stream %d: memory_management_control_operation %d in a field picture is out of scope (operation 1 is implemented)", si,
                              sh.memory_management_control_operation[k]);
                    return H264MI_EUNSUPPORTED;
                }
    }
    if (sps.max_num_ref_frames > d->cfg.max_ref_frames) {
        set_error("stream %d: max_num_ref_frames %d exceeds the configured max_ref_frames %d", si, sps.max_num_ref_frames, d->cfg.max_ref_frames);
        return H264MI_ECAPACITY;
    }
    const int wmb = sps.pic_width_in_mbs, hmb = sps.pic_height_in_mbs; // of the frame
    const int hmb_pic = sh.field_pic ? hmb / 2 : hmb;                   // of this picture (h264/slice.go:159-176 PicHeightInMbs)
    if (wmb * 16 > d->Wmax || hmb * 16 > d->Hmax || hmb > 320) {
        set_error("stream %d: %dx%d exceeds the configured maximum %dx%d", si, wmb * 16, hmb * 16, d->Wmax, d->Hmax);
        return H264MI_ECAPACITY;
    }
    // (7.4.1.2.4 cannot tell two pictures apart whose headers agree -- e.g. POC type 2 and the frame_num 1 that follows a memory
    // management operation 5 in a picture with frame_num 1 --: a slice that starts where a slice of the current picture already
    // started begins a new picture whatever the headers say.  Not "first_mb_in_slice == 0": with slice groups or arbitrary slice
    // order that slice may come late.)
    const bool restarts = std::find(s.cur_first_mbs.begin(), s.cur_first_mbs.end(), sh.first_mb_in_slice) != s.cur_first_mbs.end();
    if (type == 5) s.lead = s.skipping = false; // the counts start over: nothing after this precedes the entry picture
    if (s.lead && !entry) {
        // random access, leading pictures: a picture behind the non-IDR entry picture in decoding order and in front of it in output order predicts
        // from pictures the stream never had -- it is neither decoded nor output (Dpb::skip_picture)
        if (s.skipping && !new_picture(sps, s.skip_sh, sh) && sh.first_mb_in_slice != s.skip_sh.first_mb_in_slice) return H264MI_OK; // one more slice of it
        s.skipping = false;
        if (s.dpb.cur_slot < 0 || restarts || new_picture(sps, s.dpb.first_sh, sh)) { // the first slice of a picture
            if (s.dpb.cur_slot >= 0) finish_picture(d, si); // (its marking may move the counts: operation 5)
            if (s.lead && s.dpb.peek_poc(sps, sh) < s.lead_poc) {
                r = flush_pending_field(d, si, &sps, &pps, &sh); // (a lone first field: its second field would not have been a leading picture)
                if (r == H264MI_OK) r = fill_frame_num_gap(d, si, sps, sh);
                if (r != H264MI_OK) return r;
                if (!s.dpb.skip_picture(sps, sh)) {
                    set_error("stream %d: frame pool exhausted", si);
                    return H264MI_ECAPACITY;
                }
                s.skipping = true, s.skip_sh = sh;
                s.ra.skipped_leading_pictures++;
                s.sei = {0, 0, 0, 0, 0};
                return H264MI_OK;
            }
        }
    }
    if (s.dpb.cur_slot >= 0 && (restarts || new_picture(sps, s.dpb.first_sh, sh))) finish_picture(d, si);
    if (s.active_sps != pps.sps_id || s.wmb != wmb || s.hmb != hmb) { // (re)activate: new sequence geometry
        if (sh.nal_unit_type != 5 && s.active_sps >= 0 && (s.wmb != wmb || s.hmb != hmb)) {
            set_error("stream %d: picture size changes without an IDR", si);
            return H264MI_EBITSTREAM;
        }
        r = flush_pending_field(d, si, &sps, &pps, &sh); // (a lone first field of the old sequence goes out before anything of the new one)
        if (r != H264MI_OK) return r;
        s.active_sps = pps.sps_id, s.wmb = wmb, s.hmb = hmb;
    }
    if (s.dpb.cur_slot < 0) { // first slice of a new picture
        // the second field of the frame whose first field was the previous picture (7.4.1.2.4, 3.30 / 3.31): opposite parity, same frame_num, not
        // an IDR picture, reference or not like the first one
        bool second = false;
        if (s.dpb.pend_slot >= 0) {
            const Slot &f = s.dpb.slots[s.dpb.pend_slot];
            if (sh.field_pic && type != 5 && !entry && f.fields == (sh.bottom_field ? 1 : 2) && f.frame_num == sh.frame_num && (f.ref != 0) == (ref_idc != 0))
                second = true;
            else if ((r = flush_pending_field(d, si, &sps, &pps, &sh)) != H264MI_OK)
                return r;
        }
        if (!second) {
            r = d->conceal_pics ? conceal_frame_num_gap(d, si, sps, pps, pps_id, sh) : 1;
            if (r == 1) r = fill_frame_num_gap(d, si, sps, sh);
            if (r != H264MI_OK) return r;
        }
        r = start_picture(d, si, sps, pps, pps_id, sh, type, second);
        if (r != H264MI_OK) return r;
        // random access: what the access unit said about it goes with the frame (h264mi_frame_entry: a second field adds nothing); a non-IDR entry
        // picture starts a sequence of its own, and what has a smaller count than it from now on is a leading picture
        if (OutFrame *of = second ? nullptr : (sh.field_pic ? &s.pend_out : &g.out[si].back())) {
            of->rp = s.sei, of->entry = entry;
            if (entry && type != 5) of->new_sequence = 1;
        }
        s.sei = {0, 0, 0, 0, 0};
        s.decoded_any = true;
        if (entry && type != 5) s.lead_poc = sh.field_pic ? s.dpb.slots[s.dpb.cur_slot].fpoc[sh.bottom_field ? 1 : 0] : s.dpb.slots[s.dpb.cur_slot].poc;
        if (s.lead && ref_idc && sh.adaptive_ref_pic_marking_mode_flag)
            for (int k = 0; k < sh.n_memory_management_control_operations; k++)
                if (sh.memory_management_control_operation[k] == 5) s.lead = false; // the counts start over
    }
    if (s.cur_slices >= d->cfg.max_slices_per_frame) {
        set_error("stream %d: more than %d slices in a frame", si, d->cfg.max_slices_per_frame);
        return H264MI_ECAPACITY;
    }
    if (sh.first_mb_in_slice >= wmb * hmb_pic) return H264MI_EBITSTREAM;
    s.cur_first_mbs.push_back(sh.first_mb_in_slice);
    PicDesc &pd = g.h_pics[s.cur_pic];
    SliceDesc &sd = g.h_slices[g.n_slices];
    memset(&sd, 0, sizeof(sd));
    sd.rbsp_off = static_cast<uint32_t>(off), sd.rbsp_size = static_cast<uint32_t>(rlen);
    sd.data_bit_off = static_cast<uint32_t>(sh.slice_data_bit_offset);
    {
        size_t n = rlen;
        while (n > 0 && rbsp[n - 1] == 0) n--;
        sd.stop_bit = n ? static_cast<uint32_t>((n - 1) * 8 + 7 - __builtin_ctz(rbsp[n - 1])) : 0;
    }
    sd.pic_idx = s.cur_pic, sd.first_mb = sh.first_mb_in_slice;
    sd.slice_type = static_cast<uint8_t>(st);
    sd.cabac_init_idc = static_cast<uint8_t>(sh.cabac_init), sd.slice_qp = static_cast<uint8_t>(sh.slice_qp_y);
    sd.num_ref_idx_active = static_cast<uint8_t>(st != 2 ? sh.num_ref_idx_l0_active_minus1 + 1 : 0);
    sd.alpha_off = static_cast<int8_t>(2 * sh.slice_alpha_c0_offset_div2), sd.beta_off = static_cast<int8_t>(2 * sh.slice_beta_offset_div2);
    sd.dbf_idc = static_cast<uint8_t>(sh.disable_deblocking_filter);
    sd.slice_in_pic = static_cast<uint16_t>(s.cur_slices);
    for (int i = 0; i < MI_MAX_REFS; i++) sd.ref_slot[i] = -1;
    int level = 0;
    // PicOrderCnt of the current picture and of a list entry (list_entry_poc): a field's own count in a field picture, the frame's otherwise
    const bool fieldpic = sh.field_pic != 0;
    const int cur_poc = fieldpic ? s.dpb.slots[s.dpb.cur_slot].fpoc[sh.bottom_field ? 1 : 0] : s.dpb.slots[s.dpb.cur_slot].poc;
    if (st != 2) {
        pd.is_intra_only = 0;
        const bool bslice = st == 1;
        const bool explicit_wp = bslice ? pps.weighted_bipred == 1 : pps.weighted_pred != 0;
        BSliceExt bx;
        memset(&bx, 0, sizeof(bx));
        r = s.dpb.build_ref_lists(sps, sh, bslice, sd.ref_slot, bx.ref_slot1);
        if (r != H264MI_OK) return r;
        for (int i = 0; i <= sh.num_ref_idx_l0_active_minus1 && i < MI_MAX_REFS; i++) wave_after(g, s.dpb, s.cur_pic, sd.ref_slot[i]);
        if (bslice)
            for (int i = 0; i <= sh.num_ref_idx_l1_active_minus1 && i < MI_MAX_REFS; i++) wave_after(g, s.dpb, s.cur_pic, bx.ref_slot1[i]);
        sd.wp_flag = static_cast<uint8_t>(explicit_wp);
        sd.luma_log2_denom = static_cast<uint8_t>(sh.luma_log2_weight_denom), sd.chroma_log2_denom = static_cast<uint8_t>(sh.chroma_log2_weight_denom);
        for (int i = 0; i < MI_MAX_REFS; i++) {
            sd.wp_lw[i] = static_cast<int16_t>(explicit_wp ? sh.luma_weight_l0[i] : 1), sd.wp_lo[i] = static_cast<int16_t>(sh.luma_offset_l0[i]);
            for (int j = 0; j < 2; j++)
                sd.wp_cw[i][j] = static_cast<int16_t>(explicit_wp ? sh.chroma_weight_l0[i][j] : 1), sd.wp_co[i][j] = static_cast<int16_t>(sh.chroma_offset_l0[i][j]);
        }
        if (bslice) {
            r = ensure_b_buffers(d);
            if (r != H264MI_OK) return r;
            pd.has_b = 1;
            auto entry_slot = [&](int e) -> const Slot & { return s.dpb.slots[fieldpic ? MI_REF_SLOT(e) : e]; };
            const int n0 = sh.num_ref_idx_l0_active_minus1 + 1, n1 = sh.num_ref_idx_l1_active_minus1 + 1;
            bx.num_ref_idx_l1_active = static_cast<uint8_t>(n1);
            bx.direct_spatial = static_cast<uint8_t>(sh.direct_spatial_mv_pred), bx.direct_8x8_inference = static_cast<uint8_t>(sps.direct_8x8_inference);
            bx.wp_mode = static_cast<uint8_t>(pps.weighted_bipred);
            for (int i = 0; i < MI_MAX_REFS; i++) {
                bx.wp_lw1[i] = static_cast<int16_t>(explicit_wp ? sh.luma_weight_l1[i] : 1), bx.wp_lo1[i] = static_cast<int16_t>(sh.luma_offset_l1[i]);
                for (int j = 0; j < 2; j++)
                    bx.wp_cw1[i][j] = static_cast<int16_t>(explicit_wp ? sh.chroma_weight_l1[i][j] : 1), bx.wp_co1[i][j] = static_cast<int16_t>(sh.chroma_offset_l1[i][j]);
            }
            // POC distances: DistScaleFactor of temporal direct prediction (8.4.1.2.3) per refIdxL0 against RefPicList1[0], and the
            // implicit bi-prediction weights (8.4.2.3.1) per (refIdxL0, refIdxL1)
            auto dist_scale = [&](int slot0, int slot1, bool *copy) {
                const Slot &p0 = entry_slot(slot0);
                const int poc0 = list_entry_poc(s.dpb, slot0, fieldpic), poc1 = list_entry_poc(s.dpb, slot1, fieldpic);
                const int tb = std::min(std::max(cur_poc - poc0, -128), 127), td = std::min(std::max(poc1 - poc0, -128), 127);
                *copy = td == 0 || p0.ref == 2;
                if (td == 0) return 256;
                const int tx = (16384 + std::abs(td / 2)) / td;
                return std::min(std::max((tb * tx + 32) >> 6, -1024), 1023);
            };
            const int col_slot = bx.ref_slot1[0];
            for (int i = 0; i < MI_MAX_REFS; i++) {
                bool copy = true;
                int dsf = 256;
                if (i < n0 && sd.ref_slot[i] >= 0 && col_slot >= 0) dsf = dist_scale(sd.ref_slot[i], col_slot, &copy);
                bx.dist_scale[i] = static_cast<int16_t>(copy ? 256 : dsf);
                for (int j = 0; j < MI_MAX_REFS; j++) {
                    int w1 = 32;
                    if (i < n0 && j < n1 && sd.ref_slot[i] >= 0 && bx.ref_slot1[j] >= 0) {
                        bool cp;
                        const int f = dist_scale(sd.ref_slot[i], bx.ref_slot1[j], &cp) >> 2;
                        const int td = list_entry_poc(s.dpb, bx.ref_slot1[j], fieldpic) - list_entry_poc(s.dpb, sd.ref_slot[i], fieldpic);
                        if (td != 0 && entry_slot(sd.ref_slot[i]).ref != 2 && entry_slot(bx.ref_slot1[j]).ref != 2 && f >= -64 && f <= 128) w1 = f;
                    }
                    bx.implicit_w1[i][j] = static_cast<int16_t>(w1);
                }
            }
            // the co-located picture: its motion record array, and when its slices are entropy-decoded relative to this one
            level = 1;
            if (col_slot >= 0) {
                const Slot &cs = entry_slot(col_slot);
                const int cslot = fieldpic ? MI_REF_SLOT(col_slot) : col_slot, cpar = fieldpic && (col_slot & MI_REF_PARITY) ? 1 : 0;
                // the co-located picture must have the structure of the current one (8.4.1.2.1's frame-from-field-pair and field-from-frame
                // cases, with their vertical vector scaling, are not implemented)
                if (cs.field_coded != fieldpic && !cs.nonexisting) {
                    set_error("stream %d: a B %s whose RefPicList1[0] was coded as %s is out of scope (direct prediction across picture structures)", si,
                              fieldpic ? "field" : "frame picture", cs.field_coded ? "field pictures" : "a frame picture");
                    return H264MI_EUNSUPPORTED;
                }
                bx.col = colrec_of(d, si, cslot, cpar);
                bx.col_short = cs.ref == 1;
                const int cpic = fieldpic ? cs.fpic[cpar] : cs.pic;
                if (cpic >= 0) {
                    level = g.pics[cpic].level + 1;
                    g.pics[cpic].save_col = 1;
                } else if (!cs.col_valid[cpar] && !cs.nonexisting) {
                    // decoded by an earlier batch, before this decoder kept motion (the arrays exist from the first B slice on, ensure_b_buffers):
                    // direct prediction from it would silently see an intra picture
                    set_error("stream %d: the co-located picture of a B slice was decoded before the decoder's first B slice; its motion was not kept", si);
                    return H264MI_EUNSUPPORTED;
                }
            }
            sd.bext = static_cast<uint32_t>(g.n_bext);
            g.h_bext[g.n_bext++] = bx;
        }
    }
    { // K11: the picture order counts the lists were built with, before a memory management operation 5 of this picture rewrites them
        g.slices.resize(g.n_slices), g.slices.emplace_back();
        g.slices[g.n_slices].level = level;
        Stage::SliceRefs &sr = g.slices[g.n_slices].refs;
        sr.cur_poc = cur_poc;
        const int16_t *lists[2] = {st != 2 ? sd.ref_slot : nullptr, st == 1 ? g.h_bext[sd.bext].ref_slot1 : nullptr};
        const int active[2] = {sh.num_ref_idx_l0_active_minus1 + 1, sh.num_ref_idx_l1_active_minus1 + 1};
        for (int l = 0; l < 2; l++) {
            if (!lists[l]) continue;
            sr.n[l] = static_cast<uint8_t>(std::min(std::max(active[l], 0), MI_MAX_REFS));
            for (int i = 0; i < sr.n[l]; i++) sr.poc[l][i] = lists[l][i] >= 0 ? list_entry_poc(s.dpb, lists[l][i], fieldpic) : sr.cur_poc;
        }
    }
    g.pics[s.cur_pic].level = std::max(g.pics[s.cur_pic].level, level);
    g.bits_used = std::max(g.bits_used, off + rlen);
    g.bits_end = std::max(g.bits_end, g.bits_used);
    g.n_slices++;
    s.cur_slices++;
    return H264MI_OK;
}
