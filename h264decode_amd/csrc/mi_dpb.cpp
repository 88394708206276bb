// h264decode_amd/csrc/mi_dpb.cpp -- picture management (8.2) of one stream: see mi_dpb.hpp.
#include "mi_dpb.hpp"
#include <algorithm>
#include <cstring>
#include <utility>
#include "mi_parse.hpp"

namespace mi {

static int max_frame_num(const h264mi_sps &sps) { return 1 << (sps.log2_max_frame_num_minus4 + 4); }
// FrameNumWrap (8-27) of a short-term frame as a picture with frame_num `cur` sees it (never stored: it depends on who asks); on picture numbers, picNumLX of 8-34 / 8-37
static int frame_num_wrap(int frame_num, int cur, int max_fn) { return frame_num > cur ? frame_num - max_fn : frame_num; }

void Dpb::reset() {
    for (auto &sl : slots) sl = Slot();
    cur_slot = -1, cur_field = 0, cur_second = false, pend_slot = -1, skipped_slot = -1;
    prev_poc_msb = prev_poc_lsb = prev_frame_num = prev_frame_num_offset = prev_ref_frame_num = 0;
}
void Dpb::drop_references() { for (auto &sl : slots) sl.ref = 0; }
void Dpb::begin_batch() {
    for (auto &sl : slots) sl.held = sl.ref != 0, sl.pic = sl.fpic[0] = sl.fpic[1] = -1; // reference pictures at batch start stay put for the whole batch
    if (pend_slot >= 0) slots[pend_slot].held = true; // a first field waiting for its second one
    cur_slot = -1;
}
int Dpb::first_free_slot() const {
    for (int i = 0; i < static_cast<int>(slots.size()); i++)
        if (!slots[i].ref && !slots[i].held) return i;
    return -1;
}
int Dpb::free_slots() const { return static_cast<int>(std::count_if(slots.begin(), slots.end(), [](const Slot &sl) { return !sl.ref && !sl.held; })); }

int Dpb::compute_poc(const h264mi_sps &sps, const h264mi_slice_header &sh) { // 8.2.1
    const bool idr = sh.nal_unit_type == 5;
    const int max_fn = max_frame_num(sps);
    int poc = 0;
    if (sps.pic_order_count_type == 0) {
        const int max_lsb = 1 << (sps.log2_max_pic_order_cnt_lsb_min4 + 4);
        int prev_msb = idr ? 0 : prev_poc_msb, prev_lsb = idr ? 0 : prev_poc_lsb, msb;
        if (sh.pic_order_cnt_lsb < prev_lsb && prev_lsb - sh.pic_order_cnt_lsb >= max_lsb / 2)
            msb = prev_msb + max_lsb;
        else if (sh.pic_order_cnt_lsb > prev_lsb && sh.pic_order_cnt_lsb - prev_lsb > max_lsb / 2)
            msb = prev_msb - max_lsb;
        else
            msb = prev_msb;
        const int top = msb + sh.pic_order_cnt_lsb, bot = top + sh.delta_pic_order_cnt_bottom; // (8-4 / 8-5: a field picture has the one count, delta is 0)
        poc = std::min(top, bot);
        top_above_poc = top - poc;
        poc_top = top, poc_bot = bot;
        if (sh.nal_ref_idc) prev_poc_msb = msb, prev_poc_lsb = sh.pic_order_cnt_lsb;
    } else {
        int fno = idr ? 0 : (prev_frame_num > sh.frame_num ? prev_frame_num_offset + max_fn : prev_frame_num_offset);
        if (sps.pic_order_count_type == 1) {
            int n = sps.num_ref_frames_in_pic_order_cnt_cycle;
            int abs_fn = n ? fno + sh.frame_num : 0;
            if (!sh.nal_ref_idc && abs_fn > 0) abs_fn--;
            int expected = 0;
            if (abs_fn > 0) {
                int cyc = (abs_fn - 1) / n, in_cyc = (abs_fn - 1) % n, delta = 0;
                for (int i = 0; i < n; i++) delta += sps.offset_for_ref_frame_list[i];
                expected = cyc * delta;
                for (int i = 0; i <= in_cyc; i++) expected += sps.offset_for_ref_frame_list[i];
            }
            if (!sh.nal_ref_idc) expected += sps.offset_for_non_ref_pic;
            const int top = expected + sh.delta_pic_order_cnt[0], bot = top + sps.offset_for_top_to_bottom_field + sh.delta_pic_order_cnt[1];
            if (sh.field_pic) // 8-10: a bottom field is at expected + offset_for_top_to_bottom_field + delta_pic_order_cnt[0]
                poc = sh.bottom_field ? expected + sps.offset_for_top_to_bottom_field + sh.delta_pic_order_cnt[0] : top, poc_top = poc_bot = poc;
            else
                poc = std::min(top, bot), poc_top = top, poc_bot = bot;
        } else {
            poc = idr ? 0 : (sh.nal_ref_idc ? 2 * (fno + sh.frame_num) : 2 * (fno + sh.frame_num) - 1);
            poc_top = poc_bot = poc;
        }
        prev_frame_num_offset = fno;
    }
    prev_frame_num = sh.frame_num;
    return poc;
}

void Dpb::begin_picture(const h264mi_sps &sps, const h264mi_slice_header &sh, int slot, bool second, int pic) {
    cur_slot = slot, first_sh = sh;
    cur_field = sh.field_pic ? 1 + (sh.bottom_field ? 1 : 0) : 0, cur_second = second;
    if (second) pend_slot = -1; // (it is the current picture's frame now; back in pend_slot only if it still lacks a field when this picture ends)
    Slot &sl = slots[slot];
    if (!second) {
        sl = Slot();
        sl.held = true, sl.frame_num = sh.frame_num, sl.field_coded = sh.field_pic != 0;
    }
    const int pic_poc = compute_poc(sps, sh);
    if (sh.field_pic) {
        sl.fpoc[sh.bottom_field ? 1 : 0] = pic_poc;
        sl.fpic[sh.bottom_field ? 1 : 0] = pic;
        if (!second) sl.poc = pic_poc;
    } else {
        sl.poc = pic_poc, sl.fpoc[0] = poc_top, sl.fpoc[1] = poc_bot;
        sl.fields = 3; // (a frame picture delivers both fields; it is not in its own reference lists)
        sl.pic = pic;
    }
}

// The reference frames a picture with this frame_num and structure (0 frame, 1 top field, 2 bottom field) predicts from -- st: short-term,
// lt: long-term by LongTermFrameIdx -- and its initial lists (8.2.4.2); false: there are none.
// A frame picture (8.2.4.2.1 / 8.2.4.2.3) predicts from frames (or complementary field pairs) of which BOTH fields are reference fields.
// A field picture (8.2.4.2.2 / 8.2.4.2.4 + 8.2.4.2.5): the lists hold FIELDS.  The reference frames are put in order first -- P: by FrameNumWrap, the frame
// of the current field included when this is its second field and the first one is a reference; B: by PicOrderCnt around the current field,
// list 0 the earlier ones nearest first and then the later ones, list 1 the other way round; long-term frames by LongTermFrameIdx --, then
// their fields are taken alternately, the parity of the current field first; a frame that lacks the wanted field is passed over, and when one
// parity is used up the rest of the other one follows in order.
bool Dpb::initial_lists(const h264mi_sps &sps, int frame_num, int field, bool bslice, std::vector<int> &st, std::vector<int> &lt, std::vector<int> lists[2]) const {
    const int max_fn = max_frame_num(sps), bottom = field == 2;
    for (int i = 0; i < static_cast<int>(slots.size()); i++) {
        const Slot &sl = slots[i];
        if (field ? i == cur_slot && !(cur_second && sl.ref == 1) : i == cur_slot) continue; // (a second field may predict from the first field of its frame)
        if (!field && sl.ref && (sl.fields != 3 || sl.funref)) continue;
        if (sl.ref) (sl.ref == 1 ? st : lt).push_back(i);
    }
    std::sort(lt.begin(), lt.end(), [&](int a, int b) { return slots[a].long_idx < slots[b].long_idx; });
    if (st.empty() && lt.empty()) return false;
    auto wrap = [&](int i) { return frame_num_wrap(slots[i].frame_num, frame_num, max_fn); };
    if (!bslice) // PicNum / FrameNumWrap descending
        std::sort(st.begin(), st.end(), [&](int a, int b) { return wrap(a) > wrap(b); });
    if (!field) {
        if (!bslice) // 8.2.4.2.1: then LongTermPicNum ascending
            lists[0] = st;
        else { // 8.2.4.2.3: by PicOrderCnt relative to the current picture
            const int cur_poc = slots[cur_slot].poc;
            std::vector<int> before, after;
            for (int i : st) {
                if (slots[i].nonexisting && !slots[i].poc_known && sps.pic_order_count_type == 0) continue; // 8.2.4.2.3: no PicOrderCnt, not in the lists of B slices
                (slots[i].poc < cur_poc ? before : after).push_back(i);
            }
            std::sort(before.begin(), before.end(), [&](int a, int b) { return slots[a].poc > slots[b].poc; });
            std::sort(after.begin(), after.end(), [&](int a, int b) { return slots[a].poc < slots[b].poc; });
            lists[0] = before;
            lists[0].insert(lists[0].end(), after.begin(), after.end());
            lists[1] = after;
            lists[1].insert(lists[1].end(), before.begin(), before.end());
            lists[1].insert(lists[1].end(), lt.begin(), lt.end());
        }
        lists[0].insert(lists[0].end(), lt.begin(), lt.end());
    } else {
        std::vector<int> ord[2];
        if (!bslice)
            ord[0] = st;
        else {
            // PicOrderCnt of a reference frame here: the smaller of its fields' (Slot::poc); of the current frame (second field): its first field's
            const int cur_poc = slots[cur_slot].fpoc[bottom];
            std::vector<std::pair<int, int>> before, after; // (PicOrderCnt, slot)
            for (int i : st) {
                if (slots[i].nonexisting && !slots[i].poc_known) continue;
                const int fp = i == cur_slot ? slots[i].fpoc[!bottom] : slots[i].poc;
                (fp <= cur_poc ? before : after).push_back({fp, i});
            }
            std::stable_sort(before.begin(), before.end(), [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.first > b.first; });
            std::stable_sort(after.begin(), after.end(), [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.first < b.first; });
            for (auto &e : before) ord[0].push_back(e.second);
            for (auto &e : after) ord[0].push_back(e.second), ord[1].push_back(e.second);
            for (auto &e : before) ord[1].push_back(e.second);
        }
        for (int l = 0; l < (bslice ? 2 : 1); l++)
            for (int grp = 0; grp < 2; grp++) { // short-term frames, then long-term frames: each group alternates on its own
                const std::vector<int> &fr = grp ? lt : ord[l];
                const int nfr = static_cast<int>(fr.size());
                int a = 0, b = 0; // next frame to look at for the same / the opposite parity
                for (int want_same = 1;; want_same ^= 1) {
                    int &cursor = want_same ? a : b;
                    const int par = want_same ? bottom : !bottom;
                    while (cursor < nfr && !slots[fr[cursor]].ref_field(par)) cursor++;
                    if (cursor == nfr) { // this parity is used up: the rest of the other one
                        int &other = want_same ? b : a;
                        for (; other < nfr; other++)
                            if (slots[fr[other]].ref_field(!par)) lists[l].push_back(fr[other] | (!par ? MI_REF_PARITY : 0));
                        break;
                    }
                    lists[l].push_back(fr[cursor] | (par ? MI_REF_PARITY : 0));
                    cursor++;
                }
            }
    }
    if (bslice && lists[1].size() > 1 && lists[1] == lists[0]) std::swap(lists[1][0], lists[1][1]);
    return true;
}

int Dpb::initial_p_entry0(const h264mi_sps &sps, int frame_num, int field) const {
    std::vector<int> st, lt, lists[2];
    return initial_lists(sps, frame_num, field, false, st, lt, lists) && !lists[0].empty() ? lists[0][0] : -1;
}

int Dpb::second_field_p_entry0(const h264mi_sps &sps, int frame_num, int field) {
    if (pend_slot < 0 || cur_slot >= 0) return -1;
    const bool was_second = cur_second;
    cur_slot = pend_slot, cur_second = true; // (what the list looks at of the picture under construction)
    const int e = initial_p_entry0(sps, frame_num, field);
    cur_slot = -1, cur_second = was_second;
    return e;
}

int Dpb::build_ref_lists(const h264mi_sps &sps, const h264mi_slice_header &sh, bool bslice, int16_t *out0 /*MI_MAX_REFS*/, int16_t *out1) const {
    const bool field = sh.field_pic != 0;
    const int max_fn = max_frame_num(sps), bottom = sh.bottom_field ? 1 : 0;
    std::vector<int> st, lt, lists[2];
    if (!initial_lists(sps, sh.frame_num, field ? 1 + bottom : 0, bslice, st, lt, lists)) {
        set_error("P/B slice without reference pictures");
        return H264MI_EBITSTREAM;
    }
    const int max_pic_num = field ? 2 * max_fn : max_fn, cur_pic_num = field ? 2 * sh.frame_num + 1 : sh.frame_num; // 8.2.4.1: MaxPicNum, CurrPicNum
    // the list entry with this picNum (among `frames` = st) / LongTermPicNum (lt); -1: none.  A frame's number is its FrameNumWrap / LongTermFrameIdx n; a field's
    // 2 n + 1 if it has the parity of the current field, 2 n otherwise (8.2.4.1)
    auto entry_of = [&](const std::vector<int> &frames, bool long_term, int num) {
        int target = -1;
        for (int i : frames) {
            const int n = long_term ? slots[i].long_idx : frame_num_wrap(slots[i].frame_num, sh.frame_num, max_fn);
            if (!field && n == num) target = i;
            for (int par = 0; field && par < 2; par++)
                if (slots[i].ref_field(par) && 2 * n + (par == bottom) == num) target = i | (par ? MI_REF_PARITY : 0);
        }
        return target;
    };
    for (int l = 0; l < (bslice ? 2 : 1); l++) {
        std::vector<int> &list = lists[l];
        const int nact = (l ? sh.num_ref_idx_l1_active_minus1 : sh.num_ref_idx_l0_active_minus1) + 1;
        if (nact > MI_MAX_REFS) {
            set_error(field ? "num_ref_idx_l%d_active %d > %d reference fields is out of scope" : "num_ref_idx_l%d_active %d > %d (field refs are out of scope)", l, nact, MI_MAX_REFS);
            return H264MI_EUNSUPPORTED;
        }
        list.resize(nact, -1); // the initial list is cut (or padded with "no reference picture") to the active size
        list.resize(nact + 1, -1);
        const int32_t *idcs = l ? sh.modification_of_pic_nums_l1 : sh.modification_of_pic_nums, *vals = l ? sh.modification_value_l1 : sh.modification_value;
        const int nmod = l ? sh.n_ref_pic_list_modifications_l1 : sh.n_ref_pic_list_modifications;
        if (l ? sh.ref_pic_list_modification_flag_l1 : sh.ref_pic_list_modification_flag_l0) { // 8.2.4.3
            int pred = cur_pic_num, idx = 0;
            for (int k = 0; k < nmod && idx < nact; k++) {
                int target;
                if (idcs[k] < 2) {
                    const int diff = vals[k] + 1;
                    if (idcs[k] == 0) {
                        pred -= diff;
                        if (pred < 0) pred += max_pic_num;
                    } else {
                        pred += diff;
                        if (pred >= max_pic_num) pred -= max_pic_num;
                    }
                    target = entry_of(st, false, frame_num_wrap(pred, cur_pic_num, max_pic_num));
                } else
                    target = entry_of(lt, true, vals[k]);
                if (target < 0) {
                    set_error(field ? "ref_pic_list_modification names a missing field" : "ref_pic_list_modification names a missing picture");
                    return H264MI_EBITSTREAM;
                }
                for (int c = nact; c > idx; c--) list[c] = list[c - 1];
                list[idx++] = target;
                int nidx = idx;
                for (int c = idx; c <= nact; c++)
                    if (list[c] != target) list[nidx++] = list[c];
            }
        }
        int16_t *out = l ? out1 : out0;
        for (int i = 0; i < MI_MAX_REFS; i++) out[i] = static_cast<int16_t>(i < nact ? list[i] : -1);
    }
    return H264MI_OK;
}

// 8.2.5.3 for a picture with this frame_num (the one under construction, if any, does not count): when the window is full the short-term
// frame with the smallest FrameNumWrap leaves it
void Dpb::sliding_window(const h264mi_sps &sps, int frame_num) {
    const int max_fn = max_frame_num(sps), maxref = std::max(sps.max_num_ref_frames, 1);
    int nref = 0;
    Slot *oldest = nullptr;
    for (int i = 0; i < static_cast<int>(slots.size()); i++) {
        Slot &sl = slots[i];
        if (i == cur_slot || !sl.ref) continue;
        nref++;
        if (sl.ref == 1 && (!oldest || frame_num_wrap(sl.frame_num, frame_num, max_fn) < frame_num_wrap(oldest->frame_num, frame_num, max_fn))) oldest = &sl;
    }
    if (nref >= maxref && oldest) oldest->ref = 0;
}

void Dpb::free_long_term_idx(int idx) { // the long-term frame that holds LongTermFrameIdx idx, if any, is no reference any more
    for (auto &o : slots)
        if (o.ref == 2 && o.long_idx == idx) o.ref = 0;
}

// 8.2.5: marking after the current picture is complete
void Dpb::mark_reference(const h264mi_sps &sps) {
    const h264mi_slice_header &sh = first_sh;
    Slot &cur = slots[cur_slot];
    const int max_fn = max_frame_num(sps);
    if (sh.nal_ref_idc) prev_ref_frame_num = sh.frame_num; // (operation 5 below: 0)
    if (cur_field && sh.nal_ref_idc && sh.nal_unit_type != 5 && sh.adaptive_ref_pic_marking_mode_flag) {
        // 8.2.5.4.1 in a field picture: picNumX names a FIELD (8.2.4.1); the frame stays in the window while its other field is a reference.
        // (operations 2..6 on fields were refused when the picture started)
        const int bottom = cur_field == 2, cur_pic_num = 2 * sh.frame_num + 1;
        for (int k = 0; k < sh.n_memory_management_control_operations; k++) {
            const int picnum = cur_pic_num - (sh.mmco_arg1[k] + 1);
            for (auto &sl : slots) {
                if (sl.ref != 1) continue;
                const int wrap = frame_num_wrap(sl.frame_num, sh.frame_num, max_fn);
                for (int par = 0; par < 2; par++)
                    if (sl.ref_field(par) && 2 * wrap + (par == bottom) == picnum) {
                        sl.funref |= 1 << par;
                        if (!(sl.fields & ~sl.funref)) sl.ref = 0; // (the current frame, whose other field is being decoded, is marked just below)
                    }
            }
        }
        cur.ref = 1;
        return;
    }
    // 8.2.5.3: the second field of a frame whose first field is a reference joins it; nothing leaves the window
    if (cur_field && cur_second && cur.ref) return;
    if (!sh.nal_ref_idc) {
        cur.ref = 0;
        return;
    }
    if (sh.nal_unit_type == 5) {
        drop_references();
        cur.ref = sh.long_term_reference_flag ? 2 : 1;
        cur.long_idx = 0;
        return;
    }
    cur.ref = 1;
    if (!sh.adaptive_ref_pic_marking_mode_flag) {
        sliding_window(sps, sh.frame_num);
        return;
    }
    for (int k = 0; k < sh.n_memory_management_control_operations; k++) {
        const int op = sh.memory_management_control_operation[k];
        if (op == 1 || op == 3) {
            const int picnum = sh.frame_num - (sh.mmco_arg1[k] + 1);
            for (auto &sl : slots)
                if (&sl != &cur && sl.ref == 1 && frame_num_wrap(sl.frame_num, sh.frame_num, max_fn) == picnum) {
                    if (op == 1)
                        sl.ref = 0;
                    else {
                        free_long_term_idx(sh.mmco_arg2[k]);
                        sl.ref = 2, sl.long_idx = sh.mmco_arg2[k];
                    }
                }
        } else if (op == 2)
            free_long_term_idx(sh.mmco_arg1[k]);
        else if (op == 4) {
            for (auto &sl : slots)
                if (sl.ref == 2 && sl.long_idx >= sh.mmco_arg1[k]) sl.ref = 0;
        } else if (op == 5) {
            for (auto &sl : slots)
                if (&sl != &cur) sl.ref = 0;
            cur.frame_num = 0, cur.poc = 0; // 8.2.1: tempPicOrderCnt is subtracted, the picture ends up at PicOrderCnt 0
            const int m = std::min(cur.fpoc[0], cur.fpoc[1]);
            cur.fpoc[0] -= m, cur.fpoc[1] -= m;
            prev_frame_num = prev_frame_num_offset = prev_poc_msb = prev_ref_frame_num = 0;
            // 8.2.1.1: prevPicOrderCntLsb = TopFieldOrderCnt after tempPicOrderCnt was subtracted -- 0 unless the bottom field is the earlier one
            prev_poc_lsb = sps.pic_order_count_type == 0 ? top_above_poc : 0;
        } else if (op == 6) {
            free_long_term_idx(sh.mmco_arg2[k]);
            cur.ref = 2, cur.long_idx = sh.mmco_arg2[k];
        }
    }
}

void Dpb::finish_picture(const h264mi_sps &sps) {
    mark_reference(sps);
    if (!cur_field) return;
    Slot &cur = slots[cur_slot];
    cur.fields |= 1 << (cur_field - 1);
    cur.poc = cur.fields == 3 ? std::min(cur.fpoc[0], cur.fpoc[1]) : cur.fpoc[cur_field - 1];
    pend_slot = cur.fields == 3 ? -1 : cur_slot; // a first field waits for the second one
}

int Dpb::missing_frames(const h264mi_sps &sps, const h264mi_slice_header &sh) const {
    if (sh.nal_unit_type == 5 || sh.frame_num == prev_ref_frame_num) return 0;
    const int max_fn = max_frame_num(sps);
    return (sh.frame_num - (prev_ref_frame_num + 1) % max_fn + max_fn) % max_fn;
}

bool Dpb::add_nonexisting_frame(const h264mi_sps &sps, int fn) {
    sliding_window(sps, fn); // 8.2.5.3 with this frame as the current one
    const int slot = first_free_slot();
    if (slot < 0) return false;
    Slot &sl = slots[slot];
    sl = Slot();
    sl.ref = 1, sl.nonexisting = true, sl.frame_num = fn, sl.fields = 3;
    if (sps.pic_order_count_type != 0) { // 8.2.1: as a reference frame with this frame_num (keeps FrameNumOffset right across a wrap)
        h264mi_slice_header f;
        memset(&f, 0, sizeof(f));
        f.frame_num = fn, f.nal_ref_idc = 1, f.nal_unit_type = 1;
        sl.poc = compute_poc(sps, f);
    }
    prev_ref_frame_num = fn;
    return true;
}

bool Dpb::start_at_entry(const h264mi_sps &sps, int frame_num) {
    drop_references();
    prev_poc_msb = prev_poc_lsb = prev_frame_num = prev_frame_num_offset = 0;
    prev_ref_frame_num = frame_num;
    skipped_slot = -1;
    // What the sliding window held when the encoder coded this picture is known without having seen it: the max_num_ref_frames - 1 reference frames
    // with the frame_num values before this one's.  They enter as non-existing frames, oldest first, with counts below any the stream can reach and
    // rising with frame_num: behind every real picture in P lists (FrameNumWrap) and in the earlier half of B lists (PicOrderCnt), and IN FRONT of the
    // later half of list 0 -- where the encoder's list has the pictures they stand for.  They leave through the sliding window as those did.
    const int max_fn = max_frame_num(sps), n = std::min(std::max(sps.max_num_ref_frames, 1) - 1, max_fn - 1);
    for (int k = n; k >= 1; k--) {
        const int slot = first_free_slot();
        if (slot < 0) return false;
        Slot &sl = slots[slot];
        sl = Slot();
        sl.ref = 1, sl.nonexisting = true, sl.poc_known = true, sl.frame_num = (frame_num - k + max_fn) % max_fn, sl.fields = 3;
        sl.poc = sl.fpoc[0] = sl.fpoc[1] = -(1 << 24) - 2 * k;
    }
    return true;
}

int Dpb::peek_poc(const h264mi_sps &sps, const h264mi_slice_header &sh) const {
    Dpb history; // (no slots: compute_poc reads and writes the history only)
    history.prev_poc_msb = prev_poc_msb, history.prev_poc_lsb = prev_poc_lsb, history.prev_frame_num = prev_frame_num, history.prev_frame_num_offset = prev_frame_num_offset;
    return history.compute_poc(sps, sh);
}

bool Dpb::skip_picture(const h264mi_sps &sps, const h264mi_slice_header &sh) {
    const int poc = compute_poc(sps, sh);
    if (!sh.nal_ref_idc) return true;
    if (sh.field_pic && skipped_slot >= 0) { // the second field of the frame skipped last?
        Slot &f = slots[skipped_slot];
        if (f.ref == 1 && f.nonexisting && f.poc_known && f.frame_num == sh.frame_num && f.fields == (sh.bottom_field ? 1 : 2)) {
            f.fpoc[sh.bottom_field ? 1 : 0] = poc, f.poc = std::min(f.fpoc[0], f.fpoc[1]), f.fields = 3;
            skipped_slot = -1;
            return true;
        }
    }
    sliding_window(sps, sh.frame_num);
    const int slot = first_free_slot();
    if (slot < 0) return false;
    Slot &sl = slots[slot];
    sl = Slot();
    sl.ref = 1, sl.nonexisting = true, sl.poc_known = true, sl.frame_num = sh.frame_num, sl.poc = poc;
    sl.field_coded = sh.field_pic != 0;
    if (sh.field_pic)
        sl.fields = sh.bottom_field ? 2 : 1, sl.fpoc[0] = sl.fpoc[1] = poc, skipped_slot = slot;
    else
        sl.fields = 3, sl.fpoc[0] = poc_top, sl.fpoc[1] = poc_bot, skipped_slot = -1;
    prev_ref_frame_num = sh.frame_num;
    return true;
}

bool new_picture(const h264mi_sps &sps, const h264mi_slice_header &a, const h264mi_slice_header &b) { // 7.4.1.2.4
    if (a.frame_num != b.frame_num || a.pps_id != b.pps_id) return true;
    if (a.field_pic != b.field_pic || a.bottom_field != b.bottom_field) return true; // (the two fields of a frame are two pictures)
    if ((a.nal_ref_idc == 0) != (b.nal_ref_idc == 0)) return true;
    if ((a.nal_unit_type == 5) != (b.nal_unit_type == 5)) return true;
    if (a.nal_unit_type == 5 && a.idr_pic_id != b.idr_pic_id) return true;
    if (sps.pic_order_count_type == 0 && (a.pic_order_cnt_lsb != b.pic_order_cnt_lsb || a.delta_pic_order_cnt_bottom != b.delta_pic_order_cnt_bottom)) return true;
    if (sps.pic_order_count_type == 1 && (a.delta_pic_order_cnt[0] != b.delta_pic_order_cnt[0] || a.delta_pic_order_cnt[1] != b.delta_pic_order_cnt[1])) return true;
    // not in the list of 7.4.1.2.4, but a consequence of 7.4.3: all slices of a picture carry the same slice_group_change_cycle (the map is the
    // picture's), the same marking script and the same long_term_reference_flag -- a difference means another picture even when frame_num and the
    // picture order count agree (they do after memory management operation 5 resets both)
    if (a.slice_group_change_cycle != b.slice_group_change_cycle) return true;
    if (a.adaptive_ref_pic_marking_mode_flag != b.adaptive_ref_pic_marking_mode_flag || a.n_memory_management_control_operations != b.n_memory_management_control_operations) return true;
    for (int k = 0; k < a.n_memory_management_control_operations; k++)
        if (a.memory_management_control_operation[k] != b.memory_management_control_operation[k] || a.mmco_arg1[k] != b.mmco_arg1[k] || a.mmco_arg2[k] != b.mmco_arg2[k]) return true;
    return false;
}

} // namespace mi
