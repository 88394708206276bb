// h264decode_amd/csrc/mi_dpb.hpp -- picture management (clause 8.2) of one stream, in plain C++: picture order counts (8.2.1), reference picture
// lists (8.2.4), reference marking (8.2.5) with the sliding window and the frames inferred for gaps in frame_num, and the frame slots all of it
// works on.  No device, no batch: mi_picture.cpp places pictures in the batch's tables and asks here which slot, which count, which lists.
#pragma once
#include <cstdint>
#include <vector>
#include "../../include/h264mi.h"
#include "mi_types.h" // MI_MAX_REFS, MI_REF_PARITY / MI_REF_SLOT

namespace mi {

struct Slot {
    int ref = 0; // 0 unused, 1 short-term, 2 long-term
    int frame_num = 0, long_idx = 0, poc = 0;
    // Output of the current batch, or a reference picture at the start of the batch: not reused before the next prepare.
    // (The second half keeps h264mi_batch_execute repeatable: a slot freed by a marking operation in the middle of the
    // batch still holds the samples earlier pictures of the batch predict from.)
    bool held = false;
    bool nonexisting = false; // a frame inferred by the gaps-in-frame_num process (8.2.5.2): a place in the window, no picture
    bool poc_known = false;   // ... a non-existing frame that stands for a leading reference picture (random access): no samples, but its PicOrderCnt -- it keeps its place in the lists of B slices
    int pic = -1; // index into the PicDesc table of the batch being prepared, -1: decoded by an earlier batch (field-coded frames: fpic[])
    // Fields (h264/slice.go:867-872 field_pic_flag / bottom_field_flag; h264/sps.go:316-322).  A frame slot holds both fields of a frame, however
    // they were coded: a frame picture fills both at once (fields = 3), a field picture the rows of its parity.
    int fields = 0;          // decoded fields: bit 0 top, bit 1 bottom
    int funref = 0;          // fields taken out of the reference set one by one (memory_management_control_operation 1 in a field picture, 8.2.5.4.1)
    int fpoc[2] = {0, 0};    // PicOrderCnt of the top / bottom field (8.2.1); `poc` is the frame's: the smaller one, or that of the only field there is
    int fpic[2] = {-1, -1};  // PicDesc of the field pictures decoded by the batch being prepared
    bool field_coded = false;          // coded as field pictures (direct prediction needs a co-located picture of the same structure as the current one)
    bool col_valid[2] = {false, false}; // the ColRec array of the frame / top field [0], the bottom field [1] holds this picture's motion
    bool ref_field(int par) const { return ((fields & ~funref) >> par) & 1; } // the field of parity `par` is decoded and still a reference field
};

struct Dpb {
    std::vector<Slot> slots;
    int prev_poc_msb = 0, prev_poc_lsb = 0, prev_frame_num = 0, prev_frame_num_offset = 0;
    int top_above_poc = 0; // TopFieldOrderCnt - PicOrderCnt of the picture compute_poc() was last asked about (> 0: its bottom field comes first)
    int poc_top = 0, poc_bot = 0; // TopFieldOrderCnt / BottomFieldOrderCnt of that picture (a field picture: both its one count)
    int prev_ref_frame_num = 0; // PrevRefFrameNum (7.4.3): frame_num of the previous reference picture; 0 after an IDR picture or operation 5
    int cur_slot = -1;        // the picture under construction (begin_picture .. finish_picture): its frame slot, -1: there is none
    int cur_field = 0;        // ... is 0 a frame, 1 a top field, 2 a bottom field
    bool cur_second = false;  // ... and the second field of its frame (it may predict from the first one)
    h264mi_slice_header first_sh; // ... its first slice: what marking reads
    // A frame whose first field has been decoded waits here for its second field (the next picture, if it is a field of the other parity
    // with the same frame_num, 7.4.1.2.4 / 3.30).  The wait may span a batch boundary.
    int pend_slot = -1;
    int skipped_slot = -1; // skip_picture: the frame of the reference field skipped last, which its second field joins

    void reset();           // forget all slots and the POC / frame_num history
    void drop_references(); // after a failed slice: nothing is a reference picture any more
    void begin_batch();     // what is a reference picture (or a waiting first field) now is not reused during the batch; no slot holds a picture of the batch yet
    int first_free_slot() const; // the first slot in index order that is neither a reference nor held; -1: none
    int free_slots() const;
    // frame_num values skipped between the previous reference picture and the picture `sh` starts (7.4.3): 0 if none, or an IDR picture
    int missing_frames(const h264mi_sps &sps, const h264mi_slice_header &sh) const;
    // 8.2.5.2: one "non-existing" short-term frame with frame_num `fn`, through the sliding window like a decoded one; false: no free slot
    bool add_nonexisting_frame(const h264mi_sps &sps, int fn);
    // Random access: the stream starts at the non-IDR picture with this frame_num as if nothing had come before -- no reference picture with samples,
    // the history of 8.2.1 zero, PrevRefFrameNum such that the picture is no frame_num gap -- except that the window is filled with non-existing frames
    // for the frame_num values a sliding window held in front of it, so that later lists carry the pictures to come at the indices the encoder meant.
    // (The slots stay held as they are: their samples may still be read.)  false: no free slot
    bool start_at_entry(const h264mi_sps &sps, int frame_num);
    // PicOrderCnt (8.2.1) the picture `sh` starts would get, without touching the history
    int peek_poc(const h264mi_sps &sps, const h264mi_slice_header &sh) const;
    // Random access: a leading picture `sh` starts, which is not decoded.  The counts of 8.2.1 advance as for any picture; a reference picture enters
    // the window as a non-existing frame with its frame_num and its PicOrderCnt (the second field of such a frame joins it) and the sliding window
    // runs.  false: no free slot
    bool skip_picture(const h264mi_sps &sps, const h264mi_slice_header &sh);
    // The picture `sh` starts lives in `slot` (second: it is the second field of the frame waiting there) and is PicDesc `pic` of the batch: the
    // slot is set up and gets the picture's PicOrderCnt (8.2.1).  The picture is under construction until finish_picture.
    void begin_picture(const h264mi_sps &sps, const h264mi_slice_header &sh, int slot, bool second, int pic);
    // 8.2.4: RefPicList0 (P and B slices) and RefPicList1 (B slices) of a slice of the picture under construction, MI_MAX_REFS entries each, -1 beyond
    // the active ones: frame slots, or -- field pictures -- fields written as frame slot | parity << 14 (MI_REF_PARITY)
    int build_ref_lists(const h264mi_sps &sps, const h264mi_slice_header &sh, bool bslice, int16_t *out0, int16_t *out1) const;
    // Entry 0 of the initial P list (8.2.4.2.1 / 8.2.4.2.2 + 8.2.4.2.5) of a picture with this frame_num and structure (0 frame, 1 top field, 2 bottom
    // field) -- the picture under construction, or, with none, the next one --, written like a list entry; -1: the list is empty
    int initial_p_entry0(const h264mi_sps &sps, int frame_num, int field) const;
    // The same for the SECOND field (structure `field`: the parity the frame in pend_slot lacks) of the frame that waits in pend_slot, before that
    // field is under construction: what initial_p_entry0 returns once begin_picture(..., second = true) has run; -1 also when no frame waits
    int second_field_p_entry0(const h264mi_sps &sps, int frame_num, int field);
    // The picture under construction is complete: marking (8.2.5), and the field it adds to its frame -- which then waits in pend_slot for the other one
    void finish_picture(const h264mi_sps &sps);

  private:
    int compute_poc(const h264mi_sps &sps, const h264mi_slice_header &sh);
    bool initial_lists(const h264mi_sps &sps, int frame_num, int field, bool bslice, std::vector<int> &st, std::vector<int> &lt, std::vector<int> lists[2]) const;
    void mark_reference(const h264mi_sps &sps);
    void sliding_window(const h264mi_sps &sps, int frame_num);
    void free_long_term_idx(int idx);
};

bool new_picture(const h264mi_sps &sps, const h264mi_slice_header &a, const h264mi_slice_header &b); // 7.4.1.2.4

} // namespace mi
