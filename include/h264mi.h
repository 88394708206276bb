/*
 * include/h264mi.h -- C ABI of libh264mi.so: MI355X-native H.264 Annex-B decode path.
 *
 * This is the drop-in boundary for the hot path of mrmod/h264decode's Go package `h264`
 * (Annex-B bytes -> NAL -> SPS/PPS/slice header -> macroblocks -> Y/Cb/Cr planes).  The reference
 * has no FFI of its own ("No interface contracts are implemented right now", README.md:4): the
 * boundary is the set of exported Go identifiers; each entry point below names the reference
 * function(s) it replaces.  The cgo / ctypes bindings are shown in INTEGRATION.md.
 *
 * Rules:
 *  - extern "C", plain pointers and sizes only; no C++/torch types.
 *  - every function returns an int32 status (0 = OK, negative = H264MI_E*); nothing aborts or
 *    throws across the boundary (the reference panics/os.Exit()s: h264/server.go:136-143).
 *  - caller owns input buffers for the duration of the call only; the library owns device memory.
 *  - threading: a decoder handle is used by one thread at a time (any thread: every entry point selects the decoder's
 *    HIP device for the duration of the call and restores the caller's); distinct handles are independent.  The error
 *    text of h264mi_last_error_string() is thread-local: fetch it on the thread that received the status (a Go caller
 *    wraps call + fetch in runtime.LockOSThread).
 *  - the pixel path runs ONLY on the GPU (HIP, gfx950).  There is no CPU fallback: without a
 *    usable device h264mi_init / h264mi_decoder_create fail with H264MI_ENODEVICE.
 *
 * Field names follow the reference structs in snake_case (Go: CamelCase): NalUnit
 * h264/nalUnit.go:3-30, SPS h264/sps.go:9-103, PPS h264/pps.go:10-38, SliceHeader
 * h264/slice.go:23-75.  Values are spec-correct where the reference is not.
 */
#ifndef H264MI_H
#define H264MI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H264MI_OK 0
#define H264MI_EINVAL (-1)      /* bad argument */
#define H264MI_EBITSTREAM (-2)  /* malformed / truncated syntax */
#define H264MI_EUNSUPPORTED (-3)/* valid H.264 outside the implemented scope (MBAFF, CABAC-coded field pictures unless asked for, SP/SI slices, data partitioning,
                                 * 4:2:2 / 4:4:4, more than 8 bits ...): the message says what and why.  Of SVC / MVC / 3D-AVC streams the base layer / base view
                                 * is decoded; their extension NAL units (14, 15, 20, 21) are passed over */
#define H264MI_ENODEVICE (-4)   /* no usable HIP device / kernel image */
#define H264MI_ENOMEM (-5)
#define H264MI_EDEVICE (-6)     /* HIP runtime error */
#define H264MI_ECAPACITY (-7)   /* caller buffer or decoder configuration too small */
#define H264MI_EDECODE (-8)     /* a GPU entropy kernel reported a slice error.  With h264mi_config.conceal_errors a failed slice of a concealable picture
                                 * (a non-IDR frame picture -- with H264MI_CONCEAL_FIELDS: or field picture; with H264MI_CONCEAL_IDR: or IDR frame picture -- that has a reference picture) is not an error: it is concealed and counted (h264mi_decoder_concealed) */

/* ---- NAL unit: h264/nalUnit.go:3-30 (NalUnit), :75-131 (NewNalUnit) ---- */
typedef struct {
    int32_t num_bytes;          /* NumBytes: NAL size incl. header */
    int32_t forbidden_zero_bit; /* ForbiddenZeroBit */
    int32_t ref_idc;            /* RefIdc */
    int32_t type;               /* Type */
    int32_t header_bytes;       /* HeaderBytes (1; 4 for types 14/20/21) */
    int32_t svc_extension_flag, avc_3d_extension_flag; /* SvcExtensionFlag, Avc3dExtensionFlag (parsed, Annex G/H/J not decoded) */
    int64_t offset;             /* byte offset of the NAL header inside the scanned buffer */
} h264mi_nal;

/* replaces isStartSequence/readNalUnit (h264/server.go:28-39,64-111): finds every NAL of an
 * Annex-B buffer (3- and 4-byte start codes, trailing zeros stripped).  *n receives the count;
 * returns H264MI_ECAPACITY if more than `cap` NALs exist (first `cap` are still written). */
int32_t h264mi_annexb_scan(const uint8_t *buf, size_t len, h264mi_nal *out, int32_t cap, int32_t *n);
/* replaces NewNalUnit + (*NalUnit).RBSP() (h264/nalUnit.go:72,75-131): parses the header of the
 * NAL at nal_bytes[0..len) and writes the RBSP (emulation prevention removed) to rbsp_out
 * (capacity >= len).  *rbsp_len receives its size. */
int32_t h264mi_nal_parse(const uint8_t *nal_bytes, size_t len, h264mi_nal *nal, uint8_t *rbsp_out, size_t *rbsp_len);

/* ---- SPS: h264/sps.go:9-103, NewSPS :192-437 ---- */
typedef struct {
    int32_t profile, constraint_flags, level, id;                      /* Profile, Constraint0..5 (packed), Level, ID */
    int32_t chroma_format, use_separate_color_plane;                   /* ChromaFormat, UseSeparateColorPlane */
    int32_t bit_depth_luma_minus8, bit_depth_chroma_minus8;            /* BitDepthLumaMinus8, BitDepthChromaMinus8 */
    int32_t qprime_y_zero_transform_bypass, seq_scaling_matrix_present;/* QPrimeYZeroTransformBypass, SeqScalingMatrixPresent */
    int32_t log2_max_frame_num_minus4, pic_order_count_type, log2_max_pic_order_cnt_lsb_min4;
    int32_t delta_pic_order_always_zero, offset_for_non_ref_pic, offset_for_top_to_bottom_field;
    int32_t num_ref_frames_in_pic_order_cnt_cycle;
    int32_t offset_for_ref_frame_list[256];                            /* OffsetForRefFrameList */
    int32_t max_num_ref_frames, gaps_in_frame_num_value_allowed;
    int32_t pic_width_in_mbs_minus1, pic_height_in_map_units_minus1;
    int32_t frame_mbs_only, mb_adaptive_frame_field, direct_8x8_inference;
    int32_t frame_cropping, frame_crop_left_offset, frame_crop_right_offset, frame_crop_top_offset, frame_crop_bottom_offset;
    int32_t vui_parameters_present;
    int32_t aspect_ratio_info_present, aspect_ratio, sar_width, sar_height;
    int32_t overscan_info_present, overscan_appropriate;
    int32_t video_signal_type_present, video_format, video_full_range, color_description_present;
    int32_t color_primaries, transfer_characteristics, matrix_coefficients;
    int32_t chroma_loc_info_present, chroma_sample_loc_type_top_field, chroma_sample_loc_type_bottom_field;
    int32_t timing_info_present;
    uint32_t num_units_in_tick, time_scale;
    int32_t fixed_frame_rate;
    int32_t nal_hrd_parameters_present, vcl_hrd_parameters_present, low_hrd_delay, pic_struct_present;
    int32_t cpb_cnt_minus1, bit_rate_scale, cpb_size_scale;
    int32_t initial_cpb_removal_delay_length_minus1, cpb_removal_delay_length_minus1, dpb_output_delay_length_minus1, time_offset_length;
    int32_t bitstream_restriction, motion_vectors_over_pic_boundaries, max_bytes_per_pic_denom, max_bits_per_mb_denom;
    int32_t log2_max_mv_length_horizontal, log2_max_mv_length_vertical, max_num_reorder_frames, max_dec_frame_buffering;
    /* resolved scaling lists (Table 7-2 fall-back applied), zig-zag order */
    uint8_t scaling_list_4x4[6][16];
    uint8_t scaling_list_8x8[2][64];
    /* derived (h264/slice.go:159-176 PicWidthInMbs ... PicSizeInMbs) */
    int32_t pic_width_in_mbs, pic_height_in_mbs, width, height;       /* width/height = cropped display size */
} h264mi_sps;
/* replaces NewSPS(rbsp, showPacket) (h264/sps.go:192) */
int32_t h264mi_sps_parse(const uint8_t *rbsp, size_t len, h264mi_sps *sps);

/* ---- PPS: h264/pps.go:10-38, NewPPS :40-133 ---- */
typedef struct {
    int32_t id, sps_id, entropy_coding_mode, bottom_field_pic_order_in_frame_present, num_slice_groups_minus1;
    int32_t num_ref_idx_l0_default_active_minus1, num_ref_idx_l1_default_active_minus1;
    int32_t weighted_pred, weighted_bipred, pic_init_qp_minus26, pic_init_qs_minus26, chroma_qp_index_offset;
    int32_t deblocking_filter_control_present, constrained_intra_pred, redundant_pic_cnt_present;
    int32_t transform_8x8_mode, pic_scaling_matrix_present, second_chroma_qp_index_offset;
    uint8_t scaling_list_4x4[6][16];
    uint8_t scaling_list_8x8[2][64];
    /* slice groups (num_slice_groups_minus1 > 0; h264/pps.go:16-23, :57-80).  slice_group_id[] of map type 6 is one entry
     * per map unit and does not live in this struct: h264mi_pps_slice_group_ids() */
    int32_t slice_group_map_type, run_length_minus1[8], top_left[8], bottom_right[8];
    int32_t slice_group_change_direction, slice_group_change_rate_minus1, pic_size_in_map_units_minus1;
} h264mi_pps;
/* replaces NewPPS(sps, rbsp, showPacket) (h264/pps.go:40).  `sps` is the SPS the PPS refers to
 * (the reference passes "the last SPS": h264/server.go:155). */
int32_t h264mi_pps_parse(const h264mi_sps *sps, const uint8_t *rbsp, size_t len, h264mi_pps *pps);
/* PPS.SliceGroupId (h264/pps.go:23, :72-78): slice_group_id[i] of a PPS with slice_group_map_type 6, one byte per map unit.
 * *n receives pic_size_in_map_units_minus1 + 1 (0 for any other PPS); at most cap entries are written. */
int32_t h264mi_pps_slice_group_ids(const h264mi_sps *sps, const uint8_t *rbsp, size_t len, uint8_t *ids, size_t cap, size_t *n);

/* ---- slice header: h264/slice.go:23-75, NewSliceContext :835-1048 ---- */
typedef struct {
    int32_t first_mb_in_slice, slice_type, pps_id, color_plane_id, frame_num;
    int32_t field_pic, bottom_field, idr_pic_id, pic_order_cnt_lsb, delta_pic_order_cnt_bottom;
    int32_t delta_pic_order_cnt[2], redundant_pic_cnt, direct_spatial_mv_pred;
    int32_t num_ref_idx_active_override, num_ref_idx_l0_active_minus1, num_ref_idx_l1_active_minus1;
    int32_t ref_pic_list_modification_flag_l0, n_ref_pic_list_modifications;
    int32_t modification_of_pic_nums[66], modification_value[66]; /* idc / abs_diff_pic_num_minus1 | long_term_pic_num */
    int32_t luma_log2_weight_denom, chroma_log2_weight_denom;
    int32_t luma_weight_l0_flag[32], luma_weight_l0[32], luma_offset_l0[32];
    int32_t chroma_weight_l0_flag[32], chroma_weight_l0[32][2], chroma_offset_l0[32][2];
    /* list 1 of B slices (7.3.3.1, 7.3.3.2) */
    int32_t ref_pic_list_modification_flag_l1, n_ref_pic_list_modifications_l1;
    int32_t modification_of_pic_nums_l1[66], modification_value_l1[66];
    int32_t luma_weight_l1_flag[32], luma_weight_l1[32], luma_offset_l1[32];
    int32_t chroma_weight_l1_flag[32], chroma_weight_l1[32][2], chroma_offset_l1[32][2];
    int32_t no_output_of_prior_pics_flag, long_term_reference_flag, adaptive_ref_pic_marking_mode_flag;
    int32_t n_memory_management_control_operations;
    int32_t memory_management_control_operation[66], mmco_arg1[66], mmco_arg2[66];
    int32_t cabac_init, slice_qp_delta, sp_for_switch, slice_qs_delta;
    int32_t disable_deblocking_filter, slice_alpha_c0_offset_div2, slice_beta_offset_div2;
    int32_t slice_group_change_cycle; /* slice group map types 3..5 (h264/slice.go:1028-1031) */
    /* derived */
    int32_t nal_ref_idc, nal_unit_type, slice_qp_y; /* SliceQPy (h264/cabac.go:113) */
    int64_t slice_data_bit_offset;                  /* where slice_data() starts inside the RBSP */
} h264mi_slice_header;
/* replaces NewSliceContext's header part (h264/slice.go:857-1032) */
int32_t h264mi_slice_header_parse(const h264mi_sps *sps, const h264mi_pps *pps, int32_t nal_ref_idc, int32_t nal_unit_type,
                                  const uint8_t *rbsp, size_t len, h264mi_slice_header *sh);

/* First slice of a new picture?  7.4.1.2.4 on two slice headers of one stream (`prev`: the first slice of the current picture), plus what
 * 7.4.3 makes constant over the slices of a picture (slice_group_change_cycle, the marking script) -- memory management operation 5
 * resets frame_num and the picture order count, so the headers of the next picture may agree with it in everything 7.4.1.2.4 lists.
 * Returns 1 / 0 (negative: H264MI_EINVAL).  What h264mi_batch_prepare applies itself; exported for front-ends that cut a byte stream
 * into access units (the reference reads NAL by NAL and never needs it: h264/server.go:113-166). */
int32_t h264mi_slice_starts_picture(const h264mi_sps *sps, const h264mi_slice_header *prev, const h264mi_slice_header *cur);

/* ---- slice groups (FMO, 8.2.2): h264/slice.go:134-158, :457-552 ----
 * MapUnitToSliceGroupMap(sps, pps, header) (h264/slice.go:457): map types 0..6 (the reference stops at 2).  ids / n_ids: the
 * slice_group_id array of a type-6 PPS (NULL / 0 otherwise); slice_group_change_cycle: the slice header's field (types 3..5).
 * *n receives PicSizeInMapUnits; H264MI_ECAPACITY if cap is smaller. */
int32_t h264mi_map_unit_to_slice_group_map(const h264mi_sps *sps, const h264mi_pps *pps, const uint8_t *ids, size_t n_ids,
                                           int32_t slice_group_change_cycle, uint8_t *map, size_t cap, size_t *n);
/* MbToSliceGroupMap(sps, pps, header) (h264/slice.go:134): 8.2.2.8, one entry per macroblock of the picture. */
int32_t h264mi_mb_to_slice_group_map(const h264mi_sps *sps, const h264mi_pps *pps, const uint8_t *ids, size_t n_ids,
                                     int32_t slice_group_change_cycle, int32_t field_pic, uint8_t *map, size_t cap, size_t *n);
/* nextMbAddress(n, ...) (h264/slice.go:530): the next macroblock of n's slice group in `map`, n_mbs if there is none. */
int32_t h264mi_next_mb_address(const uint8_t *map, size_t n_mbs, size_t n);

/* ---- GPU decode: replaces NewSliceData / MbPred and the absent L7 reconstruction
 *      (h264/slice.go:570-830, :252-454; README.md:8-10 TODO items) ---- */
typedef struct h264mi_decoder h264mi_decoder;

typedef struct {
    /* sizeof(h264mi_config) as the CALLER was compiled: the struct grows at its end from version to version, and a field that lies beyond
     * struct_size is taken as 0 (its default) instead of being read from whatever follows a shorter struct.  0 is refused: zero-initialise
     * the struct and set this field (H264MI_CONFIG_INIT).  Adding this field in front was a ONE-TIME ABI break (round 4): binaries built against
     * the header without it do not work with this library; size-based compatibility starts with this version of the struct. */
    uint32_t struct_size;
    int32_t device;                /* HIP device ordinal */
    int32_t max_streams;           /* independent streams decoded side by side */
    int32_t max_width, max_height; /* display size upper bound (coded size is rounded up to 16) */
    int32_t max_frames_per_batch;  /* PICTURES per stream and per h264mi_decode_batch call: a frame picture is one, a frame coded as two field
                                    * pictures (h264/slice.go:867-872 field_pic_flag) is two */
    int32_t max_slices_per_frame;
    int64_t max_bitstream_bytes;   /* per batch, summed over streams */
    void *hip_stream;              /* hipStream_t to launch on; NULL = a private stream */
    /* Sizing knobs, 0 = default.  max_ref_frames: the largest max_num_ref_frames (h264/sps.go:61) the streams will carry; the frame
     * pool holds that many reference slots per stream (default 16, the limit of any level; a 1080p slot is 3.1 MB per stream) and
     * a stream that declares more is refused with H264MI_ECAPACITY.  coef_blocks_per_mb: residual pool size in 32-byte blocks per
     * macroblock (default 8 of at most 26; see h264mi_decoder_coef_pool). */
    int32_t max_ref_frames, coef_blocks_per_mb;
    /* b_pictures: 0 = what only B pictures need (list-1 vectors, the motion of reference pictures kept for direct prediction: 16 GB for 256
     * streams of 1080p) is allocated when the first B slice arrives -- I / P deployments never pay for it, and the FIRST B picture a decoder
     * sees must find its co-located picture in the same batch or the one before (otherwise that stream is refused until its next IDR picture);
     * 1 = allocated at create time, motion kept from the first picture on. */
    int32_t b_pictures;
    /* allow_unpinned_field_cabac: 1 = field pictures (h264/slice.go:867-872 field_pic_flag) coded with CABAC are decoded.  The default is a refusal
     * (H264MI_EUNSUPPORTED): the initialisation values of the contexts only field-coded blocks use (ctxIdx 277-398, 436-459; four sets) were entered
     * into this library's tables without the standard at hand and nothing pins them -- no third-party field-coded stream, no reference table on the
     * build machine.  With a wrong value a slice loses synchronisation and does not end on end_of_slice_flag at the picture's last macroblock: such
     * slices fail (H264MI_EDECODE, the stream waits for its next IDR picture) and are counted: h264mi_decoder_unpinned_failures. */
    int32_t allow_unpinned_field_cabac;
    /* conceal_errors: 0 (default) = a slice that fails in the entropy kernel takes its stream out until the next IDR picture, and macroblocks no slice
     * delivered are mid-grey.  1 = error concealment: in a frame picture that is not an IDR picture and for which the initial P reference list
     * (8.2.4.2.1) is not empty, the LOST macroblocks -- the ones no slice delivered, and ALL macroblocks of a slice the entropy kernel failed on -- are
     * reconstructed as a zero-motion copy of entry 0 of that list; the result is bit for bit what a conforming decoder produces for the stream in
     * which those macroblocks are coded as P slices of P_Skip macroblocks (one active reference, slice_qp_delta 0, deblocking on, default weights).
     * The picture is kept and used as a reference, the stream's status stays H264MI_OK, nothing waits for an IDR picture.  The repair happens on the
     * device inside the pass, so pipelined callers get it for the batch prepared before the failure was known as well.  A slice NAL unit of
     * type 1 whose header does not parse is dropped and counted as a lost slice of the non-IDR picture under construction (of the next picture, if there is
     * none or it is an IDR picture) when that picture is concealable; otherwise it fails the stream as with 0.
     * The field is a bit set; 0 and 1 mean what they always meant.  H264MI_CONCEAL_PICTURES (2, together with bit 1: value 3) = wholly lost REFERENCE FRAMES
     * are concealed too.  They show as a gap in frame_num (the first slice of a picture that is not an IDR picture and not the second field of the frame
     * before it, in a stream with gaps_in_frame_num_value_allowed_flag 0, carries a frame_num that is neither PrevRefFrameNum nor its successor):
     * m = (frame_num - PrevRefFrameNum - 1) mod MaxFrameNum frames are missing.  If m <= H264MI_CONCEAL_MAX_GAP, entry 0 of the initial P list (8.2.4.2.1)
     * of a frame with the first missing frame_num exists and holds samples, and the m pictures plus the revealing one fit into what the batch has left
     * (max_frames_per_batch -- leave H264MI_CONCEAL_MAX_GAP of headroom --, frame slots, macroblock records), the decoder inserts one frame picture per
     * missing value, in increasing frame_num order, in front of the revealing picture; otherwise everything is as with the bit clear ("reference pictures
     * are missing", the stream waits for its IDR picture).  The result is bit for bit what a conforming decoder produces for the stream in which each
     * missing frame is coded as: nal_unit_type 1, nal_ref_idc 1; one P slice of P_Skip macroblocks per slice group (first_mb_in_slice the lowest address
     * of the group); pic_parameter_set_id and slice_group_change_cycle of the first slice seen of the revealing picture; the missing frame_num;
     * field_pic_flag 0; pic_order_cnt_lsb = (prevPicOrderCntLsb + 2) mod MaxPicOrderCntLsb (8.2.1.1, inserted pictures included) and
     * delta_pic_order_cnt_bottom 0 / delta_pic_order_cnt[0] = [1] = 0 / nothing for picture order count types 0 / 1 / 2; redundant_pic_cnt 0; one active
     * reference, no list modification, a pred_weight_table() with all flags 0, sliding-window marking, cabac_init_idc 0, slice_qp_delta 0,
     * disable_deblocking_filter_idc 0 with zero offsets.  Every boundary strength of such a picture is 0, so an inserted picture is an exact copy of
     * entry 0 of its initial P list.  It is output in decoding order like any frame (h264mi_frame_get_info: its frame_num and PicOrderCnt, nal_ref_idc 1,
     * idr 0), stays a reference and goes through the sliding window, updates PrevRefFrameNum and the picture order count state, and
     * h264mi_frame_concealed reports all of its macroblocks (h264mi_decoder_concealed_pictures counts it).
     * As with 0, whatever the bits: a lost NON-reference picture leaves no gap and is not noticed; pictures lost in front of an IDR picture are not
     * inserted; a gap of a multiple of MaxFrameNum pictures is invisible; what the lost pictures carried is lost (a memory management operation, a
     * long-term assignment, operation 5), and a later slice that depends on it fails as it always did ("ref_pic_list_modification names a missing
     * picture", ...); in streams with B pictures the chosen PicOrderCnt can equal that of a B picture nearby, and the outcome is whatever the repaired
     * stream decodes to.
     * H264MI_CONCEAL_FIELDS (4, together with bit 1) = the rule of value 1 holds for FIELD pictures too: a field picture that is not an IDR picture and
     * whose initial P list for fields (8.2.4.2.5, built for this field: it includes the first field of the same frame when that is a reference) is not
     * empty and has an entry 0 that holds samples.  The lost macroblocks are a zero-motion copy of that entry 0 -- for the second field of an IDR frame
     * the frame's own first field --; in the repaired stream the replacement P slices carry field_pic_flag 1 and the picture's bottom_field_flag, and
     * delta_pic_order_cnt_bottom / delta_pic_order_cnt[1] are absent (7.3.3).  The tolerance for type-1 slices whose header does not parse extends to
     * such pictures.  CABAC field pictures still need allow_unpinned_field_cabac, and h264mi_decoder_unpinned_failures counts their failed slices
     * whether they are concealed or not.
     * H264MI_CONCEAL_IDR (16, together with bit 1) = lost and damaged slices of IDR FRAME pictures are concealed too.  An IDR picture X (all its slices
     * nal_unit_type 5, field_pic_flag 0) is concealable when the SPS active for X gives the same picture size in macroblocks, chroma_format_idc,
     * frame_mbs_only_flag and log2_max_frame_num_minus4 as the one the stream's reference frames were decoded under (a re-sent identical SPS is fine),
     * and the initial P list (8.2.4.2.1) -- built when X's first slice arrives, BEFORE X's marking drops the references, for a frame picture with
     * frame_num F' = (PrevRefFrameNum + 1) mod MaxFrameNum -- is not empty and its entry 0 holds samples.  That entry is X's concealment reference.  So
     * the first picture of a stream, and an IDR picture after a reset or after an error that dropped the references, are not concealable; what is not
     * concealable behaves exactly as with the bit clear.  The lost macroblocks of a concealable X (same definition as for bit 1) come out bit for bit
     * as a conforming decoder reconstructs X in the stream in which: every slice NAL unit of X has nal_unit_type 1 with nal_ref_idc unchanged; every
     * slice header of X carries frame_num F', no idr_pic_id, and a dec_ref_pic_marking() of adaptive_ref_pic_marking_mode_flag 1 with memory management
     * operation 5 and the end code 0 (operation 5 takes effect after the picture is decoded: X predicts from the old references and leaves behind
     * exactly the state an IDR picture leaves); the intact I slices keep every other header field and their slice data (slice_type 7 is written as 2:
     * the picture holds P slices now); each lost slice is a P slice of P_Skip macroblocks over the same macroblocks, written as for bit 1 (one active
     * reference, no list modification, an all-zero pred_weight_table() where the PPS asks for one, slice_qp_delta 0, disable_deblocking_filter_idc 0 with
     * zero offsets, cabac_init_idc 0) with the same rewritten frame_num and marking.  The rule defines X's samples only: what is REPORTED for X stays an
     * IDR picture's (h264mi_frame_get_info: idr 1, its own frame_num and PicOrderCnt), its marking is the real IDR marking, and later pictures predict
     * from the concealed X as from any picture.  (A later B picture that uses TEMPORAL direct prediction with a concealed macroblock of X as co-located
     * block refers to a picture that is no longer a reference: the outcome is whatever the repaired stream decodes to.)  A slice NAL unit of type 5 whose
     * header does not parse is counted as a lost slice of the IDR picture under construction -- of the next picture, if there is none or it is not an IDR
     * picture -- and tolerated only if that picture turns out to be a concealable IDR picture; a dropped unit whose type does not match the picture it
     * falls to fails the stream as with 0.  Cost: with the bit set a concealable IDR picture is reconstructed behind its concealment reference when one
     * batch decodes both, damaged or not (the device learns about damage only after the entropy launch), so a batch that holds several GOPs of one
     * stream loses the overlap between them; a reference decoded by an earlier batch costs nothing.
     * H264MI_CONCEAL_LONE_FIELDS (64, together with bits 1 and 4) = a wholly lost FIELD of a frame coded as two field pictures is concealed too.  A first
     * field F is lone when what the decoder meets next for the stream is not its second field: another picture (one that is not a non-IDR field of the
     * opposite parity with F's frame_num and the same zero-ness of nal_ref_idc), an end-of-sequence or end-of-stream NAL unit, or a change of the active
     * sequence.  At that point, in front of the revealing picture, the decoder inserts the field picture F': opposite parity, F's frame_num, reference
     * or not like F, no slices.  The result is bit for bit what a conforming decoder produces for the stream in which F' is coded as: nal_unit_type 1,
     * nal_ref_idc equal to F's; one P slice of P_Skip macroblocks per slice group (first_mb_in_slice the lowest address of the group); F's
     * pic_parameter_set_id and slice_group_change_cycle; F's frame_num; field_pic_flag 1 and bottom_field_flag the opposite of F's; pic_order_cnt_lsb =
     * (F's + 1) mod MaxPicOrderCntLsb / delta_pic_order_cnt[0] = 0 / nothing for picture order count types 0 / 1 / 2 (delta_pic_order_cnt_bottom and
     * delta_pic_order_cnt[1] are absent in a field, 7.3.3); one active reference (num_ref_idx_active_override_flag 1), no list modification, a
     * pred_weight_table() with all flags 0 where the PPS asks for one, adaptive_ref_pic_marking_mode_flag 0 if F' is a reference, cabac_init_idc 0,
     * slice_qp_delta 0, disable_deblocking_filter_idc 0 with zero offsets.  So F' is a zero-motion copy of entry 0 of the initial P list for fields
     * (8.2.4.2.5) built for F', used exactly as H264MI_CONCEAL_FIELDS uses it -- the field of F''s own parity of the first reference frame in FrameNumWrap
     * order that has one; F itself when there is none, as in the IDR frame (a zero luma vector into a field of the other parity is a chroma vector of
     * a quarter sample, 8.4.1.4) --, nothing of it is filtered, h264mi_frame_concealed reports its macroblocks with its frame and
     * h264mi_decoder_concealed_fields counts it.  A lost FIRST
     * field needs no rule of its own: the surviving second field is taken for a first field, as it always was, and gets its complement by the rule above
     * (the survivor's reference lists lack the lost field: the outcome is whatever the repaired stream decodes to).  F' is NOT inserted, and everything is
     * as with the bit clear (the rows mid-grey, no error), when entry 0 does not exist or holds no samples; when the SPS or PPS F was decoded under has
     * been replaced by other content since; when allow_unpinned_field_cabac is off for a CABAC stream; or when F' and the revealing picture do not fit into
     * what the batch has left (max_frames_per_batch, macroblock records, staging room for a slice group map).  A field always counted as a picture against
     * max_frames_per_batch: a caller who sized it for two pictures per frame needs NO extra headroom for this bit.  A lone field at the very end of
     * input, with nothing behind it, waits for its second field as it always did.
     * With every value: IDR FIELD pictures whose own slices are lost, wholly lost IDR pictures, a wholly missing field without H264MI_CONCEAL_LONE_FIELDS
     * (its rows stay mid-grey), MBAFF (out of scope altogether), pictures without any reference picture and parameter-set errors are handled as with 0; so
     * are IDR frame pictures without H264MI_CONCEAL_IDR.  The legal values are 0, 1, 3, 5, 7, 17, 19, 21 and 23, and with H264MI_CONCEAL_LONE_FIELDS 69, 71,
     * 85 and 87: any other (bit 2, 4 or 16 without bit 1; bit 64 without bits 1 and 4; bits 8 and 32, which are unassigned; anything above 87) is refused
     * by h264mi_decoder_create (H264MI_EINVAL). */
    int32_t conceal_errors;
} h264mi_config;
#define H264MI_CONCEAL_SLICES 1    /* h264mi_config.conceal_errors: lost and damaged slices of non-IDR frame pictures */
#define H264MI_CONCEAL_PICTURES 2  /* ... and wholly lost reference frames (only together with H264MI_CONCEAL_SLICES) */
#define H264MI_CONCEAL_FIELDS 4    /* ... and lost and damaged slices of field pictures (only together with H264MI_CONCEAL_SLICES) */
#define H264MI_CONCEAL_IDR 16      /* ... and lost and damaged slices of IDR frame pictures that still have a reference frame (only together with H264MI_CONCEAL_SLICES) */
#define H264MI_CONCEAL_LONE_FIELDS 64 /* ... and the wholly lost field of a frame coded as two field pictures (only together with H264MI_CONCEAL_SLICES and H264MI_CONCEAL_FIELDS) */
#define H264MI_CONCEAL_MAX_GAP 16  /* the longest run of lost frames that is concealed: the largest DPB -- older frames would have left the sliding window anyway */
#define H264MI_CONFIG_INIT {(uint32_t)sizeof(h264mi_config)} /* h264mi_config cfg = H264MI_CONFIG_INIT; then set the fields */

typedef struct {
    int32_t n_frames;         /* frames decoded in this batch */
    int32_t n_slices;
    int64_t n_macroblocks;
    int64_t bitstream_bytes;  /* RBSP bytes resident on the device */
    int32_t width, height, coded_width, coded_height; /* of stream 0 */
    double host_prepare_ms;   /* NAL scan + header parse + DPB bookkeeping + upload enqueue */
} h264mi_batch_info;

int32_t h264mi_init(int32_t device);
int32_t h264mi_decoder_create(const h264mi_config *cfg, h264mi_decoder **out);
int32_t h264mi_decoder_destroy(h264mi_decoder *dec);
int32_t h264mi_decoder_set_stream(h264mi_decoder *dec, void *hip_stream);
/* Forget all reference pictures of every stream (seek / new sequence). */
int32_t h264mi_decoder_reset(h264mi_decoder *dec);
/* Forget everything about ONE stream slot -- parameter sets, reference pictures, POC / frame_num history -- before the
 * slot is given to a new connection (the reference starts every connection from scratch: h264/server.go:113-125). */
int32_t h264mi_stream_reset(h264mi_decoder *dec, int32_t stream);
/* Error isolation for batches of unrelated streams (one connection each).  Off (default): the first stream error fails
 * h264mi_batch_prepare / h264mi_batch_sync.  On: a stream whose chunk cannot be parsed, or whose slices fail in the
 * entropy kernel, is dropped from the batch and marked; the calls return H264MI_OK and the other streams decode
 * normally.  A marked stream resumes at its next IDR picture (with H264MI_RA_RECOVERY_POINT: at its next entry point, see "Random access").  (With h264mi_config.conceal_errors a failed slice of a concealable picture
 * marks nothing: only what cannot be concealed takes a stream out.) */
int32_t h264mi_decoder_set_isolation(h264mi_decoder *dec, int32_t on);
/* Status of a stream in the current batch: H264MI_OK or the H264MI_E* that took it out (valid after prepare; entropy
 * kernel failures appear after sync).  Pipelined callers (execute(k); prepare(k + 1); execute(k + 1); ... one sync for
 * several batches): h264mi_batch_sync looks at every batch executed since the last sync, and h264mi_batch_prepare at the
 * batch whose staging set it takes back, so a failure in batch k marks its stream (references dropped, nothing decoded
 * before its next IDR picture) before batch k + 2 is parsed at the latest; batch k + 1 of that stream, prepared before the
 * failure was known, is decoded from the damaged pictures.  The status VALUE is reset by every prepare: read it after
 * the sync that follows an execute if it matters.  With h264mi_config.conceal_errors failed slices of concealable pictures leave the
 * status at H264MI_OK (batch k + 1 is then decoded from the concealed pictures, which is what a decoder of the repaired stream does). */
int32_t h264mi_stream_status(h264mi_decoder *dec, int32_t stream, int32_t *status);

/* Stage 1 (host + H2D): scan and parse each stream's Annex-B chunk (whole access units), run
 * picture management (POC 8.2.1, reference lists 8.2.4, marking 8.2.5), and make the RBSP bytes
 * and slice/picture descriptors resident in device memory.  bufs[i]/lens[i] = chunk of stream i
 * (NULL/0 = nothing for that stream). */
int32_t h264mi_batch_prepare(h264mi_decoder *dec, int32_t n_streams, const uint8_t *const *bufs, const size_t *lens, h264mi_batch_info *info);
/* Stage 2 (GPU only): entropy-decode every slice of the prepared batch (one slice per wavefront),
 * then reconstruct and deblock picture by picture.  Asynchronous on the decoder's stream.  May be
 * called repeatedly for the same prepared batch (benchmarks); results are identical each time. */
int32_t h264mi_batch_execute(h264mi_decoder *dec);
/* Wait for the stream and collect per-slice status written by the entropy kernels. */
int32_t h264mi_batch_sync(h264mi_decoder *dec);
/* prepare + execute + sync */
int32_t h264mi_decode_batch(h264mi_decoder *dec, int32_t n_streams, const uint8_t *const *bufs, const size_t *lens, h264mi_batch_info *info);

/* Frames of the last batch, in decoding order (== output order unless the stream has B pictures: h264mi_stream_output_order).  A frame coded as two
 * field pictures (h264/slice.go:867-872) is ONE frame here: it is reported with the batch that holds its second field -- the first field's batch
 * reports nothing for it --, or, if the second field never comes, with the batch in which something else follows it (another picture, an
 * end-of-sequence / end-of-stream NAL unit), the rows of the missing field mid-grey (with H264MI_CONCEAL_LONE_FIELDS: concealed). */
int32_t h264mi_stream_frame_count(h264mi_decoder *dec, int32_t stream, int32_t *n);
/* Device pointers + pitches of a decoded frame (coded size; planes are resident in HBM until the
 * next h264mi_batch_prepare). */
int32_t h264mi_frame_device_planes(h264mi_decoder *dec, int32_t stream, int32_t frame, void **y, void **cb, void **cr, int32_t *pitch_y,
                                   int32_t *pitch_c, int32_t *coded_width, int32_t *coded_height);
/* Geometry and picture-order data of a decoded frame (the picture's own SPS: a batch may span a resolution change). */
typedef struct {
    int32_t width, height, coded_width, coded_height, crop_x, crop_y; /* display size, coded size, crop origin (luma samples) */
    int32_t pic_order_cnt;                                            /* PicOrderCnt(CurrPic) 8.2.1, after a possible MMCO 5 */
    int32_t frame_num, nal_ref_idc, idr;
    int32_t new_sequence; /* picture order counts start over here: IDR picture, or memory_management_control_operation 5 */
} h264mi_frame_info;
int32_t h264mi_frame_get_info(h264mi_decoder *dec, int32_t stream, int32_t frame, h264mi_frame_info *info);
/* Output (display) order of the frames of the last batch of one stream: order[k] = index (decoding order) of the k-th frame
 * to show -- ascending PicOrderCnt inside each coded video sequence (a new one starts at an IDR picture or at a picture
 * with memory_management_control_operation 5).  The batch is ordered on its own: a caller that cuts batches in the middle
 * of a group of B pictures merges the tail of one batch with the head of the next by pic_order_cnt.  (The reference has no
 * output process at all: h264/server.go:113-166 stops at the parsed slice.) */
int32_t h264mi_stream_output_order(h264mi_decoder *dec, int32_t stream, int32_t *order, int32_t cap, int32_t *n);
/* Tight I420 layout of a w x h frame, the one every output call below writes: w * h luma bytes, then the Cb and the Cr plane of
 * ceil(w / 2) x ceil(h / 2) bytes each -- w * h * 3 / 2 for even sizes.  The display size is odd only for monochrome streams (crop
 * units of one luma sample, 7.4.2.1.1); a chroma plane then starts at (crop_x / 2, crop_y / 2) of the coded plane like any other. */
#define H264MI_I420_SIZE(w, h) ((size_t)(w) * (size_t)(h) + 2 * (((size_t)(w) + 1) / 2) * (((size_t)(h) + 1) / 2))
/* Copy a frame to host memory as tight I420 (crop != 0: display size, else coded size); cap >= H264MI_I420_SIZE of that size. */
int32_t h264mi_frame_read(h264mi_decoder *dec, int32_t stream, int32_t frame, int32_t crop, uint8_t *dst, size_t cap);
/* Cropped, tightly packed I420 copy on the device (K6): dst is a DEVICE pointer. */
int32_t h264mi_frame_pack_device(h264mi_decoder *dec, int32_t stream, int32_t frame, void *dst_device, size_t cap);
/* The same for every frame of the last executed batch in ONE launch: frames of stream `stream` (or of all streams when
 * stream = -1, stream-major) in decoding order, back to back.  *bytes receives the total size (also on H264MI_ECAPACITY). */
int32_t h264mi_batch_pack_device(h264mi_decoder *dec, int32_t stream, void *dst_device, size_t cap, size_t *bytes);

/* ---- Output formats (K7): NV12 and RGB on the device.  The reference has no output process (h264/server.go:113-166 stops at the parsed slice) ----
 * A converted frame is a function of the tight I420 frame h264mi_frame_read(crop = 1) returns, and of nothing else: Y[h][w], Cb[hc][wc], Cr[hc][wc] with
 * wc = ceil(w / 2), hc = ceil(h / 2) (chroma from (crop_x / 2, crop_y / 2) of the coded plane, as K6 takes it; 128 in monochrome streams, so RGB comes
 * out grey and the NV12 chroma plane is 128).  Everything below is integer arithmetic; this comment is the contract.
 *   H264MI_FMT_NV12   w * h luma bytes, then hc rows of wc (Cb, Cr) byte pairs                  H264MI_I420_SIZE(w, h) bytes
 *   H264MI_FMT_RGB24  h x w x 3 bytes R, G, B, tight                                           3 * w * h bytes
 *   H264MI_FMT_RGBP   three tight h x w planes R, G, B (torch's CHW)                            3 * w * h bytes
 * Any other format is H264MI_EINVAL (H264MI_FMT_I420 is what the pack calls above write; of the calls of this section only h264mi_output_size accepts it, the scale calls below do too).
 * csc, a small bit set: the matrix in the low four bits (H264MI_CSC_AUTO, _BT601, _BT709), H264MI_CSC_FULL_RANGE (only with an explicit matrix: with AUTO
 * the range comes from the stream), H264MI_CSC_CHROMA_BILINEAR (default: nearest).  For NV12 csc must be 0 -- nothing is converted.  Anything else is
 * H264MI_EINVAL.
 * AUTO is resolved per frame from the SPS that frame was decoded under: video_full_range_flag is the range (0 when the VUI or video_signal_type is absent,
 * E.2.1); matrix_coefficients (2, "unspecified", when absent) 1 gives BT.709, 5 and 6 give BT.601, 2 gives BT.709 when the display width is >= 1280 or the
 * display height is > 576 and BT.601 otherwise; every other value (0 GBR, 4, 7, 8 YCgCo, 9 ...) is H264MI_EUNSUPPORTED, and the message names the value and
 * says that an explicit matrix can be passed.  An explicit matrix never looks at the stream.
 * Coefficients: with (Kr, Kb) = (0.299, 0.114) for BT.601 and (0.2126, 0.0722) for BT.709, Kg = 1 - Kr - Kb, sy = 255 / 219 and sc = 255 / 224 for limited
 * range (both 1 for full range):  cy = round(8192 sy), crv = round(8192 * 2 (1 - Kr) sc), cgu = round(8192 * 2 Kb (1 - Kb) / Kg * sc),
 * cgv = round(8192 * 2 Kr (1 - Kr) / Kg * sc), cbu = round(8192 * 2 (1 - Kb) sc) -- the four sets are H264MI_CSC_COEFFS below.
 * Arithmetic: y' = Y - 16 for limited range, Y for full range; u = cb - 128, v = cr - 128 with cb, cr the upsampled 8-bit chroma samples of the pixel;
 * 32-bit integers, >> is an arithmetic shift (floor), clip is to 0 .. 255:
 *   R = clip((cy y' + crv v + 4096) >> 13)    G = clip((cy y' - cgu u - cgv v + 4096) >> 13)    B = clip((cy y' + cbu u + 4096) >> 13)
 * Chroma of luma position (x, y), k = x >> 1, j = y >> 1.  Nearest: cb = Cb[j][k].  Bilinear: the 4:2:0 siting of chroma_sample_loc_type 0 (co-sited with
 * even luma columns, midway between luma rows 2j and 2j + 1): Hrow(r) = 2 C[r][k] for even x, C[r][k] + C[r][min(k + 1, wc - 1)] for odd x;
 * j' = max(j - 1, 0) for even y, min(j + 1, hc - 1) for odd y; c = (3 Hrow(j) + Hrow(j') + 4) >> 3 (weights sum to 8, one rounding).  The clamps are at the
 * edges of the DISPLAY chroma plane: coded samples outside the crop rectangle are never read.  The rule is applied to frames as they are, whether they
 * were coded as frame or field pictures (deinterlace first where that matters: "Deinterlaced output" below); interlace-aware upsampling inside this
 * rule, and chroma_sample_loc_type other than 0, are out of scope. */
#define H264MI_FMT_I420 0
#define H264MI_FMT_NV12 1
#define H264MI_FMT_RGB24 2
#define H264MI_FMT_RGBP 3
#define H264MI_CSC_AUTO 0
#define H264MI_CSC_BT601 1
#define H264MI_CSC_BT709 2
#define H264MI_CSC_FULL_RANGE 16
#define H264MI_CSC_CHROMA_BILINEAR 32
/* {cy, crv, cgu, cgv, cbu}: BT.601 limited, BT.601 full, BT.709 limited, BT.709 full */
#define H264MI_CSC_COEFFS { \
    {9539, 13075, 3209, 6660, 16525}, \
    {8192, 11485, 2819, 5850, 14516}, \
    {9539, 14686, 1747, 4366, 17305}, \
    {8192, 12901, 1535, 3835, 15201}}
/* Bytes of a w x h frame in `format` (H264MI_FMT_I420 too).  Pure: no decoder, no device. */
int32_t h264mi_output_size(int32_t format, int32_t w, int32_t h, size_t *bytes);
/* The AUTO rule above as a pure function: *resolved = the matrix (H264MI_CSC_BT601 / _BT709) | H264MI_CSC_FULL_RANGE or 0 | the chroma bit of csc, for a
 * frame of width x height display samples whose SPS carries matrix_coefficients (2 when absent) and video_full_range (0 when absent).  H264MI_EINVAL for a
 * csc that is not legal, H264MI_EUNSUPPORTED for AUTO over a matrix_coefficients value outside 1, 2, 5, 6. */
int32_t h264mi_csc_resolve(int32_t csc, int32_t matrix_coefficients, int32_t video_full_range, int32_t width, int32_t height, int32_t *resolved);
/* matrix_coefficients and video_full_range_flag a frame of the last batch was coded under (its own SPS: a batch may span a change of them); 2 and 0
 * where the SPS does not carry them.  What AUTO resolves from. */
int32_t h264mi_frame_colour(h264mi_decoder *dec, int32_t stream, int32_t frame, int32_t *matrix_coefficients, int32_t *video_full_range);
/* One frame of the last executed batch, cropped and converted on the device (K7) into the DEVICE buffer dst_device; cap >= h264mi_output_size of its
 * display size.  Asynchronous on the decoder's stream, like h264mi_frame_pack_device. */
int32_t h264mi_frame_convert_device(h264mi_decoder *dec, int32_t stream, int32_t frame, int32_t format, int32_t csc, void *dst_device, size_t cap);
/* The same for every frame of the last executed batch in ONE launch -- h264mi_batch_pack_device's contract: frames of stream `stream` (or of all streams
 * when stream = -1, stream-major) in decoding order, back to back; *bytes receives the total size (also on H264MI_ECAPACITY).  All frames are resolved
 * before anything is launched: one frame AUTO cannot resolve fails the call (H264MI_EUNSUPPORTED) with nothing written. */
int32_t h264mi_batch_convert_device(h264mi_decoder *dec, int32_t stream, int32_t format, int32_t csc, void *dst_device, size_t cap, size_t *bytes);

/* ---- Scaled output (K8): resize while converting, on the device ----
 * A scaled frame is a function of the tight I420 frame, the output size ow x oh and the filter; a scaled and converted frame is the function of
 * "Output formats" above applied to the scaled I420 frame of size ow x oh.  All arithmetic is integer, >> is a floor shift; this comment is the contract.
 * Sizes: luma is scaled from w x h to ow x oh, each chroma plane from ceil(w / 2) x ceil(h / 2) to ceil(ow / 2) x ceil(oh / 2), per plane and per axis
 * independently.  Source samples are those of the tight I420 frame: every clamp is at the edges of the display planes, coded samples outside the crop
 * rectangle are never read.  Chroma planes are scaled as planes, centre-aligned: the siting of chroma_sample_loc_type is not modelled in the scaler
 * (as for the upsampling above, only type 0 is, and only there).  In a monochrome stream the chroma is 128 and stays 128.  Frames are scaled as they are,
 * whether coded as frame or field pictures: scaling a woven frame blends its two fields, so deinterlace first ("Deinterlaced output" below).
 * H264MI_SCALE_BILINEAR, for an axis of n_in samples scaled to n_out, output index i:
 *   step = (n_in << 16) / n_out (floor);  P = i step + (step >> 1) - 32768, clamped to 0 .. (n_in - 1) << 16;  a = P >> 16;  f = (P >> 8) & 255;
 *   b = min(a + 1, n_in - 1);  with (ax, bx, fx) of the column and (ay, by, fy) of the row the sample is
 *   ((256 - fy) ((256 - fx) S[ay][ax] + fx S[ay][bx]) + fy ((256 - fx) S[by][ax] + fx S[by][bx]) + 32768) >> 16
 *   -- one rounding; everything fits 32 bits for n_in, n_out <= 16384 (i step < n_in << 16 <= 2^30, the sum is below 2^24); n_out == n_in gives f = 0,
 *   a = i: the identity.
 * H264MI_SCALE_AREA, downscaling only (ow <= w and oh <= h for every frame of the call, else H264MI_EINVAL): output sample i of an axis weighs source
 *   sample k by the overlap of [i n_in, (i + 1) n_in) with [k n_out, (k + 1) n_out): max(0, min((i + 1) n_in, (k + 1) n_out) - max(i n_in, k n_out)); the
 *   weights of one output sample sum to n_in.  The sample is (sum_y wy sum_x wx S + ((w_p h_p) >> 1)) / (w_p h_p) with w_p x h_p the source plane: unsigned
 *   32-bit arithmetic and one floor division per output sample.  That needs 255 w h + ((w h) >> 1) < 2^32 (the largest sum and its rounding term: about
 *   16.8 million samples): a larger display size is H264MI_EUNSUPPORTED with the reason.  n_out == n_in is the identity.
 * Formats: H264MI_FMT_I420 -- the scaled planes, tight, H264MI_I420_SIZE(ow, oh) bytes -- and _NV12, _RGB24, _RGBP: exactly the rule of "Output formats"
 * applied to the scaled frame (the same coefficient sets; nearest or H264MI_CSC_CHROMA_BILINEAR upsampling of the SCALED chroma planes; csc must be 0 for
 * I420 and NV12).  H264MI_CSC_AUTO resolves per frame from that frame's SPS and its display (source) size, never from the output size. */
#define H264MI_SCALE_BILINEAR 0
#define H264MI_SCALE_AREA 1
#define H264MI_SCALE_MAX 16384 /* the largest out_w, out_h (and axis of h264mi_scale_taps) */
/* The rule above for one output index of one axis, as a pure function (no decoder, no device): tap t (0 <= t < *count) reads source sample
 * min(*first + t, n_in - 1) with weights[t].  Bilinear: two taps, a and b, with weights {256 - f, f} as they come out -- at the far clamp b is a again.
 * Area: the overlapping source samples with their overlaps (they sum to n_in; at most ceil(n_in / n_out) + 1 of them).  *first and *count are also set
 * on H264MI_ECAPACITY (cap < *count: nothing is written to weights).  H264MI_EINVAL: an unknown filter, n_in or n_out outside 1 .. H264MI_SCALE_MAX,
 * i outside 0 .. n_out - 1, area with n_out > n_in. */
int32_t h264mi_scale_taps(int32_t filter, int32_t n_in, int32_t n_out, int32_t i, int32_t *first, int32_t *count, int32_t *weights, int32_t cap);
/* One frame of the last executed batch, cropped, scaled to out_w x out_h and converted on the device (K8) into the DEVICE buffer dst_device;
 * cap >= h264mi_output_size(format, out_w, out_h).  Asynchronous on the decoder's stream, like h264mi_frame_convert_device. */
int32_t h264mi_frame_scale_device(h264mi_decoder *dec, int32_t stream, int32_t frame, int32_t format, int32_t csc, int32_t out_w, int32_t out_h,
                                  int32_t filter, void *dst_device, size_t cap);
/* The same for every frame of the last executed batch in ONE launch -- h264mi_batch_convert_device's contract: frames of stream `stream` (or of all
 * streams when stream = -1, stream-major) in decoding order, back to back; *bytes receives the total size (also on H264MI_ECAPACITY); nothing is written
 * on failure.  Every frame comes out at out_w x out_h whatever its display size, so a batch of unlike streams is one uniform array of
 * n * h264mi_output_size(format, out_w, out_h) bytes.  H264MI_EINVAL: out_w or out_h outside 1 .. H264MI_SCALE_MAX, an unknown filter, area upscaling in
 * either axis of any frame of the call, an illegal format / csc pair.  All frames are checked and resolved before anything is launched. */
int32_t h264mi_batch_scale_device(h264mi_decoder *dec, int32_t stream, int32_t format, int32_t csc, int32_t out_w, int32_t out_h, int32_t filter,
                                  void *dst_device, size_t cap, size_t *bytes);

/* ---- Model input (K9): regions of frames as letterboxed, normalised float tensors, on the device ----
 * One launch takes a list of (frame, region) items and writes one tensor item per entry, all of one canvas size.  A tensor item is a function of the
 * tight I420 frame, the region, the spec, the rule of "Scaled output" and the rule of "Output formats", and of nothing else; this comment is the contract.
 * 1. Region.  (x, y, w, h) in display coordinates of the frame; w = h = 0 stands for the whole frame.  Legal: x and y even, w, h >= 1, x + w <= the
 *    display width, y + h <= the display height; anything else is H264MI_EINVAL.  The region frame is the tight I420 frame with Y = Ydisp[y : y + h, x : x + w]
 *    and C = Cdisp[y / 2 : y / 2 + ceil(h / 2), x / 2 : x / 2 + ceil(w / 2)] for both chroma planes (always inside the display chroma plane).  Every
 *    clamp below is at the edges of the region frame: samples outside the region are never read.
 * 2. Placement.  h264mi_fit_rect gives the picture's place (px, py) and size sw x sh in the out_w x out_h canvas.  H264MI_FIT_STRETCH: (0, 0, out_w, out_h).
 *    H264MI_FIT_LETTERBOX, 32-bit integers, / is floor: if w out_h >= h out_w: sw = out_w, sh = clamp((2 h out_w + w) / (2 w), 1, out_h); else
 *    sh = out_h, sw = clamp((2 w out_h + h) / (2 h), 1, out_w); px = (out_w - sw) >> 1, py = (out_h - sh) >> 1.  (The aspect ratio kept to the nearest
 *    pixel, the picture centred, the odd pixel of padding right / below.)  All sizes are 1 .. H264MI_SCALE_MAX, so the largest intermediate is
 *    2 * 16384^2 + 16384 < 2^31.
 * 3. Picture.  The region frame scaled to sw x sh by "Scaled output" (filter: H264MI_SCALE_BILINEAR or _AREA; area needs sw <= w and sh <= h for every
 *    item of the call, else H264MI_EINVAL, and its 32-bit bound applies to the region: 255 w h + ((w h) >> 1) < 2^32, else H264MI_EUNSUPPORTED), then
 *    converted to 8-bit R, G, B by "Output formats" applied to the scaled frame: csc as there, H264MI_CSC_CHROMA_BILINEAR upsampling the SCALED chroma
 *    planes.  H264MI_CSC_AUTO resolves per item from the frame's SPS and its DISPLAY size -- never from the region or the canvas.
 * 4. Canvas.  out_h x out_w pixels: pixel (px + i, py + j) is picture pixel (i, j); every other pixel is pad[0], pad[1], pad[2] = R, G, B (pad[3] is ignored).
 * 5. Element.  An 8-bit value v of colour c (R, G, B = 0, 1, 2) becomes
 *      H264MI_DT_U8    v; scale must be exactly {1, 1, 1} and bias {0, 0, 0}, else H264MI_EINVAL
 *      H264MI_DT_F32   r = fl32(fl32(float(v) * scale[c]) + bias[c]): two IEEE binary32 operations, each rounded to nearest even -- NOT a fused
 *                      multiply-add -- subnormals kept
 *      H264MI_DT_F16   r converted to binary16, round to nearest even; subnormals kept, overflow gives infinity
 *      H264MI_DT_BF16  r converted to bfloat16, round to nearest even: for finite r with binary32 bit pattern u, (u + 0x7fff + ((u >> 16) & 1)) >> 16
 *    scale and bias must be finite, else H264MI_EINVAL.  Pad bytes go through the same mapping.
 * 6. Layout.  H264MI_FMT_RGBP: three out_h x out_w planes (CHW); H264MI_FMT_RGB24: out_h x out_w x 3 (HWC); any other format is H264MI_EINVAL.
 *    H264MI_TENSOR_BGR in flags writes colour c at channel position 2 - c; scale, bias and pad stay indexed by colour.  Items are written back to back in
 *    item order, each 3 * out_w * out_h * (1, 2, 2, 4) bytes (h264mi_tensor_size).  dst_device must be aligned to the element size, else H264MI_EINVAL. */
#define H264MI_DT_U8 0
#define H264MI_DT_F16 1
#define H264MI_DT_BF16 2
#define H264MI_DT_F32 3
#define H264MI_FIT_STRETCH 0
#define H264MI_FIT_LETTERBOX 1
#define H264MI_TENSOR_BGR 1 /* h264mi_tensor_spec.flags */
typedef struct {
    int32_t format, dtype, csc, out_w, out_h, filter, fit, flags;
    uint8_t pad[4];
    float scale[3], bias[3];
} h264mi_tensor_spec;
typedef struct {
    int32_t stream, frame, x, y, w, h; /* a frame of the last executed batch and a region of it (w = h = 0: the whole frame) */
} h264mi_tensor_item;
/* Rule 2 as a pure function (no decoder, no device).  H264MI_EINVAL: an unknown fit, a size outside 1 .. H264MI_SCALE_MAX, a null pointer. */
int32_t h264mi_fit_rect(int32_t fit, int32_t w, int32_t h, int32_t out_w, int32_t out_h, int32_t *px, int32_t *py, int32_t *sw, int32_t *sh);
/* Bytes of one tensor item of the spec.  Pure; validates the spec: H264MI_EINVAL for a format other than _RGBP / _RGB24, an unknown dtype, filter, fit
 * or flag bit, an illegal csc, out_w or out_h outside 1 .. H264MI_SCALE_MAX, a scale or bias that is not finite, H264MI_DT_U8 with scale != 1 or bias != 0. */
int32_t h264mi_tensor_size(const h264mi_tensor_spec *spec, size_t *bytes);
/* The items of the list, in ONE launch (K9), back to back into the DEVICE buffer dst_device, asynchronous on the decoder's stream; `stream` and `frame`
 * of an item refer to the last executed batch, and the same frame may appear in many items.  h264mi_batch_scale_device's discipline: every item is
 * checked, resolved and sized before anything is launched; *bytes receives n * h264mi_tensor_size (also on H264MI_ECAPACITY); nothing is written on
 * failure; n = 0 succeeds with *bytes = 0. */
int32_t h264mi_items_tensor_device(h264mi_decoder *dec, const h264mi_tensor_spec *spec, const h264mi_tensor_item *items, int32_t n, void *dst_device,
                                   size_t cap, size_t *bytes);
/* The same for the whole of every frame of the last executed batch: frames of stream `stream` (or of all streams when stream = -1, stream-major) in
 * decoding order -- h264mi_batch_scale_device's order. */
int32_t h264mi_batch_tensor_device(h264mi_decoder *dec, int32_t stream, const h264mi_tensor_spec *spec, void *dst_device, size_t cap, size_t *bytes);

/* ---- Deinterlaced output (K10): derived frames for the output calls above, on the device ----
 * The output stage weaves the two fields of a frame into one frame.  A deinterlaced frame is a tight I420 frame of the same display size w x h as its
 * source, and a function of the source's tight I420 frame (what h264mi_frame_read(crop = 1) returns), a mode and a parity p (0 = top: even rows are kept;
 * 1 = bottom: odd rows are kept), and of nothing else; this comment is the contract.  Each plane is processed on its own with the same parity: luma has
 * hp = h rows and wp = w columns, each chroma plane hp = ceil(h / 2) rows and wp = ceil(w / 2) columns.  Parity counts rows of the DISPLAY plane; in
 * streams with frame_mbs_only_flag 0 the crop units (7.4.2.1.1: two luma rows for monochrome, four otherwise) make the crop origin even in every plane that
 * carries samples (the chroma of a monochrome stream is 128 throughout), so that is the coded parity as well.  Every clamp is at the edge of the display plane: coded samples outside the crop rectangle are never read.  All
 * arithmetic is in integers, >> is a floor shift.
 *   H264MI_DEINT_FIELD  rows with (y & 1) == p are copied.  Any other row: up = y - 1, dn = y + 1; if up < 0 then up = dn; if dn >= hp then dn = up; if
 *                       neither exists (hp == 1, p == 1) the row is copied; otherwise out[y][x] = (S[up][x] + S[dn][x] + 1) >> 1.
 *   H264MI_DEINT_BLEND  parity is ignored and must be 0.  Every row: out[y][x] = (S[max(y - 1, 0)][x] + 2 S[y][x] + S[min(y + 1, hp - 1)][x] + 2) >> 2 --
 *                       one rounding, not two chained averages.
 *   H264MI_DEINT_EDGE   chroma planes follow FIELD.  Luma: kept rows are copied.  A missing row whose up and dn both exist inside the plane and are
 *                       distinct tries the directions d = 0, -1, +1 in that order with cost_d = |S[up][cx(x + d)] - S[dn][cx(x - d)]|,
 *                       cx(t) = clamp(t, 0, wp - 1), takes the first direction of the strictly smallest cost and writes
 *                       (S[up][cx(x + d)] + S[dn][cx(x - d)] + 1) >> 1.  A missing row at the plane's edge (up == dn after the clamp) is S[up][x]; the
 *                       hp == 1 case is as in FIELD.
 * Any other mode is H264MI_EINVAL.  A parity is 0, 1 or H264MI_DEINT_PARITY_FIRST: the first_parity of the frame (h264mi_frame_fields), resolved per frame.
 * The three modes are spatial: they read one frame.  The motion-adaptive modes, which also read the frame before it -- across batch boundaries too -- have
 * entry points of their own: "Motion-adaptive deinterlacing" below.  Out of scope: look-ahead (a successor frame); interlace-aware chroma upsampling inside K7 (chroma
 * planes are deinterlaced as planes, then upsampled by the rule of "Output formats"); pulldown detection and SEI pic_struct; MBAFF, as everywhere. */
#define H264MI_DEINT_FIELD 0
#define H264MI_DEINT_BLEND 1
#define H264MI_DEINT_EDGE 2
#define H264MI_DEINT_PARITY_FIRST (-1)
/* The rule for row y of a plane of n_rows rows, as a pure function (no decoder, no device).  *kept = 1: the row is copied, *up and *dn are both y.  Else
 * *up and *dn are the rows above and below after the clamps (FIELD / EDGE: equal at the plane's edge; BLEND: always *kept = 0 and the two clamped
 * neighbours of y).  H264MI_EINVAL: an unknown mode, a parity outside 0 / 1, a non-zero parity with BLEND, n_rows outside 1 .. H264MI_SCALE_MAX, y outside
 * 0 .. n_rows - 1, a null pointer. */
int32_t h264mi_deint_rows(int32_t mode, int32_t parity, int32_t n_rows, int32_t y, int32_t *kept, int32_t *up, int32_t *dn);
/* What a frame's fields are.  field_coded: 1 if the frame was coded as two field pictures (a frame that went out with one field missing or concealed
 * counts as 1), else 0.  top_field_order_cnt / bottom_field_order_cnt: TopFieldOrderCnt and BottomFieldOrderCnt (8.2.1), after a possible memory
 * management operation 5, like pic_order_cnt of h264mi_frame_get_info; of a frame that went out with one field missing both are the count of the field
 * there is.  first_parity: 1 if the bottom count is lower than the top count, else 0 -- for a picture with operation 5 the relation before the counts
 * are rewritten; for a frame with one field missing the parity of the field there is; for a frame of two field pictures with EQUAL counts
 * (pic_order_cnt_type 2 gives both fields of a reference frame one count, and output order is decoding order there, 8.2.1.3) the parity of the field
 * that was decoded first. */
typedef struct {
    int32_t field_coded, top_field_order_cnt, bottom_field_order_cnt, first_parity;
} h264mi_field_info;
int32_t h264mi_frame_fields(h264mi_decoder *dec, int32_t stream, int32_t frame, h264mi_field_info *out);
/* Derived frames.  A deinterlace call makes one derived frame per item, in ONE launch (K10) on the decoder's stream, with the discipline of the output
 * calls: everything is checked, resolved and sized first, a call that fails launches nothing and leaves the previous list as it was.  Each call REPLACES
 * the decoder's list of derived frames; n = 0 empties it; h264mi_batch_execute, h264mi_decoder_reset and h264mi_stream_reset (of any stream) empty it too.
 * *n_derived (may be NULL) receives the length of the new list.  Derived frame k is frame k of the pseudo-stream H264MI_STREAM_DERIVED, and these calls
 * accept it: h264mi_stream_frame_count; h264mi_frame_get_info, h264mi_frame_colour and h264mi_frame_fields, which report the SOURCE's values;
 * h264mi_frame_read with crop = 1; every frame, batch and item call of K6 .. K9 (as `stream` of a batch call it means the derived frames only: -1 is
 * still the frames of the real streams).  Every other per-frame accessor -- h264mi_frame_read with crop = 0, h264mi_frame_device_planes,
 * h264mi_frame_read_mbrecs, h264mi_frame_read_mbmv1, h264mi_frame_concealed, h264mi_stream_output_order, h264mi_frame_ref_pocs and the side-information
 * calls of K11 (a derived frame has no macroblocks) -- returns H264MI_EINVAL for it, and so does a deinterlace item that names it.  The contract: a deinterlaced and converted / scaled / tensor item is the function of "Output formats" / "Scaled
 * output" / "Model input" applied to the deinterlaced frame; H264MI_CSC_AUTO still resolves from the source's SPS and display size.
 * A derived frame lives in decoder-owned device memory in the layout of a frame slot of its source's coded size, of which only the display rectangle is
 * written, at the source's crop origin.  The arena grows to the largest call and is kept, is zero-filled when allocated, is counted by
 * h264mi_decoder_memory and freed by h264mi_decoder_destroy; a call that cannot get its memory returns H264MI_ENOMEM with the previous list intact.
 * There is no limit on n other than that.
 * h264mi_items_deinterlace: item i is frame `frame` of stream `stream` of the last executed batch under `mode` with `parity` (0, 1 or
 * H264MI_DEINT_PARITY_FIRST; with H264MI_DEINT_BLEND it must be 0); the same frame may appear in many items.
 * h264mi_batch_deinterlace: every frame of stream `stream` (or of all streams when stream = -1, stream-major) in decoding order.  rate = 1: one derived
 * frame per frame, of parity first_parity (0 under BLEND).  rate = 2: two per frame, first_parity then the other -- field rate, "bob"; BLEND needs
 * rate = 1.  Any other rate is H264MI_EINVAL. */
#define H264MI_STREAM_DERIVED 0x40000000 /* far above any max_streams */
typedef struct {
    int32_t stream, frame, parity;
} h264mi_deint_item;
int32_t h264mi_items_deinterlace(h264mi_decoder *dec, int32_t mode, const h264mi_deint_item *items, int32_t n, int32_t *n_derived);
int32_t h264mi_batch_deinterlace(h264mi_decoder *dec, int32_t stream, int32_t mode, int32_t rate, int32_t *n_derived);

/* ---- Motion-adaptive deinterlacing (K10, second kernel): derived frames from a frame AND its predecessor ----
 * A motion-adaptive deinterlaced frame is a function of the source's tight I420 frame S, a predecessor's tight I420 frame P of the same display size or
 * "none", a spatial mode M -- H264MI_DEINT_FIELD or H264MI_DEINT_EDGE -- and a parity p, and of nothing else; this comment is the contract.  Each plane is
 * processed on its own with the same parity; plane sizes, parity and clamps are those of "Deinterlaced output" (luma h x w, chroma ceil(h / 2) x
 * ceil(w / 2), every clamp at the edge of the display plane); all arithmetic is in integers.
 *   Kept rows     A row for which h264mi_deint_rows(M, p, hp, y) says kept is copied from S (the one-row, p = 1 case included).
 *   Missing rows  With up / dn of row y from the same function:
 *                   sp[x] = the value mode M writes there: FIELD's average, or on luma EDGE's directional value with its up == dn case (chroma
 *                           follows FIELD);
 *                   t[x]  = S[y][x], the sample of the other field: the weave;
 *                   m[x]  = max(|S[up][x] - P[up][x]|, |S[dn][x] - P[dn][x]|, |S[y][x] - P[y][x]|): how far each of the three rows moved since the
 *                           predecessor, same parity against same parity;
 *                   out[y][x] = min(max(sp[x], t[x] - m[x]), t[x] + m[x]): the spatial value, pulled to within m of the weave.
 *   Properties    Where nothing moved (m = 0) the woven sample goes out, at full vertical resolution; where much moved the spatial value goes out; the
 *                 result always lies in 0 .. 255 (between sp and t).
 *   No predecessor  out = sp: the frame equals mode M's frame bit for bit.
 *   P is S itself   the frame equals the source frame bit for bit (m = 0 everywhere).
 * The rule is causal on purpose: it adds no latency and needs nothing from the next batch.  Not supported: H264MI_DEINT_BLEND has no parity and is
 * H264MI_EINVAL here; look-ahead (a successor frame), pulldown detection, SEI pic_struct and MBAFF stay out of scope.
 * h264mi_deint_motion_pixel: the rule of one sample as a pure function (no decoder, no device).  s and p hold the samples of S and P at rows up, y and dn
 * (in that order) of one column, sp the spatial value (0 .. 255); p = NULL means no predecessor (*out = sp).  H264MI_EINVAL: s or out NULL, sp outside
 * 0 .. 255.
 * Derived frames: the two calls below have the discipline of h264mi_items_deinterlace -- everything is checked first, a call that fails launches
 * nothing and leaves the list of derived frames intact, a call that succeeds REPLACES it, in ONE launch on the decoder's stream -- and share its list,
 * its arena and the pseudo-stream H264MI_STREAM_DERIVED.
 * h264mi_items_deinterlace_motion: item i is frame `frame` of stream `stream` of the last executed batch under `mode` with `parity` (0, 1 or
 * H264MI_DEINT_PARITY_FIRST) against `prev_frame`: a frame of the SAME stream in the last executed batch (it may be `frame` itself),
 * H264MI_DEINT_PREV_NONE, or H264MI_DEINT_PREV_HISTORY -- the stream's history, which must be valid (below).  A predecessor whose coded size or display
 * rectangle differs from the source's is H264MI_EINVAL, and so are any other prev_frame, a history that is not valid, and H264MI_STREAM_DERIVED as a source.
 * h264mi_batch_deinterlace_motion: items and their order are h264mi_batch_deinterlace's (decoding order, stream-major; rate 2: the first parity, then
 * the other).  A frame's predecessor is the frame before it in h264mi_stream_output_order of its stream; both derived frames of a rate-2 frame share it;
 * a predecessor of another coded size or display rectangle resolves to none.  The first frame in output order takes the stream's history if
 * flags & H264MI_DEINT_HISTORY and the history is valid, and has none otherwise.  Any other flag bit, and H264MI_STREAM_DERIVED, are H264MI_EINVAL.
 * History: one frame slot per stream in an arena of the decoder's own, allocated on first use (the first batch call with H264MI_DEINT_HISTORY),
 * zero-filled, counted by h264mi_decoder_memory and freed by h264mi_decoder_destroy; H264MI_ENOMEM leaves everything as it was.  With the flag the batch
 * call copies, after its launch and on the decoder's stream, the source of each covered stream's last frame in output order into that stream's slot; the
 * next pass waits for the launch and the copies.  A history is valid only if it was taken in the batch prepared immediately before the one executed
 * last, its coded size and display rectangle equal the source's, and neither h264mi_stream_reset of that stream nor h264mi_decoder_reset came in between:
 * executing the same prepared batch again does not make its own history its predecessor, and a batch in between that took no history ends it.
 * h264mi_derived_prev: what derived frame k was made from: a frame index, H264MI_DEINT_PREV_NONE, or H264MI_DEINT_PREV_HISTORY; for a derived frame of
 * the three spatial modes H264MI_DEINT_PREV_NONE.  H264MI_EINVAL: no such derived frame, a null pointer. */
#define H264MI_DEINT_PREV_NONE (-1)
#define H264MI_DEINT_PREV_HISTORY (-2)
#define H264MI_DEINT_HISTORY 1 /* flags of h264mi_batch_deinterlace_motion */
typedef struct {
    int32_t stream, frame, parity, prev_frame;
} h264mi_deint_motion_item;
int32_t h264mi_deint_motion_pixel(const uint8_t s[3], const uint8_t p[3], int32_t sp, int32_t *out);
int32_t h264mi_items_deinterlace_motion(h264mi_decoder *dec, int32_t mode, const h264mi_deint_motion_item *items, int32_t n, int32_t *n_derived);
int32_t h264mi_batch_deinterlace_motion(h264mi_decoder *dec, int32_t stream, int32_t mode, int32_t rate, int32_t flags, int32_t *n_derived);
int32_t h264mi_derived_prev(h264mi_decoder *dec, int32_t k, int32_t *prev);

/* ---- Macroblock side information (K11): motion, references, types, QP and coded-block flags as planes, on the device ----
 * What the reference's SliceData holds per macroblock (h264/slice.go:77-102 has no pixel in it), laid out per 4x4 luma block for every frame of a
 * list in ONE launch.  No sample is read; this comment is the contract.
 * Grid.  A frame of display size w x h has gw = ceil(w / 4) by gh = ceil(h / 4) cells.  Cell (j, i) (row, column) describes the coded 4x4 luma block that
 *   holds display sample (4 i, 4 j): the block at column bx = (crop_x >> 2) + i and row by = (crop_y >> 2) + j of the coded picture, block (bx & 3, by & 3) of
 *   macroblock (bx >> 2, by >> 2), quadrant (8x8 block) ((by & 3) >> 1) * 2 + ((bx & 3) >> 1) of it.  Every cell lies inside the coded picture.
 * Planes.  `planes` is a bit set; the selected planes are written in ascending bit order, each gh x gw int16, row-major and tight; items follow back to
 *   back, like K6's frames: h264mi_side_size bytes each.  The value of a cell:
 *   H264MI_SIDE_TYPE   the macroblock's class, H264MI_MB_*.  H264MI_MB_B stands for every coded inter type of a B slice but B_Direct_16x16.
 *   H264MI_SIDE_QP     QP_Y of the macroblock as its record holds it: 0 for I_PCM (what deblocking takes), the predicted QP for skipped macroblocks, 0 for
 *                      H264MI_MB_NONE.
 *   H264MI_SIDE_NZ     1 if the 4x4 luma block carries a non-zero coefficient, else 0, as the entropy kernels record it for the deblocking filter: with the
 *                      8x8 transform all four 4x4 blocks of an 8x8 block carry the flag of that 8x8 block; every block of an I_PCM macroblock reads 1.
 *   H264MI_SIDE_SLICE  ordinal of the macroblock's slice inside its picture, in the order the slices arrived; -1 for a concealed or undelivered macroblock.
 *   H264MI_SIDE_MVX0, _MVY0   final list-0 vector of the block in quarter luma samples; 0 where the block's quadrant does not use list 0.
 *   H264MI_SIDE_REF0   ref_idx_l0 of the quadrant; -1 where it does not use list 0.
 *   H264MI_SIDE_DPOC0  PicOrderCnt(that entry of RefPicList0) - PicOrderCnt(current picture), clamped to -32768 .. 32767; 0 where unused.
 *   H264MI_SIDE_MVX1, _MVY1, _REF1, _DPOC1   the same for list 1: 0 / 0 / -1 / 0 in pictures without B slices.
 *   A quadrant uses list X when its macroblock is an inter macroblock and the record names a reference picture for it in that list.  Intra and
 *   H264MI_MB_NONE macroblocks have vectors 0, references -1 and DPOC 0.  P_Skip, B_Skip and direct macroblocks report the vectors and references derived
 *   for them (8.4.1.1, 8.4.1.2).  Concealed macroblocks (h264mi_config.conceal_errors) read H264MI_MB_PSKIP, slice -1, a zero vector and ref_idx 0, which
 *   stands for the concealment reference, with its DPOC.
 *   The picture order counts are those the slice's reference lists were built with (8.2.4): a memory management operation 5 in the same picture rewrites
 *   the counts afterwards (h264mi_frame_get_info reports them rewritten); the difference is taken BEFORE that.
 * Refused: the pseudo-stream H264MI_STREAM_DERIVED (H264MI_EINVAL); a frame coded as two field pictures (h264mi_frame_fields: field_coded) is
 *   H264MI_EUNSUPPORTED -- its two fields are two pictures with interleaved rows, and a grid for them is a later piece of work.  Frame pictures of
 *   streams that mix both (PAFF) are served.
 * Out of scope: residual coefficient magnitudes, intra prediction modes, macroblock-granular output, field pictures, MBAFF (as everywhere).
 * A launch reads the macroblock records of the last executed batch; the next h264mi_batch_execute waits for it on the device before it reuses them.
 * When h264mi_batch_sync repeats a batch that ran out of residual blocks (h264mi_decoder_coef_pool), planes launched before that sync show the
 * pass that failed: launch them after the sync, as one does to read the stream status. */
#define H264MI_SIDE_TYPE 0x001
#define H264MI_SIDE_QP 0x002
#define H264MI_SIDE_NZ 0x004
#define H264MI_SIDE_SLICE 0x008
#define H264MI_SIDE_MVX0 0x010
#define H264MI_SIDE_MVY0 0x020
#define H264MI_SIDE_REF0 0x040
#define H264MI_SIDE_DPOC0 0x080
#define H264MI_SIDE_MVX1 0x100
#define H264MI_SIDE_MVY1 0x200
#define H264MI_SIDE_REF1 0x400
#define H264MI_SIDE_DPOC1 0x800
#define H264MI_SIDE_ALL 0xFFF
#define H264MI_MB_NONE 0 /* not delivered by any slice, and not concealed */
#define H264MI_MB_I4x4 1
#define H264MI_MB_I8x8 2
#define H264MI_MB_I16x16 3
#define H264MI_MB_IPCM 4
#define H264MI_MB_P16x16 5
#define H264MI_MB_P16x8 6
#define H264MI_MB_P8x16 7
#define H264MI_MB_P8x8 8
#define H264MI_MB_PSKIP 9
#define H264MI_MB_B 10
#define H264MI_MB_BDIRECT 11
#define H264MI_MB_BSKIP 12
/* Grid and bytes of one item (pure: no decoder, no device): *gw = ceil(w / 4), *gh = ceil(h / 4), *bytes = 2 gw gh x the number of planes; any of the three
 * pointers may be NULL.  H264MI_EINVAL: planes == 0 or a bit outside H264MI_SIDE_ALL, w or h outside 1 .. H264MI_SCALE_MAX. */
int32_t h264mi_side_size(int32_t planes, int32_t w, int32_t h, int32_t *gw, int32_t *gh, size_t *bytes);
/* The reference lists behind REF and DPOC: the picture order counts of the active entries of RefPicList`list` (0 / 1) of slice `slice` (ordinal in its
 * picture, the value of H264MI_SIDE_SLICE) of a frame of the last executed batch, and the current picture's count, both as of list-building time
 * (an entry that names a non-existing frame of a frame_num gap reads that frame's inferred count).  *n receives the number of active entries -- 0 for I
 * slices and for list 1 of P slices; at most cap values are written (H264MI_ECAPACITY if there are more; *n and *cur_poc are set).  slice = -1 is the
 * concealment pseudo-slice: *n = 1 if the picture has a concealment reference (list 0 only), else 0.  Needs no device work.  H264MI_EINVAL: no such
 * frame or slice, list outside 0 / 1, H264MI_STREAM_DERIVED; H264MI_EUNSUPPORTED: a frame coded as two field pictures.  cur_poc and pocs may be NULL. */
int32_t h264mi_frame_ref_pocs(h264mi_decoder *dec, int32_t stream, int32_t frame, int32_t slice, int32_t list, int32_t *cur_poc, int32_t *pocs,
                              int32_t cap, int32_t *n);
typedef struct {
    int32_t stream, frame; /* a frame of the last executed batch */
} h264mi_side_item;
/* The items of the list, in ONE launch (K11), back to back into the DEVICE buffer dst_device (aligned to 2 bytes, else H264MI_EINVAL), asynchronous on the
 * decoder's stream.  h264mi_batch_scale_device's discipline: every item is checked and sized before anything is launched; *bytes receives the total
 * size (also on H264MI_ECAPACITY); nothing is written on failure; n = 0 succeeds with *bytes = 0; the same frame may appear in several items. */
int32_t h264mi_items_side_device(h264mi_decoder *dec, int32_t planes, const h264mi_side_item *items, int32_t n, void *dst_device, size_t cap, size_t *bytes);
/* The same for every frame of the last executed batch: frames of stream `stream` (or of all streams when stream = -1, stream-major) in decoding order. */
int32_t h264mi_batch_side_device(h264mi_decoder *dec, int32_t stream, int32_t planes, void *dst_device, size_t cap, size_t *bytes);

/* ---- Frame statistics (K12): sums, a histogram and differences against a predecessor, on the device ----
 * What a caller needs to decide which frames are worth converting -- shot boundaries, frozen or black frames, the part of a frame that changed -- without
 * moving a sample off the device or through a tensor.  The reference has no such stage (h264/server.go:113-166 stops at the parsed slice).
 * The statistics of an item are a function of the source's tight I420 frame S (what h264mi_frame_read(crop = 1) returns), a predecessor's tight I420
 * frame P of the same display size or "none", a cell size and a threshold, and of nothing else; this comment is the contract.  Luma is h x w, each
 * chroma plane ceil(h / 2) x ceil(w / 2), as in "Deinterlaced output"; only samples of the display rectangle are read; the chroma of a monochrome stream
 * is 128 throughout and is counted like any other.  All arithmetic is in integers.
 * Record.  h264mi_frame_stats, 1120 bytes, naturally aligned, little-endian, written by the device:
 *   sum_y, sum_y2            the sum of S and of S * S over luma
 *   sum_cb, sum_cr           the sum of S over Cb and over Cr
 *   sad_y, sse_y             the sum of |S - P| and of (S - P) * (S - P) over luma
 *   sad_cb, sad_cr           the sum of |S - P| over Cb and over Cr.  All four difference sums are 0 with no predecessor.
 *   min_y, max_y             the smallest and the largest luma sample
 *   changed_y                the number of luma samples with |S - P| > thresh; 0 with no predecessor
 *   has_prev                 1 with a predecessor, else 0
 *   w, h                     the display size
 *   gw, gh                   the grid size; 0, 0 without a grid
 *   hist_y[v]                the number of luma samples equal to v
 * Grid.  cell is 8, 16, 32 or 64; gw = ceil(w / cell), gh = ceil(h / cell).  Cell (j, i) (row, column) covers display luma rows j * cell ..
 *   min((j + 1) * cell, h) - 1 and the columns likewise: edge cells are partial, and cells are anchored at the display origin, not the coded one.
 *   `planes` is a bit set: H264MI_STATS_CELL_SUM is the sum of S over the cell, H264MI_STATS_CELL_SAD the sum of |S - P| over it (all 0 without a
 *   predecessor).  The selected planes follow the record in ascending bit order, each gh x gw uint32_t, row-major and tight.  cell = 0 goes with
 *   planes = 0 and only with it: no grid.
 * Item.  One item occupies 1120 + roundup16(4 * gw * gh * popcount(planes)) bytes (h264mi_stats_size); items follow one another back to back, so every
 *   record is 16-byte aligned when dst_device is -- it must be, else H264MI_EINVAL.
 * Spec.  h264mi_stats_spec: cell and planes as above, thresh 0 .. 255, flags 0; anything else is H264MI_EINVAL.
 * Bounds.  With w, h <= H264MI_SCALE_MAX every uint64_t field is below 2^46 (2^28 samples x 255 x 255 < 2^44) and every uint32_t field below 2^31 (a
 *   count is at most 2^28, a cell sum at most 64 x 64 x 255 < 2^20): signed 64- and 32-bit views of a record are exact.
 * Invariants.  The sum of hist_y is w * h; the sum of v * hist_y[v] is sum_y; hist_y[min_y] and hist_y[max_y] are the first and the last non-zero bin;
 *   the CELL_SUM plane sums to sum_y and the CELL_SAD plane to sad_y; with P = S every difference field and changed_y are 0 and has_prev is 1.
 * h264mi_stats_size: grid and bytes of one item of a w x h frame as a pure function (no decoder, no device); any of the three pointers may be NULL.
 *   H264MI_EINVAL: a null or illegal spec, w or h outside 1 .. H264MI_SCALE_MAX.
 * h264mi_items_stats_device: item i is frame `frame` of stream `stream` of the last executed batch against `prev_frame`: a frame of the SAME stream in
 *   the last executed batch (it may be `frame` itself), H264MI_STATS_PREV_NONE, or H264MI_STATS_PREV_HISTORY -- the stream's statistics history, which
 *   must be valid (below).  A predecessor whose coded size or display rectangle differs from the source's is H264MI_EINVAL, and so is any other
 *   prev_frame.  The source may be a frame of H264MI_STREAM_DERIVED; its prev_frame is then H264MI_STATS_PREV_NONE or another derived frame, and
 *   H264MI_STATS_PREV_HISTORY is H264MI_EINVAL.  The discipline is h264mi_items_side_device's: every item is checked and sized before anything is
 *   launched; *bytes receives the total size (also on H264MI_ECAPACITY); nothing is written and nothing is launched on failure; n = 0 succeeds with
 *   *bytes = 0; the same frame may appear in many items.  ONE launch (K12) on the decoder's stream, behind a clear of the destination range on the same
 *   stream; the next pass waits for it before it rewrites the frames.
 * h264mi_batch_stats_plan: the items h264mi_batch_stats_device would use, without a device: every frame of `stream` (of all streams for -1,
 *   stream-major) in decoding order, each against the frame before it in h264mi_stream_output_order of its stream; a predecessor of another coded size
 *   or display rectangle resolves to H264MI_STATS_PREV_NONE.  The first frame in output order takes H264MI_STATS_PREV_HISTORY if
 *   flags & H264MI_STATS_HISTORY and the history is valid, and H264MI_STATS_PREV_NONE otherwise.  *n receives the number of items (also on
 *   H264MI_ECAPACITY: more than cap; nothing is written then); items may be NULL when cap is 0.  Any other flag bit, and H264MI_STREAM_DERIVED, are
 *   H264MI_EINVAL.
 * h264mi_batch_stats_device: the plan, then the item call; with H264MI_STATS_HISTORY it also takes the history, after the launch.
 * History: the rule of the deinterlacing history ("Motion-adaptive deinterlacing"), in an arena of its own: one frame slot per stream, allocated on first
 *   use (the first batch call with H264MI_STATS_HISTORY that launches: neither a refused call nor one that returns H264MI_ECAPACITY allocates it), zero-filled, counted by h264mi_decoder_memory and freed by h264mi_decoder_destroy;
 *   H264MI_ENOMEM leaves everything as it was.  With the flag the batch call copies, after its launch and on the decoder's stream, the whole coded frame
 *   of each covered stream's last frame in output order into that stream's slot; the next pass waits for the launch and the copies.  A history is valid
 *   only if it was taken in the batch prepared immediately before the one executed last, its coded size and display rectangle equal the source's, and
 *   neither h264mi_stream_reset of that stream nor h264mi_decoder_reset came in between.  It is a SECOND history: a statistics call and a motion-adaptive
 *   deinterlacing call in the same batch each date their own slot, so neither ends the other's.
 * Out of scope: scene-cut decisions (a threshold is a policy: the caller's arithmetic on the records), chroma histograms and chroma cells, per-item cell
 *   sizes, windowed metrics, look-ahead, the two fields of a frame separately, MBAFF (as everywhere). */
#define H264MI_STATS_CELL_SUM 1
#define H264MI_STATS_CELL_SAD 2
#define H264MI_STATS_PREV_NONE (-1)
#define H264MI_STATS_PREV_HISTORY (-2)
#define H264MI_STATS_HISTORY 1 /* flags of h264mi_batch_stats_plan / h264mi_batch_stats_device */
typedef struct {
    uint64_t sum_y, sum_y2, sum_cb, sum_cr;
    uint64_t sad_y, sse_y, sad_cb, sad_cr;
    uint32_t min_y, max_y, changed_y, has_prev, w, h, gw, gh;
    uint32_t hist_y[256];
} h264mi_frame_stats;
typedef struct {
    int32_t cell, planes, thresh, flags;
} h264mi_stats_spec;
typedef struct {
    int32_t stream, frame, prev_frame;
} h264mi_stats_item;
int32_t h264mi_stats_size(const h264mi_stats_spec *spec, int32_t w, int32_t h, int32_t *gw, int32_t *gh, size_t *bytes);
int32_t h264mi_items_stats_device(h264mi_decoder *dec, const h264mi_stats_spec *spec, const h264mi_stats_item *items, int32_t n, void *dst_device, size_t cap,
                                  size_t *bytes);
int32_t h264mi_batch_stats_plan(h264mi_decoder *dec, int32_t stream, int32_t flags, h264mi_stats_item *items, int32_t cap, int32_t *n);
int32_t h264mi_batch_stats_device(h264mi_decoder *dec, int32_t stream, const h264mi_stats_spec *spec, int32_t flags, void *dst_device, size_t cap, size_t *bytes);

/* ---- JPEG snapshots (K13): baseline JPEG files of decoded frames, on the device ----
 * A thumbnail for a seek bar, an evidence still, the key frame of an index: a frame as a FILE, without moving its samples off the device first.  A frame
 * is 8-bit 4:2:0 Y / Cb / Cr, which is JPEG's own layout: nothing is converted.  The reference has no such stage (h264/server.go:113-166 stops at the
 * parsed slice).  The bytes of an item are a function of the source's tight I420 frame S (what h264mi_frame_read(crop = 1) returns), of whether the
 * stream is monochrome, and of the spec, and of nothing else; this comment is the contract.  All arithmetic is in integers; "div" truncates
 * (all its operands are non-negative), ">>" is an arithmetic shift.
 * Geometry.  4:2:0: three components, Y sampled 2 x 2 and Cb, Cr 1 x 1 (component ids 1, 2, 3); an MCU is 16 x 16 luma samples, its blocks in the order
 *   Y00 Y01 Y10 Y11 Cb Cr (Y01 is the block to the right of Y00, Y10 the one below it).  Monochrome (chroma_format_idc 0): one component, an MCU is one
 *   8 x 8 block.  MCUs go in raster order, ceil(w / 16) x ceil(h / 16) of them (mono: ceil(w / 8) x ceil(h / 8)).  SOF0 carries the display size
 *   w x h; odd sizes are allowed.  Samples beyond the display rectangle are the rectangle's last column or row, replicated, per plane -- chroma over its
 *   ceil(w / 2) x ceil(h / 2) plane -- and never the coded samples outside the crop.
 * Quantisation tables.  Annex K.1's two tables (K.1 for Y, K.2 for Cb and Cr) scaled the IJG way: quality q is 1 .. 100, sc = 5000 div q for q < 50,
 *   else 200 - 2q, and Q = clamp((base * sc + 50) div 100, 1, 255).  (These are the tables libjpeg writes for the same quality.)
 * Block rule (forward DCT and quantisation).  A block s[y][n] (row y, column n) gives x = s - 128.  M[k][n] = rint(16384 * a_k * cos((2n + 1) k pi / 16)),
 *   a_0 = sqrt(1/8), a_k = 1/2 otherwise: M[0][*] = 5793, M[1] = 8035 6811 4551 1598 -1598 -4551 -6811 -8035, ...
 *   Rows:     r[y][k] = (sum over n of M[k][n] * x[y][n] + 128) >> 8
 *   Columns:  c[v][k] = sum over y of M[v][y] * r[y][k]
 *   Level:    level[v][k] = sign(c) * ((|c| + (Q << 19)) div (Q << 20)), Q the table's entry for (v, k)
 *   Everything fits int32: the absolute values of a row of M sum to at most 46344, so |r| <= 46344 * 128 >> 8 = 23172, |c| <= 46344 * 23172 < 1.08e9,
 *   and the addend is at most 255 << 19 < 1.34e8.  |level| <= 1024, and <= 1023 for AC coefficients (their rows of M sum to at most 41990).
 *   Against an orthonormal floating-point DCT with round-half-away the level never differs by more than 1 (measured over 42 000 blocks -- uniform noise,
 *   0 / 255 blocks, a narrow Gaussian: in 0.79 % of the coefficients at quality 100, 0.13 % at 90, 0.024 % at 50, 0.016 % at 10).
 * Entropy coding.  Baseline Huffman with the four tables of Annex K.3.3 (K.3, K.4 for DC; K.5, K.6 for AC), which are written into the file.  DC
 *   differences are taken per component and start from 0 in every restart interval.  Zigzag order; a run of 16 or more zeros takes ZRL codes; EOB is
 *   written unless coefficient 63 is non-zero.  Magnitude categories go up to 11 for DC and 10 for AC; a negative value v of category s is written as the
 *   low s bits of v - 1.
 * Restart intervals.  restart_mcus = 0: one MCU row per interval; 1 .. 65535: that many MCUs in raster order (an interval may span rows).  DRI is always
 *   written.  After every interval but the last come pad 1-bits to a byte boundary, then RST(j mod 8) for interval j = 0, 1, ...; the last interval is
 *   padded the same way and followed by EOI.  Every 0xFF byte of entropy-coded data is followed by 0x00, a byte that padding completed included.
 * File.  SOI; APP0 "JFIF" 1.01, density 1:1 without units, no thumbnail; DQT 0; DQT 1 (not for mono); SOF0; DHT DC 0, DHT AC 0, DHT DC 1, DHT AC 1 (mono:
 *   the first two), a segment each; DRI; SOS; the data; EOI.  Luma uses tables 0, chroma tables 1.  The header is 629 bytes (mono: 334).
 * Sample range, `range` of the spec.  H264MI_JPEG_RANGE_KEEP: samples as they are.  H264MI_JPEG_RANGE_FULL: limited to full range, per plane:
 *   Y' = (255 * (clamp(Y, 16, 235) - 16) + 109) div 219;  C' = clamp(128 +- (255 * |clamp(C, 16, 240) - 128| + 112) div 224, 0, 255), the sign that of
 *   C - 128.  H264MI_JPEG_RANGE_AUTO: FULL exactly when the frame's video_full_range is 0 (h264mi_frame_colour).  JFIF can only say BT.601: a BT.709 stream
 *   keeps its matrix and comes out slightly off in hue in a viewer; matrix conversion is out of scope.
 * Pure functions (no decoder, no device).  h264mi_jpeg_quant_table: the table of `quality` for luma (chroma = 0) or chroma (1), natural order
 *   (8 * row + column).  h264mi_jpeg_block: the block rule for 64 samples and a table, both in natural order.  h264mi_jpeg_size: the header's length and
 *   an upper bound of the length of ANY item of a w x h frame under `spec` (either pointer may be NULL).  The bound: a block takes at most
 *   1660 bits -- a DC code of at most 11 bits and 11 magnitude bits, and 63 AC coefficients of at most 16 + 10 bits each (a ZRL code replaces 16
 *   coefficients by 11 bits, and EOB is shorter than a coefficient) -- so with the padding of its interval at most 208 bytes a block; stuffing at most
 *   doubles every byte; every interval is followed by two marker bytes: bound_bytes = roundup16(header_bytes + 416 * blocks + 2 * intervals), below 2^32
 *   for every legal size.  H264MI_EINVAL: a null or illegal spec (quality outside 1 .. 100, an unknown range, restart_mcus outside 0 .. 65535, a flag
 *   bit), w or h outside 1 .. H264MI_SCALE_MAX.
 * Destination.  n h264mi_jpeg_result records of 16 bytes, rounded up to a multiple of 256 bytes; then n slots of slot_bytes each.  slot_bytes must be a
 *   multiple of 16 and at least the header's length, dst_device 16-byte aligned (else H264MI_EINVAL).  An item that fits its slot gets status 0 and
 *   bytes = its length, and its file lies at the start of its slot.  An item that does not fit gets status H264MI_JPEG_TRUNCATED and bytes = the length
 *   it needs, so that the caller can try again; its slot's content is unspecified, and nothing is written outside its own slot.  A slot of bound_bytes
 *   never truncates.  w, h: the size SOF0 carries.
 * h264mi_items_jpeg_device: item i is frame `frame` of stream `stream` of the last executed batch; frames of H264MI_STREAM_DERIVED are legal sources.  The
 *   discipline is h264mi_items_stats_device's: every item is checked and sized before anything is launched; *bytes receives the total size (also on
 *   H264MI_ECAPACITY); nothing is written and nothing is launched on failure; n = 0 succeeds with *bytes = 0; the same frame may appear in many items.
 *   Three launches (K13: sizing, a scan of the interval lengths, writing) on the decoder's stream; the next pass waits for them before it rewrites the
 *   frames.  The one piece of scratch is the interval table, 4 bytes per restart interval of the call: allocated on first use by a call that launches
 *   (neither a refused call nor one that returns H264MI_ECAPACITY allocates), grown to the largest call, counted by h264mi_decoder_memory and freed by
 *   h264mi_decoder_destroy; H264MI_ENOMEM leaves everything as it was.
 * h264mi_batch_jpeg_device: the same for every frame of `stream` (of all streams for -1, stream-major) in decoding order.
 * h264mi_i420_jpeg_device: n caller-held tight I420 frames of one size w x h (1 .. H264MI_SCALE_MAX) in device memory, back to back at
 *   H264MI_I420_SIZE(w, h) stride; with mono != 0 only their luma is read.  H264MI_FMT_I420 of "Scaled output" is the intended source: scale, then
 *   encode, gives thumbnails without a new resize rule.  H264MI_JPEG_RANGE_AUTO is H264MI_EINVAL here (there is no stream to ask).  The caller orders the
 *   writes of src_device ahead of the call on the decoder's stream.
 * Out of scope: progressive and arithmetic coding, optimised Huffman tables, 4:4:4 / 4:2:2 output, EXIF / ICC, the pixel aspect ratio of the VUI, rate
 *   control to a target size, matrix conversion, MBAFF (as everywhere). */
#define H264MI_JPEG_RANGE_AUTO 0
#define H264MI_JPEG_RANGE_KEEP 1
#define H264MI_JPEG_RANGE_FULL 2
#define H264MI_JPEG_TRUNCATED 1 /* h264mi_jpeg_result.status */
typedef struct {
    int32_t quality, range, restart_mcus, flags;
} h264mi_jpeg_spec;
typedef struct {
    int32_t stream, frame;
} h264mi_jpeg_item;
typedef struct {
    uint32_t bytes, status, w, h;
} h264mi_jpeg_result;
int32_t h264mi_jpeg_quant_table(int32_t quality, int32_t chroma, uint16_t q[64]);
int32_t h264mi_jpeg_block(const uint8_t s[64], const uint16_t q[64], int16_t level[64]);
int32_t h264mi_jpeg_size(const h264mi_jpeg_spec *spec, int32_t w, int32_t h, int32_t mono, size_t *header_bytes, size_t *bound_bytes);
int32_t h264mi_items_jpeg_device(h264mi_decoder *dec, const h264mi_jpeg_spec *spec, const h264mi_jpeg_item *items, int32_t n, size_t slot_bytes, void *dst_device,
                                 size_t cap, size_t *bytes);
int32_t h264mi_batch_jpeg_device(h264mi_decoder *dec, int32_t stream, const h264mi_jpeg_spec *spec, size_t slot_bytes, void *dst_device, size_t cap, size_t *bytes);
int32_t h264mi_i420_jpeg_device(h264mi_decoder *dec, const h264mi_jpeg_spec *spec, const void *src_device, int32_t w, int32_t h, int32_t mono, int32_t n,
                                size_t slot_bytes, void *dst_device, size_t cap, size_t *bytes);

/* Debug / test access to the intermediate macroblock records of a frame (host copy).
 * rec: 128 bytes per MB (layout: h264decode_amd/csrc/mi_types.h struct MbRec). */
int32_t h264mi_frame_read_mbrecs(h264mi_decoder *dec, int32_t stream, int32_t frame, uint8_t *rec, size_t cap);
/* ... and to the list-1 motion vectors of a picture with B slices: 64 bytes per MB, int16 (x, y) per 4x4 block in raster order
 * (zeros for pictures without B slices).  Together they are what h264/slice.go:77-102 SliceData holds per macroblock. */
int32_t h264mi_frame_read_mbmv1(h264mi_decoder *dec, int32_t stream, int32_t frame, uint8_t *mv1, size_t cap);

/* Time (ms) spent by the kernels of the last execute, measured with HIP events on the decoder's
 * stream: [0] entropy, [1] inter recon, [2] intra recon, [3] deblock, [4] total.  Valid after sync
 * when profiling was enabled with h264mi_decoder_set_profiling(dec, 1). */
int32_t h264mi_decoder_set_profiling(h264mi_decoder *dec, int32_t on);
int32_t h264mi_last_kernel_times(h264mi_decoder *dec, double ms[5]);
/* Duration (ms) of every single launch of one kernel in that pass, in launch order (kernel: 0 entropy, 1 inter, 2 intra,
 * 3 deblock; launch k of the pixel kernels handles picture k of every stream, so launch 0 of a GOP is the IDR picture).
 * *n receives the number of launches; at most cap values are written. */
int32_t h264mi_last_launch_times(h264mi_decoder *dec, int32_t kernel, float *ms, int32_t cap, int32_t *n);

/* Device memory (bytes) the decoder holds right now: everything is sized at create time, except what only B pictures need
 * (list-1 vectors, co-located motion arrays), which is allocated when a stream's first B slice arrives. */
int32_t h264mi_decoder_memory(h264mi_decoder *dec, int64_t *device_bytes);

/* Residual-coefficient pool: blocks (32 bytes each) the fullest of the pipelined batches still on the device took, and the
 * capacity.  Large decoders reserve 8 blocks per macroblock, not the worst case of 26 (a batch that needs more fails with
 * H264MI_EDECODE, "code 40"); the environment variable H264MI_COEF_BLOCKS_PER_MB, read at create time, sizes it.  Call after
 * h264mi_batch_sync. */
int32_t h264mi_decoder_coef_pool(h264mi_decoder *dec, int64_t *used_blocks, int64_t *capacity_blocks);
/* Slices of CABAC field pictures (h264mi_config.allow_unpinned_field_cabac) that failed in the entropy kernels since the decoder was created: what a wrong
 * value in the unpinned context tables of field-coded blocks looks like (a damaged stream looks the same). */
int32_t h264mi_decoder_unpinned_failures(h264mi_decoder *dec, int64_t *n);

/* Error concealment (h264mi_config.conceal_errors).  h264mi_frame_concealed: macroblocks of a frame of the last batch that were concealed (valid after
 * h264mi_batch_sync; 0 without the mode).  h264mi_decoder_concealed: totals since the decoder was created -- slices that failed in the entropy kernels or
 * were dropped for an unparsable header and were concealed, and concealed macroblocks (lost NAL units the decoder never saw count as macroblocks only). */
int32_t h264mi_frame_concealed(h264mi_decoder *dec, int32_t stream, int32_t frame, int32_t *n_macroblocks);
int32_t h264mi_decoder_concealed(h264mi_decoder *dec, int64_t *slices, int64_t *macroblocks);
/* Frames inserted for wholly lost pictures (H264MI_CONCEAL_PICTURES) since the decoder was created, counted like the totals above when their batch is
 * synchronised.  Their macroblocks are part of the macroblock total of h264mi_decoder_concealed; the slice total does not count them. */
int32_t h264mi_decoder_concealed_pictures(h264mi_decoder *dec, int64_t *pictures);
/* Fields inserted for wholly lost fields (H264MI_CONCEAL_LONE_FIELDS) since the decoder was created, counted the same way (h264mi_decoder_concealed_pictures
 * does not count them).  Their macroblocks are part of h264mi_frame_concealed of their frame and of the macroblock total of h264mi_decoder_concealed. */
int32_t h264mi_decoder_concealed_fields(h264mi_decoder *dec, int64_t *fields);

/* ---- Random access: start and resume decoding at recovery points ----
 * Off (H264MI_RA_OFF, the default): a stream begins at an IDR picture, and a marked stream (h264mi_decoder_set_isolation) resumes at one; nothing else
 * about the decoder changes.  With H264MI_RA_RECOVERY_POINT (any other mode: H264MI_EINVAL; the mode takes effect with the next prepare):
 * - Waiting.  A stream WAITS FOR AN ENTRY POINT while it has decoded no picture since the decoder was created or since h264mi_stream_reset /
 *   h264mi_decoder_reset, and while it is marked.
 * - Entry point.  An IDR picture, or a primary coded picture whose access unit carried a recovery point SEI message (D.1.7 / D.2.7) with
 *   recovery_frame_cnt = 0.  The values of the message are kept in the stream's state when the SEI NAL unit is parsed; the next picture that starts takes
 *   them and clears them.  A recovery point with recovery_frame_cnt > 0 (gradual refresh) is recorded and reported (h264mi_frame_entry) but is no entry point.
 * - Slices while waiting.  No slice NAL unit in front of the entry point is an error: a slice whose PPS or SPS is missing, or whose header does not
 *   parse, and every slice of a picture that is no entry point is skipped and counted (skipped_waiting_nals), and the stream's status stays H264MI_OK.
 *   SPS and PPS NAL units are handled as always.
 * - State at entry.  At a non-IDR entry picture E the stream starts from empty picture management: no reference picture that holds samples;
 *   prevPicOrderCntMsb, prevPicOrderCntLsb, prevFrameNumOffset and prevFrameNum 0; PrevRefFrameNum such that E is no frame_num gap.  E is reported
 *   with new_sequence = 1 (h264mi_stream_output_order starts over there).  PicOrderCnt values from E on differ from those of a decoder that saw the
 *   whole stream by one constant per entry.  The window is not left empty, though: it is filled with non-existing frames for the
 *   max_num_ref_frames - 1 frame_num values in front of E's -- what a sliding window held there --, with picture order counts below any the stream
 *   reaches.  They hold no samples and leave through the sliding window; they are there because RefPicList0 of a B picture lists the earlier
 *   pictures in front of the later ones, so that with an empty window every later picture would stand at a smaller index than the encoder meant
 *   for as long as a picture from before E is in the encoder's window.  (A stream whose window was not full in front of E, or was managed by marking
 *   scripts there, is not reproduced by this.)
 * - Leading pictures.  After a non-IDR entry E a picture that follows E in decoding order and whose PicOrderCnt is smaller than E's (a field: its own
 *   count, against that of E's first field or frame) is a leading picture, until the counts start over at an IDR picture or at memory management
 *   operation 5.  It is neither decoded nor output.  A non-reference leading picture leaves no reference picture; a REFERENCE leading picture (B
 *   pyramids) goes through picture management as a picture without samples: the counts of 8.2.1 advance, it enters the window as a non-existing
 *   frame with its frame_num and its PicOrderCnt (two fields as one frame) and the sliding window runs (its own marking script, if it has one, is not
 *   run), so that later lists carry the surviving pictures at the indices the encoder meant.  A slice that predicts from such a frame is not detected.
 * - Short lists.  Reference lists shorter than num_ref_idx_active are padded with "no reference picture" as always; a slice that names such an
 *   entry fails in the entropy kernel, the stream is marked, and under this mode it waits for the next ENTRY POINT, not for the next IDR picture.
 * - A stream whose chunk fails in prepare loses the entry state and the counts of that chunk together with its pictures.
 * Out of scope: entering at recovery_frame_cnt > 0, decoding leading pictures approximately, I pictures without the SEI message as entry points,
 * acting on broken_link_flag while a stream is decoded continuously, every other SEI payload. */
#define H264MI_RA_OFF 0
#define H264MI_RA_RECOVERY_POINT 1
int32_t h264mi_decoder_set_random_access(h264mi_decoder *dec, int32_t mode);
typedef struct {
    int32_t found;
    int32_t recovery_frame_cnt;
    int32_t exact_match_flag;
    int32_t broken_link_flag;
    int32_t changing_slice_group_idc;
} h264mi_recovery_point;
/* The recovery point SEI message of one SEI NAL unit (pure: no decoder).  nal: the unit from its NAL header byte on, emulation prevention bytes still
 * in.  Every sei_message() of the unit is walked (0xFF extension bytes of payload type and size included), other payloads are skipped; the first
 * payload of type 6 is reported, found = 0 if there is none.  H264MI_EBITSTREAM: the unit ends inside a message; H264MI_EINVAL: not a unit of type 6.
 * The only SEI parsing this library does. */
int32_t h264mi_sei_recovery_point(const uint8_t *nal, size_t n, h264mi_recovery_point *out);
/* What the access unit of a frame of the last batch said about random access (valid after prepare; the pseudo-stream H264MI_STREAM_DERIVED is refused).
 * recovery_point and the four values of the message: reported in either mode (a frame of two fields: the first field's).  entry: 1 only on the first
 * picture decoded after the stream waited, IDR picture or not, and only with H264MI_RA_RECOVERY_POINT. */
typedef struct {
    int32_t recovery_point;
    int32_t recovery_frame_cnt;
    int32_t exact_match_flag;
    int32_t broken_link_flag;
    int32_t changing_slice_group_idc;
    int32_t entry;
} h264mi_frame_entry_info;
int32_t h264mi_frame_entry(h264mi_decoder *dec, int32_t stream, int32_t frame, h264mi_frame_entry_info *info);
/* Counted in prepare, per stream, since the decoder was created or h264mi_stream_reset: non-IDR entry points taken; slice NAL units skipped while the
 * stream waited; leading pictures skipped (a field counts as a picture). */
typedef struct {
    int64_t entries;
    int64_t skipped_waiting_nals;
    int64_t skipped_leading_pictures;
} h264mi_random_access_stats;
int32_t h264mi_stream_random_access_stats(h264mi_decoder *dec, int32_t stream, h264mi_random_access_stats *s);

const char *h264mi_last_error_string(void);
const char *h264mi_version(void);

/* Exported but NOT part of the ABI (test hooks of this repository's own suite, may change or vanish): h264mi_internal_poison,
 * h264mi_internal_deblock_plan, h264mi_internal_band_plan, h264mi_internal_intra_plan, h264mi_internal_pack_pending, h264mi_internal_side_pending, h264mi_internal_deblock_phase_clocks, h264mi_internal_vlc_selftest. */

#ifdef __cplusplus
}
#endif
#endif
