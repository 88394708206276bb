/*
 * streamgen/sg.h -- synthetic H.264 Annex-B stream generator (a small closed-loop encoder).
 *
 * Purpose: there is no network, no sample .h264 and no third-party encoder in the build image
 * (SURVEY.md fact 5), so tests and bench.py synthesise their inputs here.  The generator emits
 * (a) a conforming Annex-B byte stream and (b) its own reconstruction of every frame, produced by
 * an implementation of prediction / transform / deblocking written independently of both the
 * oracle (oracle/) and the product (h264decode_amd/).  Round-trip tests require
 * decoder output == generator reconstruction, bit for bit.
 *
 * This is input synthesis, not part of the decode product and not the oracle.
 */
#ifndef SG_H
#define SG_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int width, height;      /* display size; coded size is rounded up to 16, cropping signalled in the SPS */
    int frames;
    int profile_idc;        /* 66 Baseline, 77 Main, 100 High */
    int cabac;              /* entropy_coding_mode_flag */
    int qp;                 /* base QP (pic_init_qp); */
    int qp_jitter;          /* per-MB |mb_qp_delta| up to this value (0 = constant QP) */
    int idr_period;         /* 1 = all IDR; N = IDR every N frames, P in between; 0 = only the first frame is IDR */
    int slices;             /* slices per picture (split by MB rows as evenly as possible) */
    int transform8x8;       /* 0 off; 1 = High 8x8 transform + Intra8x8 enabled (needs profile 100) */
    int num_ref_frames;     /* 1..4 */
    int deblock_idc;        /* disable_deblocking_filter_idc: 0 on, 1 off, 2 on except slice edges */
    int alpha_off_div2, beta_off_div2;
    int cabac_init_idc;     /* 0..2, or -1: cycle per slice */
    int constrained_intra;  /* constrained_intra_pred_flag */
    int chroma_qp_offset;   /* chroma_qp_index_offset (second offset = same unless High: then +1 when transform8x8) */
    int pcm_permille;       /* probability (1/1000) of an I_PCM macroblock */
    int intra_in_p_permille;/* probability of an intra MB inside P pictures */
    int skip_permille;      /* probability of P_Skip */
    int sub8x8_permille;    /* probability of P_8x8 (with random sub-partitions) / 16x8 / 8x16 */
    int weighted_pred;      /* explicit weighted prediction in P slices */
    int scaling_matrix;     /* 0 flat, 1 = send default (non-flat) scaling lists in the SPS (High), 2 = coded lists in the SPS, 3 = every
                             * parameter-set pair (one per IDR picture) has a new matrix in the PPS, in turn after an SPS with a matrix (fall-back rule B
                             * of Table 7-2) and after one without (rule A); under every third PPS the 8x8 transform is off and the matrix has six lists */
    int noise;              /* amplitude of the uniform source noise */
    uint32_t seed;
    int long_start_code;    /* 1: 4-byte start codes everywhere; 0: 3-byte for non-parameter-set NALs */
    int poc_type;           /* 0, 1 or 2 */
    /* picture management stimulus (8.2.1, 8.2.4.3, 8.2.5.4); all 0 = sliding window, default lists, every picture a reference */
    int rplm;               /* 1: P slices carry random ref_pic_list_modification() commands (idc 0, 1 and, with long-term pictures, 2) */
    int mmco;               /* 1: reference P pictures carry random memory_management_control_operation scripts (1..6) */
    int idr_long_term;      /* 1: IDR pictures set long_term_reference_flag (with bframes: the long-term picture closes both lists of a B picture, 8.2.4.2.3,
                             * and is RefPicList1[0] of the B pictures between an IDR picture and the anchor after it; not with b_pyramid or field_pics) */
    int nonref_period;      /* N > 1: every N-th P picture is a non-reference picture (nal_ref_idc 0) */
    int slice_qp_delta;     /* d != 0: slice_qp_delta cycles through -d, 0, +d per slice */
    /* B pictures (Main / High): `bframes` non-reference B pictures between two anchors (display order I B B P -> coding
     * order I P B B); needs num_ref_frames >= 2 and forces pic_order_cnt_type 0 */
    int bframes;
    int direct_temporal;    /* 0: direct_spatial_mv_pred_flag = 1; 1: temporal direct */
    int weighted_bipred;    /* weighted_bipred_idc: 0 default average, 1 explicit, 2 implicit */
    int bskip_permille;     /* probability of B_Skip; B_Direct_16x16 gets half of it on top */
    int motion_x4, motion_y4; /* motion of the synthetic scene per frame in quarter samples (default 12, -8 = whole samples (3, -2));
                             * anything not a multiple of 4 makes fractional motion vectors the rule (6-tap interpolation) */
    int interlace_sps;      /* 1: frame_mbs_only_flag = 0 in the SPS (mb_adaptive_frame_field_flag = 0), every picture still a frame
                             * (field_pic_flag = 0): the syntax of a PAFF-capable stream that never uses a field picture */
    int fn_gap_period;      /* N > 0 (streams without B pictures / marking scripts): before every N-th picture after an IDR picture
                             * frame_num skips one or two values (8.2.5.2): the skipped frames enter the window as "non-existing"
                             * frames and the lists are re-ordered so that only real pictures are predicted from */
    int fn_gap_declared;    /* gaps_in_frame_num_value_allowed_flag of the SPS; 0 with fn_gap_period set = a stream that lost pictures */
    int b_pyramid;          /* with bframes >= 2: the middle B picture of a group is coded first, as a REFERENCE picture (nal_ref_idc 2);
                             * the other B pictures of the group may predict from it and take it as their co-located picture */
    /* Baseline extras (7.3.2.2, 8.2.2): slice_groups n >= 2 puts every picture's macroblocks into n slice groups by map type
     * fmo_type 0..6 (types 3..5: two groups, slice_group_change_cycle moves from picture to picture; 6: an explicit pseudo-random
     * map); `slices` then counts the slices PER GROUP.  aso: the slices of a picture leave in a shuffled order (arbitrary slice
     * order; needs more than one slice per picture to show) */
    int slice_groups, fmo_type, aso;
    /* PAFF: 1 = every frame is coded as two FIELD pictures (field_pic_flag = 1), top field first; 2 = bottom field first;
     * 3 = picture-adaptive: frame by frame either a frame picture or two field pictures, so that frames predict from
     * field-coded frames and fields from the fields of frame-coded ones.  The first field of an IDR frame is the IDR
     * picture, its second field a P or I field of the same frame_num; all other fields are P fields whose RefPicList0
     * alternates between fields of the same and of the opposite parity (8.2.4.2.5) and may start with the first field of
     * the same frame.  Forces interlace_sps; with cabac = 1 the field-coded blocks use the UNPINNED context values of sg_cabac_mn.c (ctxIdx 277..398,
     * 436..459: written down without the standard at hand); sliding-window marking (counted in frames, 8.2.5.3), list modification on field picture numbers
     * (rplm, P fields), marking scripts of operation 1 on single fields (mmco: a frame then lacks a field in later lists, and
     * a frame picture that finds no frame with both fields marked is coded as an I picture), non-reference frames
     * (nonref_period) and slice groups (a map unit is one macroblock of a field, 8.2.2.8) allowed, no long-term pictures.  bframes with field_pics 1 / 2 (not 3): every B frame is two non-reference B fields (spatial or
     * temporal direct prediction from the co-located field), their lists built from the anchors' fields by PicOrderCnt
     * (8.2.4.2.4) and the same alternation.  recon[] holds the woven frames. */
    int field_pics;
    /* d != 0: bottom_field_pic_order_in_frame_present_flag = 1 and every FRAME picture says where its bottom field sits relative to
     * its top field (delta_pic_order_cnt_bottom with pic_order_cnt_type 0, delta_pic_order_cnt[1] with type 1): BottomFieldOrderCnt =
     * TopFieldOrderCnt + d.  PicOrderCnt of a frame is the smaller of the two (8.2.1): a negative d moves every non-IDR picture d
     * earlier (IDR pictures keep 0 = Min(top, bottom): they send Max(d, 0); a negative d is taken as -1, the value of bottom-field-first material: anything lower would put the first pictures of a sequence before their IDR picture).  Ignored with pic_order_cnt_type 2. */
    int poc_bottom_delta;
    /* 1: chroma_format_idc 0 (monochrome; h264/sps.go:226-243 ChromaFormat; High profile only): no intra_chroma_pred_mode, coded_block_pattern by the
     * ChromaArrayType 0 column of Table 9-4 (CABAC: no chroma bins), no chroma residual, 256 samples per I_PCM macroblock, no chroma weights.  The
     * reconstruction carries chroma planes of 128 (what a decoder puts out for a 4:2:0 display). */
    int mono;
    /* value-range stimulus: all 0 = the streams of before, byte for byte.
     * wp_range 1: every slice with a pred_weight_table() draws its own two denominators from 0..7 and, per list entry and
     * separately for luma and chroma, a flag, a weight from -128..127 and an offset from -128..127, biased to the ends
     * (-128, -1, 0, 1, 127, 2^denom and its neighbours); weights of two lists keep -128 <= w0 + w1 <= (denom == 7 ? 127 : 128)
     * for every pair of entries (7.4.3.2).  Needs weighted_pred (P slices) / weighted_bipred 1 (B slices) to show.
     * 2: the same, and list modification puts one reference picture at two indices of RefPicList0 (P frame pictures with two or more active entries). */
    int wp_range;
    /* N > 1 (pic_order_cnt_type 0 / 1): PicOrderCnt advances by 2 * N per frame; the SPS then carries a 16-bit pic_order_cnt_lsb,
     * so that an anchor several B pictures ahead stays within MaxPicOrderCntLsb / 2 of the picture before it */
    int poc_step;
    /* mv_reach r > 0: the random candidate of the motion search comes from -r..r quarter samples (default 64), is drawn at the
     * ends of that range one time in four per component and is taken without a search one time in five; mv_margin m > 0: a block
     * may lie up to m samples outside the picture (default 24).  Vectors stay within -8192..8191 horizontally and -2048..2047
     * vertically (field pictures: -1024..1023), the range of levels 3.1 to 5.1 (Table A-1) */
    int mv_reach, mv_margin;
    /* 1: the source is a hard 0 / 255 pattern: per 16x16 region of the (moving) scene flat, stripes or checks of period 1..3 samples,
     * in luma and in both chroma planes */
    int contrast;
    /* deblocking stimulus: all 0 = the streams of before, byte for byte.
     * dbf_per_slice 1: every slice draws its own disable_deblocking_filter_idc from {0, 1, 2} and its own slice_alpha_c0_offset_div2 and
     * slice_beta_offset_div2 from -6..6 (deblock_idc, alpha_off_div2 and beta_off_div2 are then ignored) */
    int dbf_per_slice;
    /* 1: sg_last_deblock_trace() keeps, for every picture of this call, the planes before sg_deblock and the sg_dbmb table; changes nothing else */
    int trace_deblock;
    /* entropy-syntax stimulus: 0 = the streams of before, byte for byte.  1: the 16-bit range guard of sg_recon.c is on, and
     * - after every quantiser call and before the reconstruction is made from the levels, most blocks get their levels replaced by a drawn pattern
     *   (a target per block: TotalCoeff biased to 0, 1, max - 1 and max, TrailingOnes 0..3, the position of the last coefficient up to the last scan
     *   position, the zeros as one long run or as many short ones, magnitudes at the ends of the binarisations: 1, 2, 3, 14..17, 15 * 2^(s - 1) and its
     *   neighbours, "ladders" that take suffixLength to s = 0..6 and then need level_prefix 14, 15 or (High, CAVLC) 16, 2063 / 2064 and beyond), the density
     *   drawn per neighbourhood of macroblocks; a large level goes where it passes the guard alone (low QP, small LevelScale), the guard runs after the
     *   replacement and the reconstruction is made from what is left;
     * - profile_idc 66 / 77 with CAVLC: no |level| above 2063 (level_prefix <= 15, A.2); profile_idc 100 writes the escape of 9.2.2.1;
     * - one macroblock in twelve is heavy (every block full, the levels as large as their share of the guard's range allows); a macroblock of more
     *   than 3200 bits (A.3.1) is coded again with a thinner pattern, up to three times, the last time without any level;
     * - QP_Y is drawn from the whole 0..51, mb_qp_delta takes -26 and +25 and the wrapped form (QP_Y + mb_qp_delta outside 0..51) where the straight
     *   one is out of range, and a non-zero delta is preferred after a skipped, an I_PCM and a delta-less macroblock;
     * - slices get forced runs of skipped macroblocks longer than a row, and end in a skip run or in an I_PCM macroblock.
     * 2: the same without the second coding of large macroblocks.  3 is taken as 0.  Adding 4 to 1 or 2 changes no stream: sg_last_syntax() then counts
     * what the B slices contain and leaves the I and P slices out (a stream with B pictures has all three).
     * What the stream then really contains is counted by the entropy writers: sg_last_syntax(). */
    int syntax_stim;
    /* intra-prediction stimulus (8.3): both 0 = the streams of before, byte for byte, and not one more draw of the generator.
     * intra_stim 1: among the modes that sg_intra_mode_allowed() permits for a block, the one whose cell (kind, mode, the availability combination the
     * block sees) was chosen least often so far in this sg_encode() call wins, the SAD score (with its drawn jitter) breaking ties; the same for the
     * Intra16x16 and the chroma mode; among Intra4x4 / Intra8x8 / Intra16x16 the kind is drawn as before.  Slices of a picture without slice
     * groups are then split by macroblock COUNT, not by rows, so that they start in the middle of a row.  What was reached: the SG_R_IP_* counters */
    int intra_stim;
    /* 1: sg_last_intra_trace() keeps, for every picture of this call, the prediction and residual sample of every intra-predicted sample and the sg_ipmb
     * table (and what trace_deblock keeps); changes nothing else */
    int trace_intra;
    /* motion derivation (8.4.1): all three 0 = the streams of before, byte for byte, and not one more draw of the generator.
     * direct_4x4 1: the SPS carries direct_8x8_inference_flag = 0 (frame-only streams: refused together with field_pics and interlace_sps).  The
     * co-located block of a 4x4 block is then the 4x4 block at the same place (no corner substitution), direct prediction gives every 4x4 block of a
     * direct quadrant a vector of its own, and a direct quadrant counts as smaller than 8x8: no transform_size_8x8_flag follows a B_8x8 macroblock with
     * a direct quadrant nor a B_Direct_16x16 macroblock (7.3.5) */
    int direct_4x4;
    /* 1: sg_last_motion_trace() keeps, for every picture of this call, the sg_mvmb table and the sg_mvslice table; changes nothing else */
    int trace_motion;
    /* motion stimulus: 0 = the streams of before, byte for byte, and not one more draw of the generator.  1: where the generator draws the kind of an inter
     * macroblock (P: 16x16, 16x8, 8x16, 8x8; B: the mb_type 1 .. 22, partition shape and prediction modes in one), a sub_mb_type or a ref_idx, it takes the
     * candidate that was taken least often so far in this sg_encode() call, the drawn one winning among equals; a ref_idx must lie inside its list and
     * pass the reference barrier.  Skipped, direct and intra macroblocks are drawn as before.  In CAVLC P slices with more than one active reference,
     * P_8x8ref0 (mb_type 4: four indices of 0, not written) is a fifth kind, and any P_8x8 macroblock whose four indices are 0 is written that way.
     * Vectors still come from the motion search, but one partition in four takes one that changes what the blocks after it see in their neighbours --
     * the vector of its neighbour A, B or C (where that neighbour uses the list), a zero vector where its own index is 0 (the conditions of P_Skip and
     * of colZeroFlag), or a vector whose components come from -2 .. 2 (the boundary of colZeroFlag); it passes the same limits as any other. */
    int motion_stim;
    /* open groups of pictures: 0 = the streams of before, byte for byte, and not one more draw of the generator.  N > 0 (rounded up to a multiple of
     * bframes + 1, like idr_period): the anchor at every display index that is a positive multiple of N, and no IDR picture, is coded as a non-IDR I
     * picture (field_pics: two I fields).  In front of it, in its access unit, stand the SPS and the PPS again, byte for byte, and an SEI NAL unit with a
     * recovery point message (D.1.7): recovery_frame_cnt 0, exact_match_flag 1, broken_link_flag 0.  The B pictures between the anchor before and this
     * one are coded after it as for any anchor and predict across it: a decoder that starts at the anchor cannot decode them (leading pictures).
     * The reference barrier: a picture behind such an anchor in display order predicts from no picture in front of the anchor in display order, and from
     * no list entry that has a picture coded before the anchor and shown before it in front of it in the list (a decoder that started at the anchor
     * with an empty window finds the entries behind such a picture at other indices).  That restricts the choice of reference indices only -- a P macroblock is not skipped
     * where entry 0 is barred --; list sizes and orders are what the whole DPB gives.  Refused together with rplm, mmco, idr_long_term, fn_gap_period,
     * wp_range 2 (list modification) and direct_temporal (the index comes from the co-located block). */
    int open_gop_period;
    /* residual decoding (8.5): both 0 = the streams of before, byte for byte, and not one more draw of the generator.
     * trace_residual 1: sg_last_residual_trace() keeps, for every picture of this call, the prediction sample of every sample, the sg_rsmb table, the two
     * chroma offsets and the eight scaling lists (and what trace_deblock keeps); changes nothing else */
    int trace_residual;
    /* residual stimulus: 1: the 16-bit range guard of sg_recon.c is on and QP_Y is drawn from the whole 0..51 as under syntax_stim (one macroblock in two
     * takes the QP_Y its kind -- Intra4x4, Intra8x8, Intra16x16, inter -- had least often so far).  After every quantiser call (and after the pattern of
     * syntax_stim, where both are set) and before the reconstruction is made from the levels: per macroblock a target (luma coded_block_pattern, chroma
     * class) is the one its kind had least often so far in this sg_encode() call, blocks outside the target are emptied, blocks inside get levels -- what the
     * quantiser left, or one level at the scan position used least often so far (small, or as large as the guard lets it pass alone), or a level at every scan
     * position, or negative levels only; for chroma the planes that keep DC levels (class 1) or AC levels (class 2) are Cb, Cr or both in turn; in an 8x8
     * block the raster row pairs (0-1, 2-3, 4-5, 6-7) that keep coefficients are the subset taken least often, every pair of it holding a coefficient.  The
     * guard runs afterwards.  Heavy and thinned macroblocks of syntax_stim are left to it. */
    int residual_stim;
} sg_params;

void sg_default_params(sg_params *p);
/* Returns stream size in bytes (0 on failure / overflow).  recon (optional) receives every frame
 * at CODED size, I420 planar, back to back; recon_cap in bytes.  frame_sizes (optional, `frames`
 * entries) receives the byte size of each access unit. */
size_t sg_encode(const sg_params *p, uint8_t *stream, size_t stream_cap, uint8_t *recon, size_t recon_cap, uint32_t *frame_sizes);
/* source picture t of the synthetic sequence (coded size), for reference / PSNR */
void sg_source_frame(const sg_params *p, int t, uint8_t *dst);
const char *sg_last_error(void);
/* PicOrderCnt the generator intended for every picture of the last sg_encode() call (display order == coding order:
 * 2 * pictures since the last IDR / memory_management_control_operation 5).  Returns the number of pictures. */
int sg_last_pocs(int32_t *dst, int cap);
/* what the last sg_encode() call actually emitted: bit k = memory_management_control_operation k (1..6), bit 8/9/10 =
 * modification_of_pic_nums_idc 0/1/2, bit 11 = a long-term picture in an active reference list, bit 12 = non-reference
 * picture, bit 13 = slice_qp_delta != 0, bit 14 = pic_order_cnt_type 1 with delta_pic_order_cnt[0] != 0, bit 15 = a frame_num gap,
 * bit 16 = a non-IDR I picture with a recovery point SEI message (open_gop_period) */
uint32_t sg_last_features(void);
/* open_gop_period: the entry points of the last sg_encode() call, two numbers each -- the frame of recon[] (coding order) the non-IDR I picture is, and
 * the leading PICTURES that follow it (a field counts as one).  Returns the number of entry points; dst receives up to cap numbers. */
int sg_last_entries(int32_t *dst, int cap);
/* what the last sg_encode() call really reached, counted where the generator builds the prediction that goes into its
 * reconstruction (never in the motion search).  Returns the number of counters; dst receives up to cap of them. */
enum {
    SG_R_MVD_X, SG_R_MVD_Y,                       /* largest |mvd| per component (quarter samples) */
    SG_R_OUT_LEFT, SG_R_OUT_RIGHT, SG_R_OUT_TOP, SG_R_OUT_BOTTOM, /* predicted blocks whose whole (w + 5) x (h + 5) luma window lies outside the picture */
    SG_R_HALF1_CLIP0, SG_R_HALF1_CLIP255,         /* luma half samples b / h (one 6-tap filter) clipped at 0 / at 255 */
    SG_R_HALFJ_CLIP0, SG_R_HALFJ_CLIP255,         /* the centre half sample j (two filters) clipped */
    SG_R_W1_CLIP0, SG_R_W1_CLIP255,               /* explicitly weighted samples clipped, blocks with one list */
    SG_R_W2_CLIP0, SG_R_W2_CLIP255,               /* ... blocks with two lists */
    SG_R_DENOM_MASK,                              /* bit d: a block was predicted with log2 denominator d (luma or chroma) */
    SG_R_W_MIN, SG_R_W_MAX, SG_R_O_MIN, SG_R_O_MAX, /* smallest / largest explicit weight and offset of a block actually predicted */
    SG_R_NEG_WEIGHT,                              /* blocks predicted with a negative explicit weight */
    SG_R_ODD_NEG_OFFSETS,                         /* two-list blocks with o0 + o1 odd and negative */
    SG_R_TBTD_CLIPPED, SG_R_DSF_CLIPPED,          /* 8.4.1.2.3: tb or td clipped; DistScaleFactor clipped */
    SG_R_IMPLICIT_FALLBACK, SG_R_IMPLICIT_PAIRS,  /* implicit two-list blocks that fell back to 32 / 32, and those that did not */
    SG_R_IMPLICIT_W1_MIN, SG_R_IMPLICIT_W1_MAX,   /* ... smallest and largest w1 of the latter */
    SG_R_SCALING_FORMS,                           /* scaling-list forms written: the SG_SF_* bits */
    SG_R_GUARD_ZEROED,                            /* levels set to 0 because they would have left the 16-bit range of 8.5.12 */
    SG_R_REF_TWICE,                               /* wp_range 2: slices' lists with one picture at two indices */
    /* deblocking (8.7), counted in sg_deblock / edge_line on the final reconstruction of every picture.  A "line" is the samples across an edge at
     * one position; "clipped" means that the clip changed the value */
    SG_R_DB_FILT_LUMA,                            /* [4]: luma lines filtered with bS 1, 2, 3, 4 */
    SG_R_DB_REJ_LUMA = SG_R_DB_FILT_LUMA + 4,     /* [4]: luma lines with bS 1 .. 4 that one of the three tests of 8.7.2.2 left alone */
    SG_R_DB_FILT_CHROMA = SG_R_DB_REJ_LUMA + 4,   /* [4], [4]: the same for lines of Cb and Cr */
    SG_R_DB_REJ_CHROMA = SG_R_DB_FILT_CHROMA + 4,
    SG_R_DB_REJ_ALPHA = SG_R_DB_REJ_CHROMA + 4, SG_R_DB_REJ_BETA_P, SG_R_DB_REJ_BETA_Q, /* the first test that failed: |p0 - q0|, |p1 - p0|, |q1 - q0| */
    SG_R_DB_APAQ,                                 /* [4]: filtered luma lines with bS < 4 by ap * 2 + aq */
    SG_R_DB_DELTA_LO = SG_R_DB_APAQ + 4, SG_R_DB_DELTA_HI, SG_R_DB_DELTA_IN, /* bS < 4: delta clipped at -tc, at +tc, not clipped */
    SG_R_DB_P1_LO, SG_R_DB_P1_HI, SG_R_DB_Q1_LO, SG_R_DB_Q1_HI, /* the p1 / q1 correction clipped at -tC0 / at +tC0 */
    SG_R_DB_P0_AT0, SG_R_DB_P0_AT255, SG_R_DB_Q0_AT0, SG_R_DB_Q0_AT255, /* p0 + delta / q0 - delta clipped at 0 / at 255 */
    SG_R_DB_TC0_ZERO, SG_R_DB_TC0_ZERO_AP,        /* filtered luma lines with bS < 4 and tC0 = 0; those of them with ap set */
    SG_R_DB_BS4_SMALL, SG_R_DB_BS4_NOT_SMALL,     /* filtered luma lines with bS 4: |p0 - q0| < (alpha >> 2) + 2 or not */
    SG_R_DB_BS4_STRONG,                           /* [4]: ... by (strong filter on the p side) * 2 + (on the q side) */
    SG_R_DB_IA_MIN = SG_R_DB_BS4_STRONG + 4, SG_R_DB_IA_MAX, SG_R_DB_IB_MIN, SG_R_DB_IB_MAX, /* indexA / indexB of filtered edges */
    SG_R_DB_IA_CLIP0, SG_R_DB_IA_CLIP51,          /* edges (per plane) whose qPav + filterOffsetA lay below 0 / above 51 */
    SG_R_DB_QP_ODD,                               /* edges with qp_p != qp_q and an odd sum */
    SG_R_DB_PCM_EDGE,                             /* edges with an I_PCM macroblock on either side */
    SG_R_DB_CBCR_ALPHA,                           /* edges where Cb and Cr get different alpha */
    SG_R_DB_PAIR_DIFFERS,                         /* luma lines 2k and 2k + 1 of a segment of which one is filtered and one is not */
    SG_R_DB_CBCR_PAIR_DIFFERS,                    /* the Cb and the Cr line at one position of which one is filtered and one is not */
    SG_R_DB_SEG_NONE,                             /* segments (per plane) with bS > 0 and no line filtered */
    SG_R_DB_FIELD_BS3,                            /* field pictures: segments with bS 3 on a horizontal macroblock edge */
    SG_R_DB_B_BS1_CROSSED, SG_R_DB_B_BS1_STRAIGHT, SG_R_DB_B_BS0_CROSSED, /* two vectors on both sides: bS 1 although the pictures pair crossed /
                                                   * straight; bS 0 through the crossed pairing */
    SG_R_DB_SLICE_OFFSETS,                        /* filtered edges between two slices with different filter offsets */
    SG_R_DB_IDC1_MODIFIED,                        /* edges that changed a sample of a macroblock whose own slice has disable_deblocking_filter_idc 1 */
    SG_R_DB_IDC2_SKIPPED,                         /* macroblock edges left alone only because of idc 2 (the neighbour is in another slice) */
    /* intra prediction (8.3), counted in encode_intra on the mode finally chosen.  An availability combination is left | top << 1 | topleft << 2 |
     * topright << 3 as the BLOCK sees it (Intra16x16 and chroma: as the macroblock sees it) */
    SG_R_IP_AV4,                                  /* [9]: per Intra4x4PredMode, bit c: a block with combination c was predicted in that mode */
    SG_R_IP_AV8 = SG_R_IP_AV4 + 9,                /* [9]: the same per Intra8x8PredMode */
    SG_R_IP_AV16 = SG_R_IP_AV8 + 9,               /* [4]: per Intra16x16PredMode */
    SG_R_IP_AVC = SG_R_IP_AV16 + 4,               /* [4]: per intra_chroma_pred_mode (not counted in monochrome streams) */
    SG_R_IP_TR4 = SG_R_IP_AVC + 4,                /* [16]: per luma4x4BlkIdx, modes 3 and 7: bit 0 real samples above and to the right were read, bit 1 they were substituted */
    SG_R_IP_TR8 = SG_R_IP_TR4 + 16,               /* [4]: the same per luma8x8BlkIdx */
    SG_R_IP_PLANE16_LO = SG_R_IP_TR8 + 4, SG_R_IP_PLANE16_HI, /* samples of an Intra16x16 plane prediction below 0 / above 255 before the clip */
    SG_R_IP_PLANEC_LO, SG_R_IP_PLANEC_HI,         /* ... of a chroma plane prediction (Cb and Cr) */
    SG_R_IP_REC_LUMA_AT0, SG_R_IP_REC_LUMA_AT255, /* luma samples of intra-predicted macroblocks whose prediction + residual lay below 0 / above 255 */
    SG_R_IP_REC_CHROMA_AT0, SG_R_IP_REC_CHROMA_AT255,
    SG_R_IP_FROM_INTER,                           /* bit 0 left, 1 top, 2 topleft, 3 topright: a block's mode read samples of that direction (8.3; Intra8x8: what
                                                   * 8.3.2.2.1 reads for them included) and they belong to an inter macroblock */
    SG_R_IP_FROM_PCM,                             /* ... to an I_PCM macroblock */
    SG_R_IP_F8_TOP_NO_TL, SG_R_IP_F8_LEFT_NO_TL,  /* Intra8x8 blocks whose mode reads the row above / the column to the left, with p'[0,-1] / p'[-1,0] filtered without p[-1,-1] */
    SG_R_COUNT
};
enum {
    SG_SF_ABSENT_FIRST = 1,   /* list 0, 3, 6 or 7 absent (falls back to a Default list or to the SPS) */
    SG_SF_ABSENT_NEXT = 2,    /* list 1, 2, 4 or 5 absent (takes the list before it) */
    SG_SF_USE_DEFAULT = 4, SG_SF_CUT_SHORT = 8, SG_SF_WRAP = 16, SG_SF_ENTRY_1 = 32, SG_SF_ENTRY_255 = 64, SG_SF_FULL = 128,
    SG_SF_SPS_MATRIX = 256, SG_SF_PPS_RULE_A = 512, SG_SF_PPS_RULE_B = 1024, SG_SF_PPS_SIX_LISTS = 2048
};
int sg_last_ranges(int32_t *dst, int cap);
/* what the entropy writers of the last sg_encode() call of this thread wrote (cavlc_block, cabac_block, the mb_qp_delta / coded_block_pattern / skip /
 * mb_type writers of sg_enc.c; never counted where the stimulus draws).  Counted for every stream, with or without syntax_stim.  A set of its own
 * beside SG_R_*: the entries are mostly bitmaps, one 32-bit word per table row.  Returns the number of words; dst receives up to cap of them. */
enum {
    SG_S_TOKEN,                                   /* [5][3]: coeff_token table (nC 0-1, 2-3, 4-7, 8+, chroma DC), bit 4 * TotalCoeff + TrailingOnes over three words */
    SG_S_NC_ONE = SG_S_TOKEN + 15, SG_S_NC_NONE,  /* blocks whose nC came from one neighbour / from none (nC = 0) */
    SG_S_TZ16,                                    /* [15]: total_zeros of blocks of 16 coefficients: word tzVlcIndex - 1, bit total_zeros */
    SG_S_TZ15 = SG_S_TZ16 + 15,                   /* [15]: the same for AC blocks of 15 coefficients */
    SG_S_TZC = SG_S_TZ15 + 15,                    /* [3]: chroma DC */
    SG_S_RUN = SG_S_TZC + 3,                      /* [7]: run_before: word Min(zerosLeft, 7) - 1, bit run_before (0..14 in the last word) */
    SG_S_PREFIX_MAX = SG_S_RUN + 7,               /* largest level_prefix */
    SG_S_P14_SL, SG_S_P15_SL, SG_S_P16_SL,        /* bit s: level_prefix 14 / 15 / 16 and above written at suffixLength s */
    SG_S_LEVEL_MAX,                               /* largest |level| of a CAVLC block */
    SG_S_START_SL1,                               /* blocks that start at suffixLength 1 (TotalCoeff > 10, TrailingOnes < 3) */
    SG_S_CAVLC_8X8_FULL,                          /* CAVLC 8x8 blocks (four interleaved 4x4 blocks) with 16 coefficients in every part */
    SG_S_EGK_MAX,                                 /* CABAC: largest k reached by the Exp-Golomb suffix of coeff_abs_level_minus1 */
    SG_S_LEVEL_MAX_CABAC,                         /* largest |level| of a CABAC block */
    SG_S_CAT_BLOCKS,                              /* [6]: CABAC blocks with a coefficient, per ctxBlockCat 0..5 */
    SG_S_LAST_AT_END = SG_S_CAT_BLOCKS + 6,       /* [6]: ... whose last coefficient is at the last scan position (no last_significant_coeff_flag for it) */
    SG_S_ALL_NONZERO = SG_S_LAST_AT_END + 6,      /* [6]: ... with every coefficient non-zero */
    SG_S_INC0_SAT = SG_S_ALL_NONZERO + 6,         /* bit cat: ctxIdxInc of the first bin of coeff_abs_level_minus1 reached 4 (three or more levels of 1 before) */
    SG_S_GT1_SAT,                                 /* bit cat: the count of levels above 1 reached its cap in the ctxIdxInc of the later bins (4; 3 for chroma DC) */
    SG_S_CBF_INC,                                 /* [5]: per ctxBlockCat 0..4, bit ctxIdxInc of coded_block_flag */
    SG_S_CBF_UNAVAIL_INTRA = SG_S_CBF_INC + 5, SG_S_CBF_UNAVAIL_INTER, /* coded_block_flag increments with an unavailable neighbour, in intra / inter macroblocks */
    SG_S_DQP_MIN, SG_S_DQP_MAX,                   /* smallest / largest mb_qp_delta written */
    SG_S_DQP_WRAP_UP, SG_S_DQP_WRAP_DOWN,         /* QP_Y,PRED + mb_qp_delta above 51 / below 0 */
    SG_S_QPY_MIN, SG_S_QPY_MAX,                   /* smallest / largest QP_Y after an mb_qp_delta */
    SG_S_DQP_AFTER_SKIP, SG_S_DQP_AFTER_PCM, SG_S_DQP_AFTER_NODELTA, /* non-zero mb_qp_delta directly after a skipped / an I_PCM / a macroblock without mb_qp_delta */
    SG_S_QPC_CLIP0, SG_S_QPC_CLIP51,              /* macroblocks with an mb_qp_delta whose QP_Y + chroma_qp_index_offset lay below 0 / above 51 */
    SG_S_CBP_INTRA, SG_S_CBP_INTER = SG_S_CBP_INTRA + 2, /* [2], [2]: bit coded_block_pattern (0..47) over two words */
    SG_S_MBTYPE_I = SG_S_CBP_INTER + 2,           /* bit mb_type (0..25) of macroblocks of I slices */
    SG_S_REM4, SG_S_REM8,                         /* bit rem_intra4x4_pred_mode / rem_intra8x8_pred_mode 0..7, bit 8: the predicted mode was used */
    SG_S_SKIP_RUN_MAX,                            /* longest run of skipped macroblocks inside a slice (mb_skip_run, or mb_skip_flags in a row) */
    SG_S_END_IN_SKIP, SG_S_END_IN_PCM,            /* slices whose last macroblock is skipped / I_PCM */
    SG_S_MB_BITS_MAX,                             /* the largest macroblock, in bits (CABAC: bits the arithmetic coder put out for it) */
    SG_S_THINNED,                                 /* macroblocks coded again with a thinner pattern because they had more than 3200 bits */
    SG_S_COUNT
};
int sg_last_syntax(int32_t *dst, int cap);
/* what the last sg_encode() call of this thread did about motion (8.4.1): a third set beside SG_R_* and SG_S_*, counted for every stream.  The derivation
 * counters are counted where the generator builds the predictor that goes into the stream (mv_pred / mv_pred_l, skip_mv, b_direct; never in the motion
 * search), the syntax ones where the entropy writers write.  "slot" = 0: list 0 of a P slice, 1 / 2: list 0 / 1 of a B slice.  A direct block counts
 * once per 4x4 block it covers.  Returns the number of words; dst receives up to cap of them. */
enum {
    SG_M_PRED,                                    /* [3 slots][5 shapes: median, 16x8 upper, lower, 8x16 left, right][8 rules: directional hit, only A available,
                                                   * single match at A, at B, at C, median with 0, 2, 3 matches]: predictors of coded partitions and of P_Skip */
    SG_M_CSRC = SG_M_PRED + 120,                  /* [3 slots][3]: neighbour C of those predictors was C itself, D in its place, neither */
    SG_M_PSKIP = SG_M_CSRC + 9,                   /* [6]: P_Skip: zero because A is missing, B is missing, A is still (index 0, zero vector), B is still; predicted and non-zero, and zero */
    SG_M_SD_REF = SG_M_PSKIP + 6,                 /* [2 lists][4]: spatial direct, per macroblock derivation: the index came from A, B, C, none (negative) */
    SG_M_SD_BOTHNEG = SG_M_SD_REF + 8,            /* ... both lists negative: index 0 on both */
    SG_M_SD_OUT,                                  /* [2 lists][4]: per 4x4 block: list not used; zeroed by colZeroFlag; kept with index 0; kept with a positive index although the flag is set */
    SG_M_COL = SG_M_SD_OUT + 8,                   /* [3]: per 4x4 block of a direct block: the co-located block was intra, used list 0, used list 1 only */
    SG_M_TD_REF = SG_M_COL + 3,                   /* [2]: temporal direct, per 4x4 block: refIdxL0 0, above 0 */
    SG_M_TD_LONG = SG_M_TD_REF + 2,               /* ... RefPicList0[refIdxL0] long-term: vector copied, list 1 zero */
    SG_M_TD_NEG_REMAINDER,                        /* ... a negative component of mvCol whose product with DistScaleFactor, plus 128, is no multiple of 256 */
    SG_M_MBTYPE_P, SG_M_MBTYPE_B,                 /* bit mb_type (0..4 / 0..22) written in P / B slices (inter types only) */
    SG_M_SUBTYPE_P, SG_M_SUBTYPE_B,               /* bit sub_mb_type (0..3 / 0..12) */
    SG_M_REF_INC,                                 /* CABAC: bit ctxIdxInc 0..3 of the first bin of ref_idx */
    SG_M_REF_GE3,                                 /* ref_idx values of at least 3 written (CABAC or CAVLC) */
    SG_M_REF_DIRECT_NB,                           /* CABAC: ref_idx whose neighbour A or B is a direct or skipped block of a B slice (counted as index 0) */
    SG_M_REF_TE1, SG_M_REF_UE,                    /* CAVLC: ref_idx as the one-bit form of te() / as ue() */
    SG_M_MVD_BAND,                                /* [2 components][3]: CABAC: mvd whose context sum was below 3, 3 .. 32, above 32 */
    SG_M_MVD_SUFFIX = SG_M_MVD_BAND + 6,          /* CABAC: |mvd| of 9 and above (prefix of nine ones and an Exp-Golomb suffix) */
    SG_M_SKIP_INC_P, SG_M_SKIP_INC_B,             /* CABAC: bit ctxIdxInc 0..2 of mb_skip_flag in P / B slices */
    SG_M_BTYPE_INC,                               /* CABAC: bit ctxIdxInc 0..2 of the first bin of a B mb_type */
    SG_M_GEO,                                     /* [41 partition positions][5]: where neighbour C of a counted predictor lies: inside the macroblock and decoded, inside and
                                                   * not yet, in the macroblock above (there), above right (there), nowhere that is there.  Positions: 0 16x16, 1 / 2 16x8,
                                                   * 3 / 4 8x16, 5 + q 8x8, 9 + 2 q + k 8x4, 17 + 2 q + k 4x8, 25 + 4 q + k 4x4 (q quadrant, k partition of it) */
    SG_M_GEO_D = SG_M_GEO + 205,                  /* [41]: ... D stood in for C */
    SG_M_NOLIST = SG_M_GEO_D + 41,                /* [5]: a neighbour (A, B, or what serves as C) of a counted predictor is an available inter partition that does not use the
                                                   * list: it lies inside the macroblock, in macroblock A, B, C, D */
    SG_M_DIRECT_NB = SG_M_NOLIST + 5,             /* [2]: ... is a direct quadrant of the same macroblock (and uses the list): spatial, temporal */
    SG_M_SD_COL = SG_M_DIRECT_NB + 2,             /* [2]: spatial direct, per 4x4 block: RefPicList1[0] short-term, long-term */
    SG_M_SD_REFCOL = SG_M_SD_COL + 2,             /* [2]: ... the co-located block is not intra and refIdxCol is 0, above 0 */
    SG_M_SD_MVCOL = SG_M_SD_REFCOL + 2,           /* [2 components][5]: ... short-term, refIdxCol 0, the other component in -1 .. 1, and this one is -2, -1, 0, 1, 2 */
    SG_M_COL_CORNER = SG_M_SD_MVCOL + 10,         /* direct quadrants (inference on) whose co-located corner block has another vector than the first block of its quadrant */
    SG_M_COL_FOUR,                                /* direct quadrants (inference off) with four different co-located vectors */
    SG_M_TD_MB16, SG_M_TD_QUADRANT,               /* temporal direct derivations for a whole macroblock (B_Skip, B_Direct_16x16) / for direct quadrants of B_8x8 */
    SG_M_COUNT
};
int sg_last_motion(int32_t *dst, int cap);
/* the bits of one CAVLC coefficient level as cavlc_block() writes it (see sg_put_cavlc_level in sg_int.h): returns their number, or -1; bits receives them
 * from the first one down, in the low end of the word */
int sg_cavlc_level_bits(int level, int suffix_len, int minus2, int escape16, uint64_t *bits);
/* sg_params::trace_deblock: the pictures of the last sg_encode() call of this thread, in coding order.  Returns their number; for picture
 * `index` info receives {width, height (of the picture: a field has half the frame's rows), macroblock columns, macroblock rows, field (0 frame,
 * 1 top, 2 bottom), mono, the frame of recon[] the picture belongs to, sizeof(sg_dbmb)}, before / after the picture's I420 planes before and
 * after sg_deblock, mbs its sg_dbmb table (each optional, each with its capacity in bytes) */
int sg_last_deblock_trace(int index, int32_t info[8], uint8_t *before, uint8_t *after, size_t planes_cap, void *mbs, size_t mbs_cap);
/* sg_params::trace_intra: the same pictures (sg_last_deblock_trace() serves them too).  info receives {width, height, macroblock columns, macroblock
 * rows, field, mono, frame, sizeof(sg_ipmb), constrained_intra_pred_flag}; pred (bytes) / res (int16_t) the picture's I420 planes of prediction and
 * residual samples, 0 where a sample was not intra-predicted, planes_cap counted in samples; mbs its sg_ipmb table */
typedef struct {
    uint8_t kind;        /* 0 inter (skipped included), 1 Intra4x4, 2 Intra8x8, 3 Intra16x16, 4 I_PCM */
    uint8_t i16mode, chroma_mode, pad;
    int8_t ipm[16];      /* Intra4x4PredMode / Intra8x8PredMode of the 4x4 block at raster position 4 * row + column */
    uint16_t slice_id, pad2;
} sg_ipmb;
int sg_last_intra_trace(int index, int32_t info[9], uint8_t *pred, int16_t *res, size_t planes_cap, void *mbs, size_t mbs_cap);
/* sg_params::trace_motion: the pictures of the last sg_encode() call of this thread, in coding order: what a derivation of 8.4.1 starts from (the syntax
 * as written, nothing taken from the predictor) and what it must arrive at (the final vectors and indices).  Returns the number of pictures; for picture
 * `index` info receives {macroblock columns, macroblock rows, field (0 frame, 1 top, 2 bottom), the frame of recon[] the picture belongs to, the
 * picture's identity (the numbers of sg_mvslice::pic), slices, sizeof(sg_mvmb), sizeof(sg_mvslice)}, mbs its sg_mvmb table in macroblock address order,
 * slices its sg_mvslice table in the order the slices were sent (each optional, each with its capacity in bytes) */
typedef struct {
    uint8_t kind;        /* 0 intra, 1 16x16, 2 16x8, 3 8x16, 4 8x8, 5 P_Skip, 6 B_Direct_16x16, 7 B_Skip */
    int8_t raw;          /* mb_type as written (per slice type: Table 7-13 / 7-14; P_8x8ref0 = 4); -1: none written (skipped) or intra */
    uint8_t sub[4];      /* sub_mb_type as written (kind 4) */
    uint8_t direct8;     /* bit q: quadrant q is predicted in direct mode */
    uint8_t pad;
    uint16_t slice;      /* ordinal of the macroblock's slice in sg_mvslice order */
    int8_t ref_idx[2][4];   /* per list and quadrant: ref_idx as written (or 0 where a single active entry leaves nothing to write); -1: none for that quadrant */
    int16_t mvd[2][16][2];  /* per list: signed mvd (x, y) as written, at the 4x4 block (4 * row + column) of the partition's upper left corner; 0 elsewhere */
    int16_t mv[2][16][2];   /* the thing to be checked: final vector per list and 4x4 block (0 where the list is not used) */
    int8_t ref[2][4];       /* ... and final reference index per list and quadrant (-1: the list is not used; intra: -1) */
} sg_mvmb;
typedef struct {
    int32_t type;            /* 0 P, 1 B, 2 I */
    int32_t direct_spatial;  /* direct_spatial_mv_pred_flag (B slices) */
    int32_t cur_poc;         /* PicOrderCnt(CurrPic) */
    int32_t first_mb, count; /* the slice's first macroblock address and its number of macroblocks */
    int32_t nref[2];         /* active entries of RefPicList0 / RefPicList1 */
    int32_t pic[2][4], poc[2][4], long_term[2][4]; /* the entries: picture identity, PicOrderCnt, 1 for a long-term picture */
    int32_t col_index;       /* B slices: the index (in this trace) of the picture that is RefPicList1[0]; -1: not traced */
} sg_mvslice; /* (four entries per list and 512 slices per picture are the generator's own limits: it builds no longer list and sends no more slices) */
int sg_last_motion_trace(int index, int32_t info[8], void *mbs, size_t mbs_cap, void *slices, size_t slices_cap);
/* sg_params::trace_residual: the same pictures as sg_last_deblock_trace() (which serves them too): what 8.5 starts from.  info receives {width, height,
 * macroblock columns, macroblock rows, field, mono, frame, sizeof(sg_rsmb), chroma_qp_index_offset, second_chroma_qp_index_offset}; pred the picture's I420
 * planes of prediction samples (inter: after weighting; I_PCM: 0), planes_cap in bytes; mbs its sg_rsmb table; lists the scaling lists in force, in the
 * order of their syntax elements after the fall-back rules: six of 16 entries, then two of 64 (224 bytes; sixteens without a matrix) */
typedef struct {
    uint8_t kind;        /* 0 skipped (P_Skip, B_Skip), 1 inter, 2 Intra4x4, 3 Intra8x8, 4 Intra16x16, 5 I_PCM */
    uint8_t t8x8;        /* transform_size_8x8_flag */
    uint8_t cbp;         /* coded_block_pattern: luma | chroma << 4 (Intra16x16: what mb_type implies; skipped and I_PCM: 0) */
    uint8_t qp;          /* QP_Y in force (skipped, I_PCM and delta-less macroblocks: the value carried over) */
    uint16_t slice;
    uint8_t slice_qp, pad; /* SliceQP_Y of the macroblock's slice */
    int32_t luma[16][16];   /* the levels as written, in scan order: per 4x4 block in coding order (luma4x4BlkIdx); Intra16x16: [..][0] is 0, 1..15 the AC
                             * levels; with the 8x8 transform the same 256 numbers are four blocks of 64 */
    int32_t dc16[16];       /* Intra16x16 DC */
    int32_t cdc[2][4];      /* chroma DC */
    int32_t cac[2][4][15];  /* chroma AC */
    uint8_t pcm[384];       /* I_PCM: the samples as written (256 luma, 64 Cb, 64 Cr) */
} sg_rsmb;
int sg_last_residual_trace(int index, int32_t info[10], uint8_t *pred, size_t planes_cap, void *mbs, size_t mbs_cap, uint8_t lists[224]);

#ifdef __cplusplus
}
#endif
#endif
