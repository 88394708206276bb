"""Recipes of tests/test_value_ranges.py: generator streams that take inter prediction, the vector syntax and the scaling
lists to the ends of their value ranges (streamgen's wp_range, poc_step, mv_reach / mv_margin, contrast, scaling_matrix 2 / 3),
and what streamgen.last_ranges() must report for each of them.

The conditions are not measurements: the seeds were chosen on the CPU until the generator alone met them, and the CPU test
asserts them, so that a change to the generator cannot empty a recipe without a test failing."""

SMALL = dict(idr_period=0, frames=6)

# family -> recipes.  Pictures are 48x32 .. 96x80 (whole-window-outside blocks are common in small pictures), except the two
# far-vector recipes: 208x48 (13 macroblock columns) for the horizontal reach and 48x208 for the vertical one.
WEIGHTED = {
    "wp1_p_cavlc": dict(SMALL, width=80, height=48, profile_idc=77, cabac=0, weighted_pred=1, wp_range=1, num_ref_frames=3, slices=3, seed=100),
    "wp2_p_cabac": dict(SMALL, width=64, height=48, frames=7, profile_idc=77, cabac=1, weighted_pred=1, wp_range=2, num_ref_frames=4, slices=3, seed=21),
    "wp2_p_cavlc_2refs": dict(SMALL, width=48, height=48, frames=7, profile_idc=100, cabac=0, transform8x8=1, weighted_pred=1, wp_range=2, num_ref_frames=2,
                              slices=3, sub8x8_permille=300, seed=22),
    "wp1_b_spatial_cabac": dict(SMALL, width=64, height=64, frames=7, profile_idc=77, cabac=1, weighted_pred=1, weighted_bipred=1, wp_range=1, bframes=2,
                                num_ref_frames=3, slices=2, seed=3),
    "wp1_b_temporal_cavlc": dict(SMALL, width=64, height=64, frames=7, profile_idc=77, cabac=0, weighted_pred=1, weighted_bipred=1, wp_range=1, bframes=2,
                                 num_ref_frames=3, direct_temporal=1, slices=2, seed=4),
    "wp2_b_pyramid_cabac": dict(SMALL, width=64, height=48, frames=9, profile_idc=77, cabac=1, weighted_pred=1, weighted_bipred=1, wp_range=2, bframes=3,
                                b_pyramid=1, slices=2, seed=23),
    "wp1_field_cavlc": dict(SMALL, width=64, height=64, frames=5, profile_idc=77, cabac=0, weighted_pred=1, wp_range=1, field_pics=1, num_ref_frames=3,
                            slices=2, seed=5),
    "wp1_paff_cabac": dict(SMALL, width=64, height=64, profile_idc=77, cabac=1, weighted_pred=1, wp_range=1, field_pics=3, num_ref_frames=3, slices=2, seed=6),
    "wp1_field_b_cavlc": dict(SMALL, width=48, height=64, frames=7, profile_idc=77, cabac=0, weighted_pred=1, weighted_bipred=1, wp_range=1, field_pics=2,
                              bframes=2, num_ref_frames=2, slices=2, seed=8),
    "wp1_mono_b_cabac": dict(SMALL, width=64, height=48, frames=7, profile_idc=100, mono=1, cabac=1, weighted_pred=1, weighted_bipred=1, wp_range=1, bframes=1,
                             num_ref_frames=2, slices=3, seed=7),
}
POC = {
    "poc20_b2_spatial": dict(SMALL, width=96, height=64, frames=13, profile_idc=77, cabac=1, weighted_bipred=2, poc_step=20, bframes=2, num_ref_frames=3, seed=103),
    "poc31_b3_pyramid_temporal": dict(SMALL, width=96, height=64, frames=13, profile_idc=77, cabac=0, weighted_bipred=2, poc_step=31, bframes=3, b_pyramid=1,
                                      num_ref_frames=4, direct_temporal=1, seed=9),
    "poc20_b2_temporal_4refs": dict(SMALL, width=96, height=64, frames=13, profile_idc=100, cabac=1, transform8x8=1, weighted_bipred=2, poc_step=20, bframes=2,
                                    num_ref_frames=4, direct_temporal=1, seed=101),
}
# Field pictures: the two fields of a frame are one count apart, and td = +-1 against a tb of a whole group is the only way to the clip of
# DistScaleFactor (frame pictures have |td| >= 2 * poc_step, and |tb * tx| / 64 stays below 1024 once |td| > 32).  Such a pair always
# falls back; a pair with w1 outside 0..64 that does not is left to the frame recipes above.
POC_FIELD = {
    "poc20_field_b": dict(SMALL, width=64, height=64, frames=10, profile_idc=77, cabac=0, weighted_bipred=2, poc_step=20, field_pics=1, bframes=3,
                          num_ref_frames=2, seed=2),
}
VECTORS_FAR = {
    "mv_far_wide_cabac_p": dict(SMALL, width=208, height=48, frames=4, profile_idc=77, cabac=1, mv_reach=8000, mv_margin=2000, num_ref_frames=2, seed=10),
    "mv_far_tall_cavlc_sub8x8": dict(SMALL, width=48, height=208, frames=4, profile_idc=77, cabac=0, mv_reach=8000, mv_margin=2000, sub8x8_permille=400,
                                     num_ref_frames=2, seed=11),
}
VECTORS = dict(VECTORS_FAR, **{
    "mv_mid_b_temporal_cabac": dict(SMALL, width=96, height=80, frames=7, profile_idc=77, cabac=1, mv_reach=2000, mv_margin=500, bframes=2, direct_temporal=1,
                                    num_ref_frames=3, seed=12),
    "mv_mid_field_cavlc": dict(SMALL, width=96, height=64, frames=4, profile_idc=77, cabac=0, mv_reach=2000, mv_margin=500, field_pics=1, num_ref_frames=2,
                               sub8x8_permille=300, seed=13),
    "mv_far_field_b_cabac": dict(SMALL, width=80, height=64, frames=5, profile_idc=77, cabac=1, mv_reach=8000, mv_margin=2000, field_pics=2, bframes=1,
                                 num_ref_frames=2, seed=14),
})
CONTRAST = {
    "contrast_qp4_soft": dict(SMALL, width=64, height=48, frames=4, profile_idc=77, cabac=1, contrast=1, qp=4, motion_x4=5, motion_y4=-3, noise=0,
                              alpha_off_div2=6, beta_off_div2=6, seed=14),
    "contrast_qp4_sharp": dict(SMALL, width=64, height=48, frames=4, profile_idc=100, cabac=0, transform8x8=1, contrast=1, qp=4, motion_x4=-7, motion_y4=2,
                               noise=0, alpha_off_div2=-6, beta_off_div2=-6, seed=15),
    "contrast_qp51_soft_b": dict(SMALL, width=64, height=48, frames=5, profile_idc=77, cabac=1, contrast=1, qp=51, motion_x4=6, motion_y4=7, bframes=1,
                                 num_ref_frames=2, alpha_off_div2=6, beta_off_div2=6, seed=16),
    "contrast_qp51_sharp": dict(SMALL, width=64, height=48, frames=4, profile_idc=77, cabac=0, contrast=1, qp=51, motion_x4=3, motion_y4=-5,
                                alpha_off_div2=-6, beta_off_div2=-6, sub8x8_permille=300, seed=17),
}
SCALING = {
    "sm2_intra_8x8": dict(width=64, height=48, frames=3, idr_period=1, profile_idc=100, cabac=1, transform8x8=1, scaling_matrix=2, seed=100),
    "sm2_p_4x4_only": dict(SMALL, width=64, height=48, frames=4, profile_idc=100, cabac=0, transform8x8=0, scaling_matrix=2, seed=104),
    "sm3_p_cabac": dict(width=64, height=48, frames=8, idr_period=2, profile_idc=100, cabac=1, transform8x8=1, scaling_matrix=3, num_ref_frames=2, seed=26),
    "sm3_b_cavlc": dict(width=64, height=48, frames=12, idr_period=4, profile_idc=100, cabac=0, transform8x8=1, scaling_matrix=3, bframes=1, num_ref_frames=2,
                        seed=27),
    "sm3_field": dict(width=64, height=64, frames=6, idr_period=2, profile_idc=100, cabac=0, transform8x8=1, scaling_matrix=3, field_pics=1, num_ref_frames=2,
                      seed=28),
    "sm3_mono_qp51": dict(width=64, height=48, frames=6, idr_period=2, profile_idc=100, cabac=1, transform8x8=1, scaling_matrix=3, mono=1, qp=51, seed=29),
    "sm3_4x4_only_qp0": dict(width=48, height=32, frames=6, idr_period=2, profile_idc=100, cabac=1, transform8x8=0, scaling_matrix=3, qp=0, noise=60, seed=31),
}
ALL_AT_ONCE = {
    "everything": dict(width=96, height=80, frames=10, idr_period=5, profile_idc=100, cabac=1, transform8x8=1, scaling_matrix=3, weighted_pred=1,
                       weighted_bipred=1, wp_range=2, poc_step=31, mv_reach=2000, mv_margin=500, contrast=1, qp=10, motion_x4=5, motion_y4=-7, bframes=2,
                       num_ref_frames=3, slices=2, sub8x8_permille=300, seed=40),
    "everything_implicit_cavlc": dict(width=96, height=80, frames=10, idr_period=5, profile_idc=100, cabac=0, transform8x8=1, scaling_matrix=3, weighted_pred=1,
                                      weighted_bipred=2, wp_range=2, poc_step=31, mv_reach=2000, mv_margin=500, contrast=1, qp=10, motion_x4=5, motion_y4=-7,
                                      bframes=3, b_pyramid=1, slices=2, sub8x8_permille=300, seed=41),
}
RECIPES = {}
for _family in (WEIGHTED, POC, POC_FIELD, VECTORS, CONTRAST, SCALING, ALL_AT_ONCE):
    RECIPES.update(_family)


def pictures_of(kw):
    return kw["frames"] * (2 if kw.get("field_pics") else 1)


def decoder_cfg(kw):
    """field-coded blocks under CABAC use the unpinned context values: the product decodes them only when told to"""
    return dict(allow_unpinned_field_cabac=1) if kw.get("field_pics") and kw.get("cabac") else {}


def _popcount(v):
    return bin(v).count("1")


def unmet(name, r, forms):
    """The conditions of recipe `name` that the counters r = streamgen.last_ranges() do not meet (an empty list: all met).
    forms = streamgen.SCALING_FORMS."""
    kw, bad = RECIPES[name], []

    def need(cond, what):
        if not cond:
            bad.append(what)
    if name in WEIGHTED or name in ALL_AT_ONCE and kw["weighted_bipred"] == 1:
        need(r["denom_mask"] & 1 and r["denom_mask"] & 128 and _popcount(r["denom_mask"] & 126) >= 4, "denominators 0, 7 and four others")
        need(r["neg_weight"] > 0 and r["w_min"] < 0, "a block with a negative weight")
        need(r["w1_clip0"] > 0 and r["w1_clip255"] > 0, "one-list blocks clipped at 0 and at 255")
        if kw.get("bframes"):
            need(r["w2_clip0"] > 0 and r["w2_clip255"] > 0, "two-list blocks clipped at 0 and at 255")
            need(r["odd_neg_offsets"] > 0, "o0 + o1 odd and negative")
        if kw["wp_range"] == 2:
            need(r["ref_twice"] > 0, "a picture at two indices of a list")
    if name in VECTORS or name in ALL_AT_ONCE:
        need(r["mvd_max_x"] > 255 and r["mvd_max_y"] > 255, "|mvd| above 255 in both components")
        need(all(r["outside_" + s] > 0 for s in ("left", "right", "top", "bottom")), "whole windows outside on all four sides")
    if name in VECTORS_FAR:
        need(r["mvd_max_x"] > 4096 and r["mvd_max_y"] > 1024, "|mvd| above 4096 across and above 1024 down")
    if name in CONTRAST or name in ALL_AT_ONCE:
        need(r["half1_clip0"] > 0 and r["half1_clip255"] > 0, "b / h half samples clipped at 0 and at 255")
        need(r["halfj_clip0"] > 0 and r["halfj_clip255"] > 0, "j half samples clipped at 0 and at 255")
    if name in POC or name in ALL_AT_ONCE and kw["weighted_bipred"] == 2:
        need(r["tbtd_clipped"] > 0, "tb or td clipped")
        need(r["implicit_fallback"] > 0, "a pair that fell back to 32 / 32")
        need(r["implicit_pairs"] > 0 and (r["implicit_w1_min"] < 0 or r["implicit_w1_max"] > 64), "a pair with w1 outside 0..64 that did not fall back")
    if name in POC_FIELD:
        need(r["tbtd_clipped"] > 0, "tb or td clipped")
        need(r["dsf_clipped"] > 0, "DistScaleFactor clipped")
        need(r["implicit_fallback"] > 0 and r["implicit_pairs"] > 0, "a pair that fell back to 32 / 32 and one that did not")
    if name in SCALING or name in ALL_AT_ONCE:
        want = ["absent_first", "absent_next", "use_default", "cut_short", "wrap", "entry_1", "entry_255", "full"]
        want += ["sps_matrix"] if kw["scaling_matrix"] == 2 else ["sps_matrix", "pps_rule_a", "pps_rule_b"]
        if kw["scaling_matrix"] == 3 and kw["frames"] > 2 * kw["idr_period"]:
            want += ["pps_six_lists"]
        for f in want:
            need(r["scaling_forms"] & forms[f], "scaling list form " + f)
    return bad
