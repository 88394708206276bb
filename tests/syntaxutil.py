"""Recipes of tests/test_entropy_syntax.py: generator streams that take the entropy stage to the ends of its syntax (streamgen's syntax_stim), and what
streamgen.last_syntax() must report for each of them and for each family of them.

The conditions are not measurements: the seeds were chosen on the CPU until the generator alone met them, and the CPU test asserts them, so that a
change to the generator cannot empty a recipe without a test failing.

Which entropy build of the product a stream reaches: I / P slices go to k_entropy (k_entropy_c when every slice of the launch is CABAC-coded), B slices
and everything coded with slice groups to k_entropy_b, field pictures to k_entropy_f.  A stream with B pictures has I and P pictures too; its recipes
set syntax_stim to 1 + 4, which leaves the stream alone and makes the counters count the B slices only."""

# Pictures are 48x32 .. 96x80 and there are at most 8 frames: the smallest shapes with interior, edge and corner macroblocks and two slices.
SMALL = dict(idr_period=0, frames=8, syntax_stim=1, intra_in_p_permille=250, skip_permille=120)
B = dict(SMALL, syntax_stim=5, bframes=3, num_ref_frames=2, bskip_permille=100, intra_in_p_permille=250)
FIELD = dict(SMALL, frames=6, field_pics=1, num_ref_frames=2)

# family -> recipes.  The families of one entropy mode and one build; every table entry is reached by the family as a whole (at most three recipes)
CAVLC_IP = {
    "cavlc_baseline_slices": dict(SMALL, width=96, height=80, profile_idc=66, cabac=0, qp=2, slices=3, seed=1),
    "cavlc_high_8x8_large": dict(SMALL, width=96, height=80, profile_idc=100, cabac=0, transform8x8=1, qp=1, slices=2, seed=2),
    "cavlc_main_pcm": dict(SMALL, width=80, height=64, profile_idc=77, cabac=0, qp=4, slices=2, pcm_permille=40, seed=3),
}
CAVLC_B = {
    "b_cavlc": dict(B, width=96, height=80, profile_idc=77, cabac=0, qp=2, slices=2, seed=24297),
    "b_cavlc_high_8x8_temporal": dict(B, width=96, height=80, profile_idc=100, cabac=0, transform8x8=1, qp=1, direct_temporal=1, seed=64044),
    "b_cavlc_ibp": dict(B, width=96, height=80, profile_idc=77, cabac=0, qp=3, bframes=1, slices=2, sub8x8_permille=300, seed=65037),
}
CAVLC_FIELD = {
    "field_cavlc": dict(FIELD, width=96, height=64, profile_idc=77, cabac=0, qp=2, slices=2, seed=7),
    "field_cavlc_high_8x8": dict(FIELD, width=96, height=64, profile_idc=100, cabac=0, transform8x8=1, qp=1, seed=8),
    "paff_cavlc": dict(FIELD, width=96, height=64, profile_idc=77, cabac=0, qp=3, field_pics=3, frames=8, seed=9),
}
CABAC_IP = {
    "cabac_main_slices": dict(SMALL, width=96, height=80, profile_idc=77, cabac=1, qp=2, slices=3, cabac_init_idc=-1, seed=10),
    "cabac_high_8x8_large": dict(SMALL, width=96, height=80, profile_idc=100, cabac=1, transform8x8=1, qp=1, slices=2, seed=11),
}
CABAC_B = {
    "b_cabac": dict(B, width=96, height=80, profile_idc=77, cabac=1, qp=2, slices=2, seed=12),
    "b_cabac_high_8x8": dict(B, width=96, height=80, profile_idc=100, cabac=1, transform8x8=1, qp=1, direct_temporal=1, seed=13),
}
CABAC_FIELD = {
    "field_cabac": dict(FIELD, width=96, height=64, profile_idc=77, cabac=1, qp=2, slices=2, seed=14),
    "field_cabac_high_8x8": dict(FIELD, width=96, height=64, profile_idc=100, cabac=1, transform8x8=1, qp=1, seed=15),
}
# Baseline with slice groups: I and P slices on the FMO route of the B build
FMO = {
    "fmo_cavlc_baseline": dict(SMALL, width=96, height=80, frames=6, profile_idc=66, cabac=0, qp=2, slice_groups=3, fmo_type=1, slices=2, aso=1, seed=16),
}
MONO = {
    "mono_cavlc": dict(SMALL, idr_period=3, intra_in_p_permille=400, width=96, height=80, profile_idc=100, mono=1, cabac=0, transform8x8=1, qp=3, slices=2, pcm_permille=30, seed=8371),
    "mono_cabac": dict(SMALL, idr_period=3, intra_in_p_permille=400, width=96, height=80, profile_idc=100, mono=1, cabac=1, transform8x8=1, qp=3, slices=2, pcm_permille=30, seed=18),
}
# mb_qp_delta at base QP 0, 26 and 51, chroma_qp_index_offset at both ends
QP_BASE = dict(SMALL, idr_period=2, intra_in_p_permille=400, skip_permille=60)
QP = {
    "qp0_cabac_offset_m12": dict(QP_BASE, width=96, height=80, profile_idc=77, cabac=1, qp=0, chroma_qp_offset=-12, slices=2, pcm_permille=60, seed=58477),
    "qp26_cavlc_8x8": dict(QP_BASE, width=96, height=80, profile_idc=100, cabac=0, transform8x8=1, qp=26, chroma_qp_offset=5, slices=2, pcm_permille=60, seed=74706),
    "qp51_cabac_8x8_offset_p12": dict(QP_BASE, width=96, height=80, profile_idc=100, cabac=1, transform8x8=1, qp=51, chroma_qp_offset=12, slices=2, pcm_permille=60,
                                      seed=3815),
    "qp51_cavlc_offset_m12": dict(QP_BASE, width=96, height=80, profile_idc=66, cabac=0, qp=51, chroma_qp_offset=-12, slices=2, pcm_permille=60, seed=5288),
}
SKIP_PCM = {
    "skip_pcm_cavlc": dict(SMALL, width=96, height=80, profile_idc=66, cabac=0, qp=6, slices=3, skip_permille=900, pcm_permille=100, intra_in_p_permille=50, seed=23),
    "skip_pcm_cabac": dict(SMALL, width=96, height=80, profile_idc=77, cabac=1, qp=6, slices=3, skip_permille=900, pcm_permille=100, intra_in_p_permille=50, seed=24),
    "skip_pcm_b_cabac": dict(B, width=96, height=80, profile_idc=77, cabac=1, qp=6, slices=3, bskip_permille=600, pcm_permille=100, intra_in_p_permille=50, seed=25),
}
# macroblocks of more than 3200 bits, kept (syntax_stim 2): the bit windows of the entropy kernels under every block full of large levels
OVERSIZE = {
    "oversized_cavlc_8x8": dict(SMALL, width=64, height=48, frames=4, syntax_stim=2, profile_idc=100, cabac=0, transform8x8=1, qp=1, slices=2, seed=26),
    "oversized_cabac_8x8": dict(SMALL, width=64, height=48, frames=4, syntax_stim=2, profile_idc=100, cabac=1, transform8x8=1, qp=1, slices=2, seed=27),
}
FAMILIES = dict(oversize=OVERSIZE, cavlc_ip=CAVLC_IP, cavlc_b=CAVLC_B, cavlc_field=CAVLC_FIELD, cabac_ip=CABAC_IP, cabac_b=CABAC_B, cabac_field=CABAC_FIELD, fmo=FMO, mono=MONO, qp=QP,
                skip_pcm=SKIP_PCM)
RECIPES = {}
for _family in FAMILIES.values():
    RECIPES.update(_family)
FAMILY_OF = {name: fam for fam, members in FAMILIES.items() for name in members}
# recipes that keep macroblocks of more than 3200 bits (syntax_stim 2); every other one stays within A.3.1
OVERSIZED = tuple(OVERSIZE)
# the I / P CABAC recipes: decoded alone they take k_entropy_c, next to a CAVLC stream k_entropy's CABAC path
CABAC_IP_ROUTED = sorted(n for n, kw in RECIPES.items() if kw["cabac"] and not kw.get("bframes") and not kw.get("field_pics") and not kw.get("slice_groups"))
# what test_gpu_batch_of_four_families puts into one batch, and the recipe with the densest residual (bytes per macroblock)
BATCH_OF_FOUR = ["cavlc_high_8x8_large", "cabac_high_8x8_large", "qp0_cabac_offset_m12", "skip_pcm_cabac"]
DENSEST = "qp0_cabac_offset_m12"


def pictures_of(kw):
    return kw["frames"] * (2 if kw.get("field_pics") else 1)


def slices_of(kw):
    return max(1, kw.get("slices", 1)) * max(1, kw.get("slice_groups", 1))


def decoder_cfg(kw):
    """field-coded blocks under CABAC use the unpinned context values: the product decodes them only when told to; B pictures need their frame pool"""
    cfg = dict(allow_unpinned_field_cabac=1) if kw.get("field_pics") and kw.get("cabac") else {}
    return cfg


# ---- the full tables ----
def _token_mask(max_coeff):
    return sum(1 << (4 * tc + t1) for tc in range(max_coeff + 1) for t1 in range(min(tc, 3) + 1))


TOKEN_FULL = [_token_mask(16)] * 4 + [_token_mask(4)]
TZ16_FULL = [(1 << (17 - tc)) - 1 for tc in range(1, 16)]          # tzVlcIndex 1..15: total_zeros 0 .. 16 - tzVlcIndex
TZ15_FULL = [(1 << (16 - tc)) - 1 for tc in range(1, 15)] + [0]    # AC blocks: 15 coefficients have no total_zeros
TZC_FULL = [(1 << (5 - tc)) - 1 for tc in range(1, 4)]
RUN_FULL = [(1 << (zl + 1)) - 1 for zl in range(1, 7)] + [0x7FFF]  # zerosLeft 1..6: run_before 0 .. zerosLeft; above 6: 0 .. 14


BITMAPS = ("p14_sl", "p15_sl", "p16_sl", "inc0_sat", "gt1_sat", "cbp_intra", "cbp_inter", "mbtype_i", "rem4", "rem8")


def _missing(have, full):
    return ["%d:%x" % (i, f & ~h) for i, (h, f) in enumerate(zip(have, full)) if f & ~h]


def union(counters):
    """the counters of several recipes as those of one stream: bitmaps or-ed, maxima and minima taken, counts added"""
    out = {}
    for c in counters:
        for k, v in c.items():
            if k not in out:
                out[k] = list(v) if isinstance(v, list) else v
            elif k in ("token", "tz16", "tz15", "tzc", "run", "cbf_inc"):
                out[k] = [a | b for a, b in zip(out[k], v)]
            elif k in BITMAPS:
                out[k] |= v
            elif k in ("dqp_min", "qpy_min"):
                out[k] = min(out[k], v)
            elif k.endswith("_max") or k == "level_max_cabac":
                out[k] = max(out[k], v)
            elif isinstance(v, list):
                out[k] = [a + b for a, b in zip(out[k], v)]
            else:
                out[k] += v
    return out


def unmet(name, c, family=None):
    """The conditions that recipe `name` does not meet: c = streamgen.last_syntax() of its stream; family = {recipe: counters} of all the recipes of its
    family, for the conditions that the family meets as a whole (left out: only the recipe's own are checked).  An empty list: all met."""
    kw, fam, bad = RECIPES[name], FAMILY_OF[name], []

    def need(cond, what):
        if not cond:
            bad.append(what)
    # ---- every stimulated recipe
    if name not in OVERSIZED:
        need(c["mb_bits_max"] <= 3200, "no macroblock above 3200 bits (largest: %d)" % c["mb_bits_max"])
    if kw["cabac"]:
        need(c["prefix_max"] == 0 and c["level_max"] == 0, "no CAVLC block in a CABAC stream")
    else:
        need(c["egk_max"] == 0 and sum(c["cat_blocks"]) == 0, "no CABAC block in a CAVLC stream")
        need(c["prefix_max"] <= (15 if kw["profile_idc"] != 100 else 25), "level_prefix above 15 outside the High profile")
    if family is None:
        return bad
    u = union(family.values())
    cats = [0, 1, 2] + ([] if kw.get("mono") else [3, 4]) + ([5] if any(RECIPES[n].get("transform8x8") for n in family) else [])
    if fam in ("cavlc_ip", "cavlc_b", "cavlc_field"):
        need(len(family) <= 3, "at most three recipes")
        need(not _missing(u["token"], TOKEN_FULL), "coeff_token entries (table:missing bits) %s" % _missing(u["token"], TOKEN_FULL))
        need(not _missing(u["tz16"], TZ16_FULL), "total_zeros of 4x4 blocks %s" % _missing(u["tz16"], TZ16_FULL))
        need(not _missing(u["tz15"], TZ15_FULL), "total_zeros of AC blocks %s" % _missing(u["tz15"], TZ15_FULL))
        need(not _missing(u["tzc"], TZC_FULL), "total_zeros of chroma DC %s" % _missing(u["tzc"], TZC_FULL))
        need(not _missing(u["run"], RUN_FULL), "run_before %s" % _missing(u["run"], RUN_FULL))
        need(u["p14_sl"] == 127 and u["p15_sl"] == 127, "level_prefix 14 and 15 at every suffixLength (missing %x, %x)" % (127 & ~u["p14_sl"], 127 & ~u["p15_sl"]))
        need(u["start_sl1"] > 0, "a block that starts at suffixLength 1")
        need(u["nc_one"] > 0 and u["nc_none"] > 0, "nC from one neighbour and from none")
        need(u["prefix_max"] >= 16 and u["level_max"] >= 2064, "level_prefix 16 with |level| >= 2064 (High)")
        need(u["cavlc_8x8_full"] > 0, "a CAVLC 8x8 block with 16 coefficients in every part")
        need(u["thinned"] > 0, "a macroblock coded again because it had more than 3200 bits")
    if fam in ("cabac_ip", "cabac_b", "cabac_field"):
        need(u["egk_max"] >= 11, "an Exp-Golomb suffix with k >= 11 (%d)" % u["egk_max"])
        for cat in cats:
            need(u["cat_blocks"][cat] > 0, "blocks of category %d" % cat)
            need(u["last_at_end"][cat] > 0, "category %d: last coefficient at the last scan position" % cat)
            need(u["all_nonzero"][cat] > 0, "category %d: a full block" % cat)
            need(u["inc0_sat"] >> cat & 1 and u["gt1_sat"] >> cat & 1, "category %d: both coeff_abs_level counters saturated" % cat)
            if cat < 5:
                need(u["cbf_inc"][cat] == 15, "category %d: all four coded_block_flag increments (missing %x)" % (cat, 15 & ~u["cbf_inc"][cat]))
        need(u["cbf_unavail_intra"] > 0 and u["cbf_unavail_inter"] > 0, "an unavailable neighbour in an intra and in an inter macroblock")
        need(u["thinned"] > 0, "a macroblock coded again because it had more than 3200 bits")
    if fam == "qp":
        need(u["dqp_min"] == -26 and u["dqp_max"] == 25, "mb_qp_delta -26 and +25")
        need(u["dqp_wrap_up"] > 0 and u["dqp_wrap_down"] > 0, "a wrap in each direction")
        need(u["qpy_min"] == 0 and u["qpy_max"] == 51, "QP_Y 0 and 51")
        need(u["qpc_clip0"] > 0 and u["qpc_clip51"] > 0, "chroma QP clipped at both ends")
        need(u["dqp_after_skip"] > 0 and u["dqp_after_pcm"] > 0 and u["dqp_after_nodelta"] > 0, "a non-zero delta after a skipped, an I_PCM and a delta-less macroblock")
        full48 = sum(1 << (l | ch << 4) for l in range(16) for ch in range(3))
        need(u["cbp_intra"] == full48 and u["cbp_inter"] == full48, "all 48 coded_block_pattern values, intra and inter (missing %x, %x)"
             % (full48 & ~u["cbp_intra"], full48 & ~u["cbp_inter"]))
        need(u["mbtype_i"] == (1 << 26) - 1, "all 26 mb_type values of I slices (missing %x)" % (((1 << 26) - 1) & ~u["mbtype_i"]))
        need(u["rem4"] == 511 and u["rem8"] == 511, "all rem_intra values and the predicted mode, 4x4 and 8x8 (missing %x, %x)" % (511 & ~u["rem4"], 511 & ~u["rem8"]))
    if fam == "mono":
        for n, cc in family.items():
            need(cc["cbp_intra"] == 0xFFFF and cc["cbp_inter"] == 0xFFFF, "%s: all 16 coded_block_pattern values, intra and inter (missing %x, %x)" % (n, 0xFFFF & ~cc["cbp_intra"], 0xFFFF & ~cc["cbp_inter"]))
    if fam == "oversize":
        need(c["mb_bits_max"] > 3200, "a macroblock above 3200 bits (largest: %d)" % c["mb_bits_max"])
    if fam == "skip_pcm":
        for n, cc in family.items():
            wmb = (RECIPES[n]["width"] + 15) // 16
            need(cc["skip_run_max"] > wmb, "%s: a run of skipped macroblocks longer than a row (%d)" % (n, cc["skip_run_max"]))
            need(cc["end_in_skip"] > 0, "%s: a slice ending in a skip run" % n)
            if RECIPES[n]["cabac"]:
                need(cc["end_in_pcm"] > 0, "%s: a slice ending in I_PCM under CABAC" % n)
    return bad
